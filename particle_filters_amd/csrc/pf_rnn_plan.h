// The shape plan of the RNN resampler's recurrence kernel (pf_rnn_kernels.h: k_rnn_recur): padded
// sizes, workgroup and grid, the LDS it needs and whether the weights live there.  A pure host
// function of (N, d, H, L, cell type), checked stand-alone by tests/host/pf_rnn_plan_host_check.cpp.
//
// Sizes.  A workgroup owns RT = 16 target particles (the rows of v_mfma_f64_16x16x4_f64) of one
// problem.  The hidden units are cut into HT = ceil(H / 16) tiles of 16 (the columns of one MFMA
// result); Hp = 16 HT is the padded number of units and KS = ceil(H / 4) the number of MFMA k-steps
// of a product with a hidden state.  A tile belongs to RS waves (4 for HT = 1, 2 for HT = 2, else 1),
// which all form the tile's products - they are cheap - and share the gate update, the expensive
// part, by rows: of the 4 rows a lane's accumulator holds, a wave updates 4 / RS.  So the four SIMDs
// of a CU are busy from H = 1 on.
//
// Each unit has SLOTS = 4 pre-activation columns (LSTM: the gates i, f, c, o; GRU: z, r, the input half of h, the recurrent half of h), so
// a row of pre-activations has 4 Hp entries.
//
// Weight fragments.  A weight matrix of K = 4 KS rows by 4 Hp columns is stored in the order the
// MFMA B operand is fetched: fragment (tile, ks, slot) is 64 doubles, lane l holding the entry of row
// 4 ks + (l >> 4) and column slot Hp + 16 tile + (l & 15).  Layer l has one such matrix for the
// recurrent kernel and, for l > 0, one for the input kernel: (2 L - 1) HT KS 4 fragments in all.
//
// LDS.  The hidden states, two time parities per layer, k-major with a row stride of HS = 18 doubles
// (16 rows and 2 of padding): 2 L Hp HS doubles.  Resident: the weight fragments behind them.  The
// plan is resident when both fit into the 160 KiB of a CU, otherwise the kernel streams the
// fragments from global memory (through L2) at every timestep.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pf {
namespace rnn {

constexpr int RT = 16;        // target particles per workgroup
constexpr int SLOTS = 4;      // pre-activation columns per hidden unit
constexpr int HS = 18;        // LDS stride, in doubles, of one hidden unit's 16 rows
constexpr int MAXH = 128, MAXL = 4;  // dim and batch: MAXDIM, MAXBATCH of pf_dpf_host.h
constexpr int64_t MAXPAIRS = (int64_t)1 << 28;  // B N N
constexpr size_t LDS_CU_BYTES = 160 * 1024;
constexpr int CELL_LSTM = 0, CELL_GRU = 1;

struct Plan {
  int HT, Hp, KS;           // unit tiles, padded units, k-steps
  int RS;                   // waves per unit tile
  int threads;              // 64 HT RS
  int tiles;                // ceil(N / 16): grid.x (grid.y = B)
  int F0;                   // per-particle features of layer 0 (without the one-hot block)
  size_t frag_doubles;      // all weight fragments
  size_t state_doubles;     // hidden states in LDS
  size_t lds_bytes;         // what the kernel is launched with
  bool resident;
};

// the offset, in doubles, of fragment (tile, ks, slot) of matrix m: m = 2 l for the recurrent kernel
// of layer l, 2 l - 1 for the input kernel of layer l > 0
inline size_t frag_offset(const Plan& p, int m, int tile, int ks, int slot) {
  return ((((size_t)m * p.HT + tile) * p.KS + ks) * SLOTS + slot) * 64;
}

inline Plan make_plan(int64_t N, int d, int H, int L, int cell, bool use_weight = true, bool use_particle = true,
                      bool force_stream = false) {
  (void)cell;  // both cells use four slots per unit
  Plan p{};
  p.HT = (H + 15) / 16;
  p.Hp = 16 * p.HT;
  p.KS = (H + 3) / 4;
  p.RS = p.HT == 1 ? 4 : p.HT == 2 ? 2 : 1;
  p.threads = 64 * p.HT * p.RS;
  p.tiles = (int)((N + RT - 1) / RT);
  p.F0 = (use_weight ? 1 : 0) + (use_particle ? d : 0);
  p.frag_doubles = (size_t)(2 * L - 1) * p.HT * p.KS * SLOTS * 64;
  p.state_doubles = (size_t)2 * L * p.Hp * HS;
  const size_t all = (p.state_doubles + p.frag_doubles) * sizeof(double);
  p.resident = !force_stream && all <= LDS_CU_BYTES;
  p.lds_bytes = p.resident ? all : p.state_doubles * sizeof(double);
  return p;
}

}  // namespace rnn
}  // namespace pf
