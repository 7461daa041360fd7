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

// ---- The packing of the Keras arrays, as index maps -------------------------------------------------
// What pf_rnn_set_weights builds, stated once per destination element: where it comes from in the
// n = 3 L + 2 arrays (kernel, recurrent_kernel, bias per layer, then the output kernel and bias), or
// that it is zero.  k_rnn_pack / k_rnn_pack_T (pf_rnn_kernels.h) evaluate them on the device, one
// thread per destination element; tests/host/pf_rnn_pack_check.cpp evaluates them on the host against
// the packing loops.  Everything is a copy but the GRU's z and r biases, which are the sum of the
// input and the recurrent bias (idx2).
#ifdef __HIP__
#define PF_RNN_HD __host__ __device__
#else
#define PF_RNN_HD
#endif

struct PackNet {
  int N, H, L, cell, F0, Hp, HT, KS;
};
inline PackNet pack_net(const Plan& p, int N, int H, int L, int cell) {
  return PackNet{N, H, L, cell, p.F0, p.Hp, p.HT, p.KS};
}

struct PackSrc {
  int arr;       // the source array, or -1: the element is zero
  int64_t idx;   // its element
  int64_t idx2;  // >= 0: a second element of the same array, added to the first
};

// the gate whose column block feeds `slot` of the input kernel (rec = false) or the recurrent kernel
// (rec = true), or -1: LSTM i, f, c, o; GRU z, r, the input half of h (slot 2), the recurrent half (3)
PF_RNN_HD inline int pack_gate(int cell, int slot, bool rec) {
  if (cell == CELL_LSTM) return slot;
  if (slot < 2) return slot;
  return (slot == 3) == rec ? 2 : -1;
}

PF_RNN_HD inline PackSrc pack_zero() { return PackSrc{-1, 0, -1}; }

// rows of layer 0's kernel: W0x [F0][4 Hp] (row = feature f) and W0i [N][4 Hp] (row = F0 + i)
PF_RNN_HD inline PackSrc pack_src_k0(const PackNet& n, int64_t row, int col) {
  const int G = n.cell == CELL_LSTM ? 4 : 3, slot = col / n.Hp, u = col - slot * n.Hp;
  const int g = pack_gate(n.cell, slot, false);
  if (g < 0 || u >= n.H) return pack_zero();
  return PackSrc{0, row * ((int64_t)G * n.H) + (int64_t)g * n.H + u, -1};
}
PF_RNN_HD inline PackSrc pack_src_W0x(const PackNet& n, int64_t e) {
  const int W4 = SLOTS * n.Hp;
  return pack_src_k0(n, e / W4, (int)(e % W4));
}
PF_RNN_HD inline PackSrc pack_src_W0i(const PackNet& n, int64_t e) {
  const int W4 = SLOTS * n.Hp;
  return pack_src_k0(n, n.F0 + e / W4, (int)(e % W4));
}
// binit [L][4 Hp]
PF_RNN_HD inline PackSrc pack_src_binit(const PackNet& n, int64_t e) {
  const int W4 = SLOTS * n.Hp, l = (int)(e / W4), col = (int)(e % W4), slot = col / n.Hp, u = col - slot * n.Hp;
  if (u >= n.H) return pack_zero();
  const int64_t H = n.H;
  if (n.cell == CELL_LSTM) return PackSrc{3 * l + 2, slot * H + u, -1};
  if (slot < 2) return PackSrc{3 * l + 2, slot * H + u, 3 * H + slot * H + u};
  return PackSrc{3 * l + 2, (slot == 2 ? 2 * H : 5 * H) + u, -1};
}
// the entry of row k (an input unit) and unit u in slot `slot` of matrix m (frag_offset's m)
PF_RNN_HD inline PackSrc pack_src_entry(const PackNet& n, int m, int slot, int k, int u) {
  const int G = n.cell == CELL_LSTM ? 4 : 3, rec = (m & 1) == 0, l = (m + 1) >> 1;
  const int g = pack_gate(n.cell, slot, rec);
  if (g < 0 || k >= n.H || u >= n.H) return pack_zero();
  return PackSrc{3 * l + rec, (int64_t)k * G * n.H + (int64_t)g * n.H + u, -1};
}
// frag: fragment (m, tile, ks, slot), lane l holds row 4 ks + (l >> 4), unit 16 tile + (l & 15)
PF_RNN_HD inline PackSrc pack_src_frag(const PackNet& n, int64_t e) {
  const int lane = (int)(e & 63), slot = (int)((e >> 6) % SLOTS);
  const int64_t r = (e >> 6) / SLOTS;
  const int ks = (int)(r % n.KS), tile = (int)((r / n.KS) % n.HT), m = (int)(r / n.KS / n.HT);
  return pack_src_entry(n, m, slot, 4 * ks + (lane >> 4), 16 * tile + (lane & 15));
}
// fragT, the transposed set of the backward pass, as a permutation of frag: fragment (m, tile, ks,
// slot) holds in lane l the entry (k, u) = (16 tile + (l & 15), 4 ks + (l >> 4)), which frag keeps in
// fragment (m, u / 16, k / 4, slot), lane 16 (k % 4) + u % 16.  Returns that element of frag, or -1:
// rows k >= 4 KS are rows of padded units, zero.
PF_RNN_HD inline int64_t pack_fragT_from_frag(const PackNet& n, int64_t e) {
  const int lane = (int)(e & 63), slot = (int)((e >> 6) % SLOTS);
  const int64_t r = (e >> 6) / SLOTS;
  const int ks = (int)(r % n.KS), tile = (int)((r / n.KS) % n.HT), m = (int)(r / n.KS / n.HT);
  const int k = 16 * tile + (lane & 15), u = 4 * ks + (lane >> 4);
  if (k >= 4 * n.KS) return -1;
  return (((((int64_t)m * n.HT + u / 16) * n.KS + k / 4) * SLOTS + slot) << 6) + 16 * (k % 4) + u % 16;
}

}  // namespace rnn
}  // namespace pf
