// The plan of the RNN resampler's backward pass (pf_rnn_backward; kernels in pf_rnn_kernels.h): the
// device workspace, the LDS of the backward recurrence and whether its weight fragments live there,
// and the split of the weight-gradient reductions.  A pure host function of the forward plan
// (pf_rnn_plan.h) and (N, d, B, H, L, cell), checked stand-alone by
// tests/host/pf_rnn_bwd_plan_host_check.cpp.
//
// History.  The recording forward writes h_l(t), and for the LSTM c_l(t), of every (b, i, t, l); the
// backward sweep writes the four slot deltas dz_l(t).  All three are stored as blocks, one per
// (b, row tile, t, l), in the layout the MFMA operands are fetched in:
//   block (b, tile, t, l) = ((b tiles + tile) N + t) L + l
//   h, c: [Hp units][16 rows]   dz: [4 Hp columns][16 rows]
// which is B tiles N L 16 Hp doubles for h (and c), four times that for dz: the B N^2 L Hp growth.
//
// LDS of k_rnn_bwd_recur.  Three staging areas, k-major with the forward's row stride HS:
// h_l(t-1) and h_{l-1}(t), Hp units each, and dz, 4 Hp columns: 6 Hp HS doubles.  Resident: behind
// them the forward's weight fragments (the pre-activations are re-formed) and the transposed ones
// (the push back), 2 frag_doubles.  Resident when all of it fits a CU's 160 KiB, otherwise both sets
// of fragments are streamed from global memory at every (t, l).
//
// Weight gradients.  g R_l and g K_l are GEMMs whose reduction runs over the N^2 pairs (i, t) of a
// problem.  The timesteps are cut into wg_chunks chunks of wg_tc (the last may be shorter); a wave
// reduces one chunk, all row tiles, for one 16 x 16 tile of one matrix into a partial, and the finish
// kernel adds the partials in ascending chunk, then the problems in ascending b.  The split depends
// on N alone, so every sum has an order fixed by (N, d, H, L).
#pragma once
#include <cstddef>
#include <cstdint>

#include "pf_rnn_plan.h"

namespace pf {
namespace rnn {

constexpr int WG_MIN_TC = 8;       // about this many timesteps per chunk of the weight-gradient GEMMs, or more
constexpr int WG_MAX_CHUNKS = 64;  // and at most this many chunks

struct BwdPlan {
  size_t blocks;           // B tiles N L history blocks
  size_t hist_doubles;     // of h, and of c for the LSTM (0 for the GRU)
  size_t c_doubles;
  size_t dz_doubles;
  size_t stage_doubles;    // LDS staging areas of k_rnn_bwd_recur
  size_t lds_bytes;        // what k_rnn_bwd_recur is launched with
  bool resident;           // both sets of fragments in LDS
  int wg_tc, wg_chunks;    // timesteps per chunk, chunks
  int mats;                // 2 L - 1 matrices with fragments
  size_t part_doubles;     // B mats wg_chunks Hp 4 Hp
  size_t sums_doubles;     // S [B][N][L][4 Hp]: dz summed over the rows of a problem
  size_t w0i_doubles;      // [B][N][4 Hp]: dz of layer 0 summed over t
  size_t k0x_doubles;      // [B][F0][4 Hp]
  size_t dense_doubles;    // [B][H + 1][N]: g Kd and g bd per problem
  size_t pair_doubles;     // [B][N][N]: grad_A in, gz out
  size_t vec_doubles;      // grad_X_out, grad_X [B][N][d] each, g hid [B][N][H], grad_w [B][N]
  size_t out_doubles;      // the 3 L + 2 Keras arrays, concatenated
  size_t workspace_bytes;  // everything the first backward call allocates
};

// the block of (b, tile, t, l); times 16 Hp (h, c) or 64 Hp (dz) doubles
inline size_t hist_block(int tiles, int64_t N, int L, int b, int tile, int64_t t, int l) {
  return (((size_t)b * tiles + tile) * (size_t)N + (size_t)t) * L + l;
}

// the sizes of the Keras arrays, in their order; returns their sum
inline size_t keras_sizes(int64_t N, int F0, int H, int L, int cell, int64_t* sizes /* [3 L + 2] */) {
  const int G = cell == CELL_LSTM ? 4 : 3;
  size_t all = 0;
  for (int l = 0; l < L; ++l) {
    sizes[3 * l] = (int64_t)(l == 0 ? F0 + N : H) * G * H;
    sizes[3 * l + 1] = (int64_t)H * G * H;
    sizes[3 * l + 2] = (int64_t)(cell == CELL_LSTM ? 4 : 6) * H;
    all += sizes[3 * l] + sizes[3 * l + 1] + sizes[3 * l + 2];
  }
  sizes[3 * L] = (int64_t)H * N;
  sizes[3 * L + 1] = N;
  return all + (size_t)H * N + N;
}

inline BwdPlan make_bwd_plan(const Plan& p, int64_t N, int d, int B, int H, int L, int cell,
                             bool force_stream = false) {
  BwdPlan q{};
  const size_t W4 = (size_t)SLOTS * p.Hp;
  q.blocks = (size_t)B * p.tiles * (size_t)N * L;
  q.hist_doubles = q.blocks * RT * p.Hp;
  q.c_doubles = cell == CELL_LSTM ? q.hist_doubles : 0;
  q.dz_doubles = q.blocks * RT * W4;
  q.stage_doubles = (size_t)6 * p.Hp * HS;
  const size_t all = (q.stage_doubles + 2 * p.frag_doubles) * sizeof(double);
  q.resident = !force_stream && all <= LDS_CU_BYTES;
  q.lds_bytes = q.resident ? all : q.stage_doubles * sizeof(double);
  int chunks = (int)((N + WG_MIN_TC - 1) / WG_MIN_TC);
  if (chunks > WG_MAX_CHUNKS) chunks = WG_MAX_CHUNKS;
  q.wg_tc = (int)((N + chunks - 1) / chunks);
  q.wg_chunks = (int)((N + q.wg_tc - 1) / q.wg_tc);
  q.mats = 2 * L - 1;
  q.part_doubles = (size_t)B * q.mats * q.wg_chunks * p.Hp * W4;
  q.sums_doubles = (size_t)B * N * L * W4;
  q.w0i_doubles = (size_t)B * N * W4;
  q.k0x_doubles = (size_t)B * p.F0 * W4;
  q.dense_doubles = (size_t)B * (H + 1) * N;
  q.pair_doubles = (size_t)B * N * N;
  q.vec_doubles = (size_t)2 * B * N * d + (size_t)B * N * H + (size_t)B * N;
  int64_t sizes[3 * MAXL + 2];
  q.out_doubles = keras_sizes(N, p.F0, H, L, cell, sizes);
  q.workspace_bytes = (q.hist_doubles + q.c_doubles + q.dz_doubles + p.frag_doubles + q.part_doubles + q.sums_doubles +
                       q.w0i_doubles + q.k0x_doubles + q.dense_doubles + q.pair_doubles + q.vec_doubles + q.out_doubles) *
                      sizeof(double);
  return q;
}

}  // namespace rnn
}  // namespace pf
