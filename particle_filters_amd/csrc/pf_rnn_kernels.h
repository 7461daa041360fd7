// Device side of the RNN resampler (pf_rnn_* of include/pf_engine.h; host side pf_rnn.hip, shape
// plan pf_rnn_plan.h).
//
// One resampling of models/DPF_RNN_resampling.py ("rnn.py":263-349) for B independent problems of
// N particles in d dimensions, fp64; the backward pass is the second half of this file.  For each of the N new particles i the reference
// runs a fresh L-layer LSTM / GRU over the N old particles j = 0..N-1, the input of timestep j being
// [w_j, x_j, onehot(i)], and maps the last hidden state of the top layer to a row of assignment
// logits.  The one-hot block is constant along a sequence, so
//   x_t^(i) kernel0 = feat_t kernel0[:F0] + kernel0[F0 + i]:
// the first term is shared by all N sequences of a problem (k_rnn_project forms it once, biases
// included), the second is a per-sequence constant the recurrence keeps in registers.
//   k_rnn_project  P[b][t][4 Hp] = feat[b][t] kernel0[:F0] + the initial pre-activations of layer 0
//   k_rnn_recur    one launch: a workgroup owns 16 sequences (target particles) of one problem, the
//                  rows of v_mfma_f64_16x16x4_f64, and walks t = 0..N-1 over all layers.  A wave owns
//                  16 hidden units of every layer and all four pre-activation slots of them: after
//                  the products a lane holds, for 4 rows and one unit, every gate, so the cell
//                  update needs no exchange.  With H <= 32 a unit tile has RS = 4 or 2 waves, which
//                  repeat the products and each update 4 / RS of the 4 rows, so that all four SIMDs
//                  share the fp64 activations, the expensive part of a step.  The new h goes to LDS k-major, which
//                  is the A-operand layout, one barrier per (timestep, layer); two time parities per
//                  layer make that barrier the only one.  The weight fragments (pf_rnn_plan.h) are
//                  copied to LDS once (RES) or read from global memory at every step.
//   k_rnn_assign   one workgroup per new particle: logits = hid Kd + bd times 1 / T (or, for the
//                  baseline resampler of rnn.py:217-261, lp_j + 0.1 G_ij with the Philox Gumbels of
//                  pf_soft_draws.h), the row softmax, A written, X'_i = sum_j A_ij X_j.
//
// Padding.  Units H .. Hp - 1 have zero weights and zero biases in every matrix, so their
// pre-activations are exactly 0 at every step, and with the state starting at 0:
//   LSTM: c' = sigma(0) c + sigma(0) tanh(0) = 0.5 * 0 + 0.5 * 0 = 0,  h' = sigma(0) tanh(0) = 0;
//   GRU:  hh = tanh(0 + sigma(0) * 0) = 0,  h' = 0.5 * 0 + 0.5 * 0 = 0.
// A padded unit therefore stays exactly 0, and it meets only zero weight rows as an input.  A padding
// row (i >= N) computes row N - 1 again and stores nothing.
//
// No floating-point atomics, no grid-wide barrier; every sum has an order fixed by (N, d, H, L): two
// calls are bitwise equal, and a problem has the same bits in a batch and alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pf_rnn_bwd_plan.h"
#include "pf_rnn_plan.h"
#include "pf_soft_draws.h"

namespace pf {
namespace rnn {

typedef double dbl4 __attribute__((ext_vector_type(4)));

constexpr int PB = 256;  // lanes per workgroup of k_rnn_project and k_rnn_assign
constexpr double BASELINE_NOISE = 0.1;  // rnn.py:253

struct ProjArgs {
  int N, d, W4, F0, use_weight, use_particle;
  const double* X;      // [B][N][d]
  const double* w;      // [B][N]
  const double* W0x;    // [F0][W4]
  const double* binit;  // [W4] of layer 0
  double* P;            // [B][N][W4]
};

// grid (ceil(W4 / PB), N, B)
__global__ void __launch_bounds__(PB) k_rnn_project(ProjArgs a) {
  const int col = blockIdx.x * PB + threadIdx.x;
  if (col >= a.W4) return;
  const int t = blockIdx.y, b = blockIdx.z;
  const size_t bt = (size_t)b * a.N + t;
  double v = a.binit[col];
  int f = 0;
  if (a.use_weight) v = fma(a.w[bt], a.W0x[col], v), f = 1;
  if (a.use_particle) {
    const double* __restrict__ x = a.X + bt * a.d;
    for (int c = 0; c < a.d; ++c) v = fma(x[c], a.W0x[(size_t)(f + c) * a.W4 + col], v);
  }
  a.P[bt * a.W4 + col] = v;
}

struct RecurArgs {
  int N, H, Hp, HT, KS, RS;
  const double* P;      // [B][N][4 Hp]
  const double* W0i;    // [N][4 Hp]: the one-hot rows of layer 0's kernel
  const double* binit;  // [L][4 Hp]: initial pre-activations (layer 0's are in P)
  const double* frag;   // weight fragments (pf_rnn_plan.h)
  size_t frag_doubles;
  double* hid;          // [B][N][H]
  double* rec_h;        // REC only: h_l(t) of every (b, i, t, l), the blocks of pf_rnn_bwd_plan.h
  double* rec_c;        // REC only, LSTM: c_l(t), the same blocks
};

// hist_block of pf_rnn_bwd_plan.h on the device
__device__ __forceinline__ size_t hblock(int tiles, int N, int L, int b, int tile, int t, int l) {
  return (((size_t)b * tiles + tile) * (size_t)N + (size_t)t) * L + l;
}

__device__ __forceinline__ double sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// acc[s] += hs (16 x 4 KS, k-major in LDS) times the fragments of matrix m, for the slots in mask
template <int MASK>
__device__ __forceinline__ void accumulate(dbl4 (&acc)[SLOTS], const double* hs, const double* __restrict__ fr, int KS,
                                           int lane) {
  const int r16 = lane & 15, kq = lane >> 4;
  for (int ks = 0; ks < KS; ++ks) {
    const double aop = hs[(4 * ks + kq) * HS + r16];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
      if (MASK & (1 << s)) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, fr[(ks * SLOTS + s) * 64 + lane], acc[s], 0, 0, 0);
  }
}

// grid (ceil(N / 16), B), 64 HT RS lanes, dynamic LDS of Plan::lds_bytes.  REC is the recording variant of
// pf_rnn_backward: the same arithmetic, and every new h (and c) also goes to the history; with REC off
// no code is added.
template <int CELL, int L, bool RES, bool REC = false>
__global__ void __launch_bounds__(64 * (MAXH / 16)) k_rnn_recur(RecurArgs a) {
  extern __shared__ double rnn_lds[];
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
  const int tile = (tid >> 6) / a.RS, sub = (tid >> 6) - tile * a.RS;  // wave sub updates the rows r with r RS / 4 == sub
  const int b = blockIdx.y, i0 = blockIdx.x * RT;
  const int N = a.N, Hp = a.Hp, KS = a.KS, W4 = SLOTS * a.Hp;
  const int nstate = 2 * L * Hp * HS, lstate = Hp * HS;
  double* hst = rnn_lds;  // [L][2][Hp][HS]
  for (int q = tid; q < nstate; q += blockDim.x) hst[q] = 0.0;
  const double* fr_all = a.frag;
  if (RES) {
    double* wl = rnn_lds + nstate;
    for (size_t q = tid; q < a.frag_doubles; q += blockDim.x) wl[q] = a.frag[q];
    fr_all = wl;
  }
  __syncthreads();
  const int u = 16 * tile + r16;  // the unit this lane owns, for the rows kq + 4 r
  const size_t mat = (size_t)a.HT * KS * SLOTS * 64, mine = (size_t)tile * KS * SLOTS * 64;

  dbl4 R0[SLOTS];  // kernel0[F0 + i] of the own rows: constant over t
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = min(i0 + kq + 4 * r, N - 1);
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) R0[s][r] = a.W0i[(size_t)row * W4 + s * Hp + u];
  }
  double bl[L][SLOTS];
#pragma unroll
  for (int l = 0; l < L; ++l)
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) bl[l][s] = a.binit[(size_t)l * W4 + s * Hp + u];
  dbl4 own[L];  // LSTM: c; GRU: h, of the own (rows, unit)
#pragma unroll
  for (int l = 0; l < L; ++l) own[l] = dbl4{0.0, 0.0, 0.0, 0.0};
  dbl4 h = {0.0, 0.0, 0.0, 0.0};

  const double* __restrict__ Pb = a.P + (size_t)b * N * W4 + u;
  double pn[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) pn[s] = Pb[s * Hp];
  // slots fed by the input kernel / by the recurrent kernel (pf_rnn_plan.h)
  constexpr int IN_MASK = CELL == CELL_LSTM ? 15 : 7, REC_MASK = CELL == CELL_LSTM ? 15 : 11;

  for (int t = 0; t < N; ++t) {
    const int par = t & 1;
    double pc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) pc[s] = pn[s];
    if (t + 1 < N) {  // the next step's shared pre-activations, in flight during this step
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) pn[s] = Pb[(size_t)(t + 1) * W4 + s * Hp];
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {
      dbl4 acc[SLOTS];
      if (l == 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) acc[s] = R0[s] + pc[s];
      } else {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) acc[s] = dbl4{bl[l][s], bl[l][s], bl[l][s], bl[l][s]};
        accumulate<IN_MASK>(acc, hst + (size_t)(2 * (l - 1) + par) * lstate, fr_all + (2 * l - 1) * mat + mine, KS, lane);
      }
      accumulate<REC_MASK>(acc, hst + (size_t)(2 * l + (par ^ 1)) * lstate, fr_all + (2 * l) * mat + mine, KS, lane);
      double* hw = hst + (size_t)(2 * l + par) * lstate + u * HS + kq;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r * a.RS / 4 != sub) continue;  // another wave's row (a wave-uniform branch)
        if (CELL == CELL_LSTM) {
          const double c = sigmoid(acc[1][r]) * own[l][r] + sigmoid(acc[0][r]) * tanh(acc[2][r]);
          own[l][r] = c;
          h[r] = sigmoid(acc[3][r]) * tanh(c);
        } else {
          const double z = sigmoid(acc[0][r]), rr = sigmoid(acc[1][r]);
          const double hh = tanh(acc[2][r] + rr * acc[3][r]);
          h[r] = z * own[l][r] + (1.0 - z) * hh;
          own[l][r] = h[r];
        }
        hw[4 * r] = h[r];
        if (REC && i0 + kq + 4 * r < N) {  // a padding row records nothing
          const size_t at = hblock(gridDim.x, N, L, b, blockIdx.x, t, l) * RT * Hp + u * RT + kq + 4 * r;
          a.rec_h[at] = h[r];
          if (CELL == CELL_LSTM) a.rec_c[at] = own[l][r];
        }
      }
      __syncthreads();  // h_l(t) is complete: layer l + 1 reads it now, layer l at t + 1
    }
  }
  if (u < a.H) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + kq + 4 * r;
      if (i < N && r * a.RS / 4 == sub) a.hid[((size_t)b * N + i) * a.H + u] = h[r];
    }
  }
}

// fixed-order butterfly over the 64 lanes; every lane ends with the same value
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}

struct AssignArgs {
  int N, d, H;
  const double* hid;  // [B][N][H]           (RNN)
  const double* Kd;   // [H][N]              (RNN)
  const double* bd;   // [N]                 (RNN)
  double inv_T;       //                     (RNN)
  const double* lp;   // [B][N]              (baseline)
  soft::Prob p;       //                     (baseline)
  const double* X;    // [B][N][d]
  double* A;          // [B][N][N]
  double* X_out;      // [B][N][d]
};

// grid (N, B), PB lanes: row i of problem b
template <bool BASELINE>
__global__ void __launch_bounds__(PB) k_rnn_assign(AssignArgs a) {
  __shared__ double sh[MAXH], red[PB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x, b = blockIdx.y, N = a.N, d = a.d;
  double* __restrict__ Ai = a.A + ((size_t)b * N + i) * N;
  if (!BASELINE) {
    for (int q = tid; q < a.H; q += PB) sh[q] = a.hid[((size_t)b * N + i) * a.H + q];
    __syncthreads();
  }
  const uint32_t w3 = soft::stream_word(a.p, b);
  double mx = -INFINITY;
  for (int j = tid; j < N; j += PB) {
    double z;
    if (BASELINE) {
      const u32x4 r = soft::pair_words(a.p, w3, (uint32_t)j >> 1, (uint32_t)i);
      const double un = (j & 1) ? soft::soft_uniform(r.z, r.w) : soft::soft_uniform(r.x, r.y);
      z = a.lp[(size_t)b * N + j] + BASELINE_NOISE * soft::gumbel(un);
    } else {
      z = a.bd[j];
      for (int q = 0; q < a.H; ++q) z = fma(sh[q], a.Kd[(size_t)q * N + j], z);
      z *= a.inv_T;
    }
    Ai[j] = z;
    mx = fmax(mx, z);
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  double sum = 0.0;
  for (int j = tid; j < N; j += PB) {  // the lane's own entries
    const double e = exp(Ai[j] - mx);
    Ai[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  sum = (red[0] + red[1]) + (red[2] + red[3]);
  for (int j = tid; j < N; j += PB) Ai[j] = Ai[j] / sum;
  __threadfence_block();
  __syncthreads();  // the row is complete and visible to the workgroup
  const double* __restrict__ Xb = a.X + (size_t)b * N * d;
  for (int c = wave; c < d; c += PB / 64) {
    double v = 0.0;
    for (int j = lane; j < N; j += 64) v = fma(Ai[j], Xb[(size_t)j * d + c], v);
    v = wave_sum(v);
    if (lane == 0) a.X_out[((size_t)b * N + i) * d + c] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// The backward pass (pf_rnn_backward).  Given grad_X_out and grad_A at (X, w, T) it returns the
// gradients of sum gXo . X' + sum gA . A: to X, to w and to every weight array.  The chain, after
// the recording forward (k_rnn_project, k_rnn_recur<REC>, k_rnn_assign):
//   k_rnn_bwd_assign  one workgroup per row i: G_ij = gA_ij + gXo_i . X_j, gz_ij = A_ij (G_ij -
//                     sum_k A_ik G_ik) / T (in place over gA), g hid_i = sum_j gz_ij Kd[:, j]
//   k_rnn_bwd_cols    a lane per column j, i ascending: the direct term of grad_X, g bd, g Kd
//   k_rnn_bwd_recur   back-propagation through time, one launch: t = N-1 .. 0, l = L-1 .. 0; writes
//                     the slot deltas dz_l(t) of every (b, i, t, l)
//   k_rnn_bwd_sums    S[b][t][l] = sum_i dz_l(t): layer 0's is gP, the gradient of the projection;
//                     summed over t they are the biases
//   k_rnn_bwd_w0i     sum_t dz_0(t) of a row: the gradient of the one-hot row kernel0[F0 + i]
//   k_rnn_bwd_wgrad   g R_l = sum h_l(t-1)^T dz_l(t), g K_l = sum h_{l-1}(t)^T dz_l(t) as MFMA
//                     partials over chunks of t (pf_rnn_bwd_plan.h)
//   k_rnn_bwd_k0x     g kernel0[:F0] per problem = sum_t feat_t^T gP[t]
//   k_rnn_bwd_feat    g feat[t] = gP[t] kernel0[:F0]^T: grad_w and the rest of grad_X
//   k_rnn_bwd_finish  adds the partials in ascending chunk and the problems in ascending b, and
//                     writes the Keras layouts
// There is no gradient for the temperature.
//
// Padding.  A padded unit u >= H has zero rows and columns in every matrix, the transposed
// fragments included, so no dz reaches its dh through a product, g hid is loaded as 0 for it, and the
// cell's own paths multiply that 0: its dh, dc and so its four dz stay exactly 0 (the factors are the
// finite gate values of a zero pre-activation).  A padding row (i >= N) re-forms row N - 1, as in the
// forward pass, and k_rnn_bwd_recur sets its dz to 0 where the deltas are formed: every sum over rows
// downstream adds exact zeros for it, and the MFMA keeps rows apart, so no other row sees it.
//
// No floating-point atomics, no grid-wide barrier; every sum has an order fixed by (N, d, H, L).

struct BwdAssignArgs {
  int N, d, H;
  const double* X;    // [B][N][d]
  const double* gXo;  // [B][N][d]
  const double* A;    // [B][N][N]
  const double* Kd;   // [H][N]
  double inv_T;
  double* gz;         // [B][N][N]: grad_A on entry, gz on return
  double* ghid;       // [B][N][H]
};

// grid (N, B), PB lanes: row i of problem b
__global__ void __launch_bounds__(PB) k_rnn_bwd_assign(BwdAssignArgs a) {
  __shared__ double red[PB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x, b = blockIdx.y, N = a.N, d = a.d;
  const size_t row = ((size_t)b * N + i) * N;
  const double* __restrict__ Ai = a.A + row;
  double* __restrict__ gi = a.gz + row;
  const double* __restrict__ go = a.gXo + ((size_t)b * N + i) * d;
  const double* __restrict__ Xb = a.X + (size_t)b * N * d;
  double s = 0.0;
  for (int j = tid; j < N; j += PB) {
    double g = gi[j];
    for (int c = 0; c < d; ++c) g = fma(go[c], Xb[(size_t)j * d + c], g);
    gi[j] = g;
    s = fma(Ai[j], g, s);
  }
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  s = (red[0] + red[1]) + (red[2] + red[3]);
  for (int j = tid; j < N; j += PB) gi[j] = Ai[j] * (gi[j] - s) * a.inv_T;  // the lane's own entries
  __threadfence_block();
  __syncthreads();  // the row is complete and visible to the workgroup
  for (int q = wave; q < a.H; q += PB / 64) {
    double v = 0.0;
    for (int j = lane; j < N; j += 64) v = fma(gi[j], a.Kd[(size_t)q * N + j], v);
    v = wave_sum(v);
    if (lane == 0) a.ghid[((size_t)b * N + i) * a.H + q] = v;
  }
}

struct BwdColsArgs {
  int N, d, H;
  const double* A;    // [B][N][N]
  const double* gz;   // [B][N][N]
  const double* hid;  // [B][N][H]
  const double* gXo;  // [B][N][d]
  double* dense;      // [B][H + 1][N]: g Kd, then g bd, of each problem
  double* gX;         // [B][N][d]: the direct term
};

// grid (ceil(N / PB), H + 1 + d, B): column j, and in y the unit q of g Kd, g bd, or the coordinate c
__global__ void __launch_bounds__(PB) k_rnn_bwd_cols(BwdColsArgs a) {
  const int j = blockIdx.x * PB + threadIdx.x, y = blockIdx.y, b = blockIdx.z, N = a.N, H = a.H;
  if (j >= N) return;
  const size_t bN = (size_t)b * N;
  const double* __restrict__ M = (y <= H ? a.gz : a.A) + bN * N + j;
  double v = 0.0;
  if (y < H) {
    for (int i = 0; i < N; ++i) v = fma(a.hid[(bN + i) * H + y], M[(size_t)i * N], v);
    a.dense[((size_t)b * (H + 1) + y) * N + j] = v;
  } else if (y == H) {
    for (int i = 0; i < N; ++i) v += M[(size_t)i * N];
    a.dense[((size_t)b * (H + 1) + H) * N + j] = v;
  } else {
    const int c = y - H - 1;
    for (int i = 0; i < N; ++i) v = fma(M[(size_t)i * N], a.gXo[(bN + i) * a.d + c], v);
    a.gX[(bN + j) * a.d + c] = v;
  }
}

struct BwdRecurArgs {
  int N, H, Hp, HT, KS, RS;
  const double* P;       // [B][N][4 Hp]
  const double* W0i;     // [N][4 Hp]
  const double* binit;   // [L][4 Hp]
  const double* frag;    // the forward's weight fragments
  const double* fragT;   // the transposed ones: lane l of (tile, ks, slot) holds row 16 tile + (l & 15),
                         // column slot Hp + 4 ks + (l >> 4) of the matrix
  size_t frag_doubles;
  const double* hist_h;  // the recorded h, c (blocks of pf_rnn_bwd_plan.h)
  const double* hist_c;
  const double* ghid;    // [B][N][H]
  double* dz;            // the slot deltas, the same blocks with 4 Hp columns
};

// acc += dz (16 x 4 Hp, k-major in LDS) times the transposed fragments of one matrix, over the slots in mask
template <int MASK>
__device__ __forceinline__ void push_back(dbl4& acc, const double* dzl, const double* __restrict__ fr, int KS, int Hp,
                                          int lane) {
  const int r16 = lane & 15, kq = lane >> 4;
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
      if (MASK & (1 << s))
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(dzl[(s * Hp + 4 * ks + kq) * HS + r16], fr[(ks * SLOTS + s) * 64 + lane], acc,
                                                   0, 0, 0);
  }
}

// grid (ceil(N / 16), B), 64 HT RS lanes, dynamic LDS of BwdPlan::lds_bytes.  The ownership of k_rnn_recur:
// a workgroup owns 16 sequences, a wave 16 units of every layer and all four slots, for 4 / RS of the 4
// rows of a lane.
//
// Barriers.  Three LDS areas: hp = h_l(t-1), hb = h_{l-1}(t), both copied from the history, and dzl, the
// deltas, each in the A-operand layout.  A step (t, l) is  (a) all lanes copy hp, hb;  barrier 1;
// (b) the products re-form the pre-activations from hp, hb, the owners form dz and write dzl;  barrier 2;
// (c) the products push dzl back through the transposed fragments, and all lanes copy dzl to global
// memory.  (a) of the next step overwrites hp, hb: their last readers are in (b), before barrier 2.  (b)
// of the next step overwrites dzl: its last readers are in (c), before the next barrier 1.  So two
// barriers per step order every write against every read, and nothing is read that this launch has not
// written (the fragments' copy is ordered by the first barrier 1).
template <int CELL, int L, bool RES>
__global__ void __launch_bounds__(64 * (MAXH / 16)) k_rnn_bwd_recur(BwdRecurArgs a) {
  extern __shared__ double rnn_lds[];
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
  const int tile = (tid >> 6) / a.RS, sub = (tid >> 6) - tile * a.RS;
  const int b = blockIdx.y, i0 = blockIdx.x * RT, tiles = gridDim.x;
  const int N = a.N, Hp = a.Hp, KS = a.KS, W4 = SLOTS * a.Hp;
  const int rlast = min(N - 1 - i0, RT - 1);  // the tile's last row that is a particle
  double* hp = rnn_lds;        // [Hp][HS]
  double* hb = hp + Hp * HS;   // [Hp][HS]
  double* dzl = hb + Hp * HS;  // [4 Hp][HS]
  const double *fr_all = a.frag, *frT_all = a.fragT;
  if (RES) {
    double* wl = rnn_lds + 6 * Hp * HS;
    for (size_t q = tid; q < a.frag_doubles; q += blockDim.x) wl[q] = a.frag[q], wl[a.frag_doubles + q] = a.fragT[q];
    fr_all = wl, frT_all = wl + a.frag_doubles;
  }
  const int u = 16 * tile + r16;
  const size_t mat = (size_t)a.HT * KS * SLOTS * 64, mine = (size_t)tile * KS * SLOTS * 64;

  // dh_l and (LSTM) dc_l carried from t + 1.  The sweep starts from g hid at (t = N - 1, l = L - 1).  The
  // biases and the rows kernel0[F0 + i] are read where they are used: with four layers they would not fit
  // the registers beside these.
  dbl4 dhc[L], dcc[L];
#pragma unroll
  for (int l = 0; l < L; ++l) dhc[l] = dcc[l] = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 4; ++r)
    dhc[L - 1][r] = u < a.H ? a.ghid[((size_t)b * N + min(i0 + kq + 4 * r, N - 1)) * a.H + u] : 0.0;
  dbl4 dhin = {0.0, 0.0, 0.0, 0.0};  // dh_l(t) from layer l + 1
  const double* __restrict__ Pb = a.P + (size_t)b * N * W4 + u;
  constexpr int IN_MASK = CELL == CELL_LSTM ? 15 : 7, REC_MASK = CELL == CELL_LSTM ? 15 : 11;

  for (int t = N - 1; t >= 0; --t) {
    double pc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) pc[s] = Pb[(size_t)t * W4 + s * Hp];
#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
      // the layer as a value the compiler cannot see through: the addresses below are then formed here, at
      // every step, and not hoisted out of the loop over t for all L layers at once, which with four layers
      // costs more registers than a wave has
      int lv = l;
      asm volatile("" : "+s"(lv));
      // (a) the history of this step into the A-operand layout
      const size_t here = hblock(tiles, N, L, b, blockIdx.x, t, lv);
      const size_t prev = hblock(tiles, N, L, b, blockIdx.x, t > 0 ? t - 1 : 0, lv) * RT * Hp;
      for (int q = tid; q < Hp * RT; q += blockDim.x) {
        const int k = q >> 4, r = min(q & 15, rlast);
        hp[k * HS + (q & 15)] = t > 0 ? a.hist_h[prev + k * RT + r] : 0.0;
        if (l > 0) hb[k * HS + (q & 15)] = a.hist_h[(here - 1) * RT * Hp + k * RT + r];
      }
      dbl4 cp = {0.0, 0.0, 0.0, 0.0};
      if (CELL == CELL_LSTM && t > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) cp[r] = a.hist_c[prev + u * RT + min(kq + 4 * r, rlast)];
      }
      __syncthreads();  // barrier 1
      // (b) the pre-activations again, with the forward's products in the forward's order
      dbl4 acc[SLOTS];
      if (l == 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[s][r] = a.W0i[(size_t)min(i0 + kq + 4 * r, N - 1) * W4 + s * Hp + u] + pc[s];
      } else {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
          const double bls = a.binit[(size_t)lv * W4 + s * Hp + u];
          acc[s] = dbl4{bls, bls, bls, bls};
        }
        accumulate<IN_MASK>(acc, hb, fr_all + (2 * lv - 1) * mat + mine, KS, lane);
      }
      accumulate<REC_MASK>(acc, hp, fr_all + (2 * lv) * mat + mine, KS, lane);
      dbl4 direct = {0.0, 0.0, 0.0, 0.0};  // GRU: the path h_l(t-1) -> h_l(t) through z
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r * a.RS / 4 != sub) continue;  // another wave's row (a wave-uniform branch)
        double dh = dhc[l][r];
        if (l < L - 1) dh += dhin[r];
        double d0, d1, d2, d3;
        if (CELL == CELL_LSTM) {
          const double ig = sigmoid(acc[0][r]), fg = sigmoid(acc[1][r]), gg = tanh(acc[2][r]), og = sigmoid(acc[3][r]);
          const double tc = tanh(fg * cp[r] + ig * gg);
          const double dc = dcc[l][r] + dh * og * (1.0 - tc * tc);
          d0 = dc * gg * ig * (1.0 - ig);
          d1 = dc * cp[r] * fg * (1.0 - fg);
          d2 = dc * ig * (1.0 - gg * gg);
          d3 = dh * tc * og * (1.0 - og);
          dcc[l][r] = dc * fg;
        } else {
          const double z = sigmoid(acc[0][r]), rr = sigmoid(acc[1][r]);
          const double hh = tanh(acc[2][r] + rr * acc[3][r]);
          const double hprev = hp[u * HS + kq + 4 * r];
          const double da = dh * (1.0 - z) * (1.0 - hh * hh);
          d0 = dh * (hprev - hh) * z * (1.0 - z);
          d1 = da * acc[3][r] * rr * (1.0 - rr);
          d2 = da;
          d3 = da * rr;
          direct[r] = dh * z;
        }
        if (i0 + kq + 4 * r >= N) d0 = d1 = d2 = d3 = 0.0;  // a padding row contributes to no sum
        double* w = dzl + u * HS + kq + 4 * r;
        w[0] = d0, w[Hp * HS] = d1, w[2 * Hp * HS] = d2, w[3 * Hp * HS] = d3;
      }
      __syncthreads();  // barrier 2
      // (c) dh_l(t-1) = dz R^T (+ the direct path), dh_{l-1}(t) = dz K^T
      dbl4 pr = direct;
      push_back<REC_MASK>(pr, dzl, frT_all + (2 * lv) * mat + mine, KS, Hp, lane);
      dhc[l] = pr;
      if (l > 0) {
        dbl4 pk = {0.0, 0.0, 0.0, 0.0};
        push_back<IN_MASK>(pk, dzl, frT_all + (2 * lv - 1) * mat + mine, KS, Hp, lane);
        dhin = pk;
      }
      double* __restrict__ out = a.dz + here * RT * W4;
      for (int q = tid; q < W4 * RT; q += blockDim.x) out[q] = dzl[(q >> 4) * HS + (q & 15)];
    }
  }
}

struct BwdSumArgs {
  int N, L, Hp, tiles, F0, use_weight;
  const double* dz;
  const double* X;    // [B][N][d]
  const double* w;    // [B][N]
  const double* W0x;  // [F0][4 Hp]
  int d;
  double* S;          // [B][N][L][4 Hp]
  double* w0i;        // [B][N][4 Hp]
  double* k0x;        // [B][F0][4 Hp]
  double* gX;         // [B][N][d]
  double* gw;         // [B][N]
};

// grid (L ceil(4 Hp / PB), N, B): S[b][t][l][col], the rows of a problem in ascending order
__global__ void __launch_bounds__(PB) k_rnn_bwd_sums(BwdSumArgs a) {
  const int W4 = SLOTS * a.Hp, nb = (W4 + PB - 1) / PB;
  const int l = blockIdx.x / nb, col = (blockIdx.x - l * nb) * PB + threadIdx.x, t = blockIdx.y, b = blockIdx.z;
  if (col >= W4) return;
  double v = 0.0;
  for (int tile = 0; tile < a.tiles; ++tile) {
    const double* __restrict__ blk = a.dz + (hblock(a.tiles, a.N, a.L, b, tile, t, l) * W4 + col) * RT;
#pragma unroll
    for (int r = 0; r < RT; ++r) v += blk[r];  // a padding row holds an exact 0
  }
  a.S[(((size_t)b * a.N + t) * a.L + l) * W4 + col] = v;
}

// grid (ceil(4 Hp / PB), N, B): w0i[b][i][col] = sum_t dz_0(t) of row i, t ascending
__global__ void __launch_bounds__(PB) k_rnn_bwd_w0i(BwdSumArgs a) {
  const int W4 = SLOTS * a.Hp, col = blockIdx.x * PB + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
  if (col >= W4) return;
  double v = 0.0;
  for (int t = 0; t < a.N; ++t) v += a.dz[(hblock(a.tiles, a.N, a.L, b, i / RT, t, 0) * W4 + col) * RT + i % RT];
  a.w0i[((size_t)b * a.N + i) * W4 + col] = v;
}

__device__ __forceinline__ double feature(const BwdSumArgs& a, size_t bt, int f) {
  return (a.use_weight && f == 0) ? a.w[bt] : a.X[bt * a.d + f - a.use_weight];
}

// grid (ceil(4 Hp / PB), F0, B): k0x[b][f][col] = sum_t feat[b][t][f] gP[b][t][col], t ascending
__global__ void __launch_bounds__(PB) k_rnn_bwd_k0x(BwdSumArgs a) {
  const int W4 = SLOTS * a.Hp, col = blockIdx.x * PB + threadIdx.x, f = blockIdx.y, b = blockIdx.z;
  if (col >= W4) return;
  double v = 0.0;
  for (int t = 0; t < a.N; ++t) {
    const size_t bt = (size_t)b * a.N + t;
    v = fma(feature(a, bt, f), a.S[bt * a.L * W4 + col], v);
  }
  a.k0x[((size_t)b * a.F0 + f) * W4 + col] = v;
}

// grid (F0, N, B), one wave: g feat[b][t][f] = gP[b][t] . kernel0[f]; the weight's goes to grad_w, a
// coordinate's is added to the direct term of grad_X
__global__ void __launch_bounds__(64) k_rnn_bwd_feat(BwdSumArgs a) {
  const int W4 = SLOTS * a.Hp, f = blockIdx.x, t = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  const size_t bt = (size_t)b * a.N + t;
  const double* __restrict__ gP = a.S + bt * a.L * W4;
  double v = 0.0;
  for (int col = lane; col < W4; col += 64) v = fma(gP[col], a.W0x[(size_t)f * W4 + col], v);
  v = wave_sum(v);
  if (lane) return;
  if (a.use_weight && f == 0)
    a.gw[bt] = v;
  else
    a.gX[bt * a.d + f - a.use_weight] += v;
}

struct BwdWgradArgs {
  int N, L, Hp, HT, tiles, tc, chunks, mats;
  const double* hist_h;
  const double* dz;
  double* part;  // [B][mats][chunks][Hp][4 Hp]
};

// grid (HT 4 HT, chunks mats, B), one wave: the 16 x 16 tile (kt, ct) of matrix m (2 l: g R_l from
// h_l(t-1); 2 l - 1: g K_l from h_{l-1}(t)) over the chunk's timesteps and all row tiles, t then tile
// ascending, four k-steps of v_mfma_f64_16x16x4_f64 per block: the 16 rows are the reduction
__global__ void __launch_bounds__(64) k_rnn_bwd_wgrad(BwdWgradArgs a) {
  const int lane = threadIdx.x, r16 = lane & 15, kq = lane >> 4;
  const int W4 = SLOTS * a.Hp, nct = SLOTS * a.HT;
  const int kt = blockIdx.x / nct, ct = blockIdx.x - kt * nct;
  const int chunk = blockIdx.y / a.mats, m = blockIdx.y - chunk * a.mats, b = blockIdx.z;
  const int l = (m + 1) >> 1;
  const bool rec = !(m & 1);
  const int t0 = chunk * a.tc, t1 = min(a.N, t0 + a.tc);
  dbl4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int t = t0; t < t1; ++t) {
    if (rec && t == 0) continue;  // h_l(-1) = 0
    for (int tile = 0; tile < a.tiles; ++tile) {
      const int rlast = min(a.N - 1 - tile * RT, RT - 1);
      const double* __restrict__ hb =
          a.hist_h + (hblock(a.tiles, a.N, a.L, b, tile, rec ? t - 1 : t, rec ? l : l - 1) * a.Hp + 16 * kt + r16) * RT;
      const double* __restrict__ db = a.dz + (hblock(a.tiles, a.N, a.L, b, tile, t, l) * W4 + 16 * ct + r16) * RT;
#pragma unroll
      for (int st = 0; st < 4; ++st)  // a padding row: a recorded (finite) h times dz = 0
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(hb[min(4 * st + kq, rlast)], db[4 * st + kq], acc, 0, 0, 0);
    }
  }
  double* __restrict__ out = a.part + ((((size_t)b * a.mats + m) * a.chunks + chunk) * a.Hp + 16 * kt + kq) * W4 + 16 * ct + r16;
#pragma unroll
  for (int r = 0; r < 4; ++r) out[(size_t)4 * r * W4] = acc[r];
}

struct BwdFinishArgs {
  int kind;  // 0 kernel, 1 recurrent kernel, 2 bias of layer l; 3 the output kernel, 4 the output bias
  int l, N, H, Hp, F0, B, L, cell, chunks, mats;
  const double* part;
  const double* S;
  const double* w0i;
  const double* k0x;
  const double* dense;
  double* out;  // the array, in Keras' layout
  int64_t count;
};

// one lane per element of one Keras array: the per-problem gradient (partials in ascending chunk, or
// timesteps in ascending t), then the problems in ascending b
__global__ void __launch_bounds__(PB) k_rnn_bwd_finish(BwdFinishArgs a) {
  const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (e >= a.count) return;
  const int N = a.N, H = a.H, Hp = a.Hp, W4 = SLOTS * a.Hp, l = a.l;
  double total = 0.0;
  for (int b = 0; b < a.B; ++b) {
    double v = 0.0;
    if (a.kind <= 1) {
      const int GH = (a.cell == CELL_LSTM ? 4 : 3) * H;
      const int row = (int)(e / GH), rem = (int)(e - (int64_t)row * GH), g = rem / H, u = rem - g * H;
      const int col = ((a.cell == CELL_GRU && a.kind == 1 && g == 2) ? 3 : g) * Hp + u;
      if (a.kind == 0 && l == 0) {
        v = row < a.F0 ? a.k0x[((size_t)b * a.F0 + row) * W4 + col] : a.w0i[((size_t)b * N + row - a.F0) * W4 + col];
      } else {
        const int m = a.kind == 1 ? 2 * l : 2 * l - 1;
        const double* __restrict__ p = a.part + (((size_t)b * a.mats + m) * a.chunks * Hp + row) * W4 + col;
        for (int ch = 0; ch < a.chunks; ++ch) v += p[(size_t)ch * Hp * W4];
      }
    } else if (a.kind == 2) {
      int slot, u;
      if (a.cell == CELL_LSTM) {
        slot = (int)(e / H), u = (int)(e - (int64_t)slot * H);
      } else {  // bias[0]: the slots z, r, h-in; bias[1]: z, r, h-rec
        const int half = (int)(e / (3 * H)), rem = (int)(e - (int64_t)half * 3 * H), g = rem / H;
        u = rem - g * H;
        slot = (half == 1 && g == 2) ? 3 : g;
      }
      const double* __restrict__ p = a.S + ((size_t)b * N * a.L + l) * W4 + slot * Hp + u;
      for (int t = 0; t < N; ++t) v += p[(size_t)t * a.L * W4];
    } else if (a.kind == 3) {
      v = a.dense[(size_t)b * (H + 1) * N + e];
    } else {
      v = a.dense[((size_t)b * (H + 1) + H) * N + e];
    }
    total = b == 0 ? v : total + v;
  }
  a.out[e] = total;
}

// ---- The weights packed on the device (pf_rnn_set_weights_dev, and the transposed set of every
// backward pass): the index maps of pf_rnn_plan.h, one lane per destination element, so the writes
// are coalesced and the reads are gathers.  Every element of every buffer is written, the zeros of
// the padding included: nothing an earlier network left in the handle survives.
struct PackArgs {
  PackNet net;
  const double* src[3 * MAXL + 2];  // the Keras arrays, device pointers
  double* W0x;    // [F0][4 Hp]
  double* W0i;    // [N][4 Hp]
  double* binit;  // [L][4 Hp]
  double* frag;   // the weight fragments (pf_rnn_plan.h)
  double* Kd;    // [H][N]
  double* bd;     // [N]
  int64_t n_W0x, n_W0i, n_binit, n_frag, n_Kd, n_bd;
};

__device__ inline double pack_value(const PackArgs& a, const PackSrc s) {
  if (s.arr < 0) return 0.0;
  const double* __restrict__ p = a.src[s.arr];
  return s.idx2 >= 0 ? p[s.idx] + p[s.idx2] : p[s.idx];
}

// grid ceil((n_W0x + n_W0i + n_binit + n_frag + n_Kd + n_bd) / PB)
__global__ void __launch_bounds__(PB) k_rnn_pack(PackArgs a) {
  int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (e < a.n_W0x) { a.W0x[e] = pack_value(a, pack_src_W0x(a.net, e)); return; }
  e -= a.n_W0x;
  if (e < a.n_W0i) { a.W0i[e] = pack_value(a, pack_src_W0i(a.net, e)); return; }
  e -= a.n_W0i;
  if (e < a.n_binit) { a.binit[e] = pack_value(a, pack_src_binit(a.net, e)); return; }
  e -= a.n_binit;
  if (e < a.n_frag) { a.frag[e] = pack_value(a, pack_src_frag(a.net, e)); return; }
  e -= a.n_frag;
  if (e < a.n_Kd) { a.Kd[e] = a.src[3 * a.net.L][e]; return; }
  e -= a.n_Kd;
  if (e < a.n_bd) a.bd[e] = a.src[3 * a.net.L + 1][e];
}

// fragT from the forward's fragments, the permutation pack_fragT_from_frag.  grid ceil(count / PB)
__global__ void __launch_bounds__(PB) k_rnn_pack_T(PackNet net, int64_t count, const double* __restrict__ frag,
                                                   double* __restrict__ fragT) {
  const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (e >= count) return;
  const int64_t s = pack_fragT_from_frag(net, e);
  fragT[e] = s >= 0 ? frag[s] : 0.0;
}

}  // namespace rnn
}  // namespace pf
