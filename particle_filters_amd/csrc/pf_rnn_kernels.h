// Device side of the RNN resampler (pf_rnn_* of include/pf_engine.h; host side pf_rnn.hip, shape
// plan pf_rnn_plan.h).
//
// One resampling of models/DPF_RNN_resampling.py ("rnn.py":263-349) for B independent problems of
// N particles in d dimensions, fp64, forward only.  For each of the N new particles i the reference
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
};

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

// grid (ceil(N / 16), B), 64 HT RS lanes, dynamic LDS of Plan::lds_bytes
template <int CELL, int L, bool RES>
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

}  // namespace rnn
}  // namespace pf
