// Device side of the soft (Gumbel-Softmax) resampler (pf_soft_* of include/pf_engine.h; host side
// pf_soft.hip).
//
// One soft-resampling step (models/DPF_soft_resampling.py:309-334 and 348-350, "soft.py") for B
// independent problems of N particles in d dimensions, fp64.  With log_probs_j = log q_j formed on
// the host, row i of the assignment matrix is
//   z_ij = (log_probs_j + G_ij) / T,  a_ij = exp(z_ij - max_j z_ij) / sum_j exp(z_ij - max_j z_ij)
// and the outputs are X'_i = sum_j a_ij X_j and, on request, H_i = -sum_j a_ij log(a_ij + 1e-10).
// The N x N matrix is never stored, and neither are its N^2 Gumbel draws: G_ij is a pure function
// of (seed, epoch, problem, i, j) through Philox4x32-10 (soft_uniform, pf_soft_draws.h) and is generated where
// it is used.
//   k_soft_pass           one lane per output row i, a serial loop over the sources j staged through
//                         LDS in tiles of PT and read as broadcasts; at most PC state components per
//                         chunk, the draws regenerated per chunk; the source range split over S
//                         workgroups.  The lane keeps the running (max, sum, acc[]) of an online
//                         softmax: a source above the running maximum rescales what was summed so far.
//                         Leaves (max, sum) in pm / ps (chunk 0) and acc[] in part.
//   k_soft_finish         row maximum M_i and sum L_i from the S partials in the order s = 0..S-1,
//                         X'_i = (sum_s acc_s exp(max_s - M_i)) / L_i back in [N][d]; keeps (M_i, L_i)
//   k_soft_entropy        (on request) sum_j a_ij log(a_ij + 1e-10) over the sources of split s with
//                         the final (M_i, L_i), the draws regenerated once more
//   k_soft_entropy_finish H_i = -(sum of the S partials in the order s = 0..S-1)
//   k_soft_draws          U_ij and G_ij as the kernels above form them, for inspection and tests
//   k_soft_bwd_*          the backward pass, described in front of them at the end of this file
// The division by T is a product with 1 / T.  Tails are predicated: a padding source is never
// visited, a padding row computes row N - 1 again and stores nothing.  A Philox call serves the
// sources (2k, 2k + 1); every tile and every split starts at an even source, and with N odd the
// second half of the last call is dropped.  No floating-point atomics and no grid-wide barrier:
// launch boundaries are the synchronisation.  The order of every sum is fixed by (N, d): two calls
// on equal input are bitwise equal, and so is a problem solved in a batch or alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "philox.h"
#include "pf_dpf_plan.h"
#include "pf_soft_draws.h"

namespace pf {
namespace soft {

constexpr int PB = 256;     // lanes per workgroup of the one-dimensional kernels
constexpr int CB = dpf::CB;          // lanes (output rows) per workgroup of k_soft_pass and k_soft_entropy
constexpr int IGRAIN = dpf::IGRAIN;  // granularity of a split of the source range (even: pairs never straddle)
constexpr int MAXS = dpf::MAXS;      // most partials per output row
constexpr int PC = 16;      // most state components per chunk of k_soft_pass
constexpr int PT = 64;      // sources per LDS tile (even)
constexpr double ENTROPY_EPS = 1e-10;  // soft.py:349

// one source into the running (max, sum, acc[]) of a row's online softmax
template <int NC>
__device__ __forceinline__ void absorb(double z, const double* __restrict__ xq, double& mx, double& sum,
                                       double (&acc)[NC]) {
  if (z > mx) {  // exp(-inf - z) = 0 at the first source, where sum and acc are 0
    const double sc = exp(mx - z);
    sum *= sc;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] *= sc;
    mx = z;
  }
  const double e = exp(z - mx);
  sum += e;
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = fma(e, xq[c], acc[c]);
}

// grid (ceil(N / CB), ceil(d / PC) S, B), CB lanes: output row i, components [c0, c0 + NC) of chunk
// blockIdx.y / S, sources of split s = blockIdx.y % S.  X [B][N][d] and lp [B][N] in the host's
// layout.  pm, ps [B][S][Npad] (written by chunk 0); part [B][S][d][Npad].
template <int NC>
__global__ void __launch_bounds__(CB) k_soft_pass(Prob p, const double* __restrict__ X, const double* __restrict__ lp,
                                                  double inv_T, int chunk, int S, double* __restrict__ pm,
                                                  double* __restrict__ ps, double* __restrict__ part) {
  __shared__ double slp[PT], sx[PT * NC];
  const int t = threadIdx.x;
  const int b = blockIdx.z, ch = blockIdx.y / S, s = blockIdx.y - ch * S;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const int i = blockIdx.x * CB + t, ic = min(i, N - 1);
  const int c0 = ch * PC, nc = min(NC, d - c0);
  const int j0 = s * chunk, j1 = min(N, j0 + chunk);
  const double* __restrict__ Xb = X + (size_t)b * N * d + c0;
  const double* __restrict__ lpb = lp + (size_t)b * N;
  const uint32_t w3 = stream_word(p, b);
  double mx = -INFINITY, sum = 0.0;
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  for (int base = j0; base < j1; base += PT) {
    const int cnt = min(PT, j1 - base);
    for (int q = t; q < PT; q += CB) slp[q] = q < cnt ? lpb[base + q] : 0.0;
    for (int idx = t; idx < PT * NC; idx += CB) {
      const int q = idx / NC, c = idx - q * NC;
      sx[idx] = (c < nc && q < cnt) ? Xb[(size_t)(base + q) * d + c] : 0.0;
    }
    __syncthreads();
    for (int q = 0; q < cnt; q += 2) {
      const u32x4 r = pair_words(p, w3, (uint32_t)(base + q) >> 1, (uint32_t)ic);
      const double z0 = (slp[q] + gumbel(soft_uniform(r.x, r.y))) * inv_T;
      const double z1 = (slp[q + 1] + gumbel(soft_uniform(r.z, r.w))) * inv_T;
      absorb<NC>(z0, sx + q * NC, mx, sum, acc);
      if (q + 1 < cnt) absorb<NC>(z1, sx + (q + 1) * NC, mx, sum, acc);
    }
    __syncthreads();
  }
  if (i >= N) return;
  const size_t bs = (size_t)b * S + s;
  if (ch == 0) {
    pm[bs * P + i] = mx;
    ps[bs * P + i] = sum;
  }
  double* __restrict__ o = part + (bs * d + c0) * P + i;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < nc) o[(size_t)c * P] = acc[c];
}

// grid (ceil(N / PB), d, B): component c = blockIdx.y of row i.  Every component of a row forms the
// same (M_i, L_i) in the same order; component 0 keeps them in rowM, rowL [B][Npad].
__global__ void __launch_bounds__(PB) k_soft_finish(Prob p, int S, const double* __restrict__ pm,
                                                    const double* __restrict__ ps, const double* __restrict__ part,
                                                    double* __restrict__ rowM, double* __restrict__ rowL,
                                                    double* __restrict__ X_out) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const int i = blockIdx.x * PB + threadIdx.x;
  if (i >= N) return;
  double M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmax(M, pm[((size_t)b * S + s) * P + i]);
  double L = 0.0, v = 0.0;
  for (int s = 0; s < S; ++s) {
    const size_t bs = (size_t)b * S + s;
    const double w = exp(pm[bs * P + i] - M);
    L = fma(ps[bs * P + i], w, L);
    v = fma(part[(bs * d + c) * P + i], w, v);
  }
  X_out[((size_t)b * N + i) * d + c] = v / L;
  if (c == 0) {
    rowM[(size_t)b * P + i] = M;
    rowL[(size_t)b * P + i] = L;
  }
}

// grid (ceil(N / CB), S, B), CB lanes: hp [B][S][Npad] = sum over the sources of split s of
// a_ij log(a_ij + 1e-10), a_ij = exp(z_ij - M_i) / L_i
__global__ void __launch_bounds__(CB) k_soft_entropy(Prob p, const double* __restrict__ lp, double inv_T, int chunk,
                                                     int S, const double* __restrict__ rowM,
                                                     const double* __restrict__ rowL, double* __restrict__ hp) {
  __shared__ double slp[PT];
  const int t = threadIdx.x;
  const int b = blockIdx.z, s = blockIdx.y;
  const int N = p.N;
  const size_t P = (size_t)p.Npad;
  const int i = blockIdx.x * CB + t, ic = min(i, N - 1);
  const int j0 = s * chunk, j1 = min(N, j0 + chunk);
  const double* __restrict__ lpb = lp + (size_t)b * N;
  const uint32_t w3 = stream_word(p, b);
  const double M = rowM[(size_t)b * P + ic], L = rowL[(size_t)b * P + ic];
  double h = 0.0;
  for (int base = j0; base < j1; base += PT) {
    const int cnt = min(PT, j1 - base);
    for (int q = t; q < PT; q += CB) slp[q] = q < cnt ? lpb[base + q] : 0.0;
    __syncthreads();
    for (int q = 0; q < cnt; q += 2) {
      const u32x4 r = pair_words(p, w3, (uint32_t)(base + q) >> 1, (uint32_t)ic);
      const double a0 = exp((slp[q] + gumbel(soft_uniform(r.x, r.y))) * inv_T - M) / L;
      const double a1 = exp((slp[q + 1] + gumbel(soft_uniform(r.z, r.w))) * inv_T - M) / L;
      h = fma(a0, log(a0 + ENTROPY_EPS), h);
      if (q + 1 < cnt) h = fma(a1, log(a1 + ENTROPY_EPS), h);
    }
    __syncthreads();
  }
  if (i < N) hp[((size_t)b * S + s) * P + i] = h;
}

// grid (ceil(N / PB), B): H [B][N]
__global__ void __launch_bounds__(PB) k_soft_entropy_finish(Prob p, int S, const double* __restrict__ hp,
                                                            double* __restrict__ H) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * PB + threadIdx.x;
  if (i >= p.N) return;
  const size_t P = (size_t)p.Npad;
  double h = 0.0;
  for (int s = 0; s < S; ++s) h += hp[((size_t)b * S + s) * P + i];
  H[(size_t)b * p.N + i] = -h;
}

// grid (ceil(N N / PB), B): U, G [B][N][N] (either may be null), element (i, j) by the lane that
// the flat index i N + j names
__global__ void __launch_bounds__(PB) k_soft_draws(Prob p, double* __restrict__ U, double* __restrict__ G) {
  const int b = blockIdx.y;
  const int64_t NN = (int64_t)p.N * p.N;
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= NN) return;
  const uint32_t i = (uint32_t)(q / p.N), j = (uint32_t)(q - (int64_t)i * p.N);
  const u32x4 r = pair_words(p, stream_word(p, b), j >> 1, i);
  const double u = (j & 1) ? soft_uniform(r.z, r.w) : soft_uniform(r.x, r.y);
  if (U) U[(size_t)b * NN + q] = u;
  if (G) G[(size_t)b * NN + q] = gumbel(u);
}

// ---- the backward pass (pf_soft_backward): gX_j = sum_i a_ij gX'_i and
// glp_j = (1 / T)(X_j . gX_j - sum_i a_ij r_i) with r_i = gX'_i . X'_i, that is the transposed
// application A^T [gX' | r] to d + 1 components, a_ij = exp(z_ij - M_i) / L_i from the (M_i, L_i) of
// the forward pass: no online rescaling, a_ij <= 1.
//   k_soft_bwd_rows    r_i over all d in the order c = 0..d-1
//   k_soft_bwd_pass    one lane per source column pair (2k, 2k + 1), so that the Philox call of
//                      (k, i) serves both of the lane's columns and no draw is wasted; a serial loop
//                      over the rows i of split s, their gX'_i[c], r_i, M_i and 1 / L_i staged through
//                      LDS in tiles of PT and read as broadcasts; at most PC components per chunk,
//                      the draws regenerated per chunk, the r column riding with chunk 0
//   k_soft_bwd_finish  component c of column j (c = d: the r column) summed over the S partials in
//                      the order s = 0..S-1
//   k_soft_bwd_glp     glp_j from gX_j, X_j and the summed r column
// The draws are the forward's: the same counters, soft_uniform and gumbel, z formed by the same
// expression.  The division by L_i is a product with 1 / L_i formed once per staged row.

// grid (ceil(N / PB), B): r [B][N] of gXo, Xo [B][N][d]
__global__ void __launch_bounds__(PB) k_soft_bwd_rows(Prob p, const double* __restrict__ gXo,
                                                      const double* __restrict__ Xo, double* __restrict__ r) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * PB + threadIdx.x;
  if (i >= p.N) return;
  const size_t o = ((size_t)b * p.N + i) * p.d;
  double v = 0.0;
  for (int c = 0; c < p.d; ++c) v = fma(gXo[o + c], Xo[o + c], v);
  r[(size_t)b * p.N + i] = v;
}

// grid (ceil(ceil(N / 2) / CB), ceil(d / PC) S, B), CB lanes: source columns (2k, 2k + 1), components
// [c0, c0 + NC) of chunk blockIdx.y / S, rows of split s = blockIdx.y % S.  gXo [B][N][d], r and lp
// [B][N]; rowM, rowL [B][ldm].  bpart [B][S][d + 1][Npad], component d the r column (chunk 0).  A
// padding lane computes the last pair again and stores nothing; with N odd the second column of the
// last pair takes a_ij = 0 and is not stored.
template <int NC>
__global__ void __launch_bounds__(CB) k_soft_bwd_pass(Prob p, const double* __restrict__ gXo, const double* __restrict__ r,
                                                      const double* __restrict__ lp, const double* __restrict__ rowM,
                                                      const double* __restrict__ rowL, int ldm, double inv_T, int chunk,
                                                      int S, double* __restrict__ bpart) {
  __shared__ double sg[PT * NC], sr[PT], sM[PT], sI[PT];
  const int t = threadIdx.x;
  const int b = blockIdx.z, ch = blockIdx.y / S, s = blockIdx.y - ch * S;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const int np = (N + 1) >> 1;
  const int k = blockIdx.x * CB + t, kc = min(k, np - 1);
  const int j0 = 2 * kc;
  const bool two = j0 + 1 < N;
  const int c0 = ch * PC, nc = min(NC, d - c0);
  const int i0 = s * chunk, i1 = min(N, i0 + chunk);
  const double* __restrict__ gb = gXo + (size_t)b * N * d + c0;
  const double* __restrict__ rb = r + (size_t)b * N;
  const double* __restrict__ Mb = rowM + (size_t)b * ldm;
  const double* __restrict__ Lb = rowL + (size_t)b * ldm;
  const double lp0 = lp[(size_t)b * N + j0], lp1 = two ? lp[(size_t)b * N + j0 + 1] : 0.0;
  const uint32_t w3 = stream_word(p, b);
  double a0[NC], a1[NC], r0 = 0.0, r1 = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c) a0[c] = a1[c] = 0.0;
  for (int base = i0; base < i1; base += PT) {
    const int cnt = min(PT, i1 - base);
    for (int q = t; q < PT; q += CB) {
      const bool in = q < cnt;
      sr[q] = in ? rb[base + q] : 0.0;
      sM[q] = in ? Mb[base + q] : 0.0;
      sI[q] = in ? 1.0 / Lb[base + q] : 0.0;
    }
    for (int idx = t; idx < PT * NC; idx += CB) {
      const int q = idx / NC, c = idx - q * NC;
      sg[idx] = (c < nc && q < cnt) ? gb[(size_t)(base + q) * d + c] : 0.0;
    }
    __syncthreads();
    for (int q = 0; q < cnt; ++q) {
      const u32x4 w = pair_words(p, w3, (uint32_t)kc, (uint32_t)(base + q));
      const double z0 = (lp0 + gumbel(soft_uniform(w.x, w.y))) * inv_T;
      const double z1 = (lp1 + gumbel(soft_uniform(w.z, w.w))) * inv_T;
      const double e0 = exp(z0 - sM[q]) * sI[q];
      const double e1 = two ? exp(z1 - sM[q]) * sI[q] : 0.0;
      const double* __restrict__ g = sg + q * NC;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        a0[c] = fma(e0, g[c], a0[c]);
        a1[c] = fma(e1, g[c], a1[c]);
      }
      r0 = fma(e0, sr[q], r0);
      r1 = fma(e1, sr[q], r1);
    }
    __syncthreads();
  }
  if (k >= np) return;
  double* __restrict__ o = bpart + (((size_t)b * S + s) * (d + 1) + c0) * P + j0;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < nc) {
      o[(size_t)c * P] = a0[c];
      if (two) o[(size_t)c * P + 1] = a1[c];
    }
  if (ch == 0) {
    o[(size_t)d * P] = r0;
    if (two) o[(size_t)d * P + 1] = r1;
  }
}

// grid (ceil(N / PB), d + 1, B): component c = blockIdx.y of column j; c < d goes to gX [B][N][d],
// c = d (the r column) to ar [B][N]
__global__ void __launch_bounds__(PB) k_soft_bwd_finish(Prob p, int S, const double* __restrict__ bpart,
                                                        double* __restrict__ gX, double* __restrict__ ar) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const int j = blockIdx.x * PB + threadIdx.x;
  if (j >= N) return;
  double v = 0.0;
  for (int s = 0; s < S; ++s) v += bpart[(((size_t)b * S + s) * (d + 1) + c) * P + j];
  if (c < d) gX[((size_t)b * N + j) * d + c] = v;
  else ar[(size_t)b * N + j] = v;
}

// grid (ceil(N / PB), B): glp [B][N] = (X_j . gX_j - ar_j) / T, the dot product in the order c = 0..d-1
__global__ void __launch_bounds__(PB) k_soft_bwd_glp(Prob p, double inv_T, const double* __restrict__ X,
                                                     const double* __restrict__ gX, const double* __restrict__ ar,
                                                     double* __restrict__ glp) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * PB + threadIdx.x;
  if (j >= p.N) return;
  const size_t o = ((size_t)b * p.N + j) * p.d;
  double v = 0.0;
  for (int c = 0; c < p.d; ++c) v = fma(X[o + c], gX[o + c], v);
  glp[(size_t)b * p.N + j] = (v - ar[(size_t)b * p.N + j]) * inv_T;
}

}  // namespace soft
}  // namespace pf
