// Device side of the Sinkhorn optimal-transport resampler (pf_ot_* of include/pf_engine.h; host side
// pf_ot.hip).
//
// One sinkhorn_ot_resample (models/DPF_OT_resampling.py:119-204, "ot.py") for B independent problems
// of N particles in d dimensions, fp64:
//   k_ot_prepare   a = max(w, min_val) / (sum + min_val), particles to SoA x [d][Npad], |x|^2,
//                  f = g = 0, the problem's done flag and iteration count zeroed      ot.py:127-139
//   k_ot_cost      C_ij = max((|x_i|^2 - 2 x_i.x_j) + |x_j|^2, 0), C [N][Npad]       ot.py:25-31
//   k_ot_tau_rows  f_i <- (f_i + Tau(b, g, C[i, :])) / 2: one wave per row i, lanes along the row
//   k_ot_tau_cols  g_j <- (g_j + Tau(a, f, C[:, j])) / 2: lanes over j, a loop over i that reads
//                  C[i][j] coalesced, (f_i, a_i) broadcast from LDS; the i range split over S
//                  workgroups into (max, sum) partials when N is large               ot.py:150-164
//   k_ot_merge     (S > 1) g_j from the partials, merged in the order s = 0..S-1
//   k_ot_check     forms max|f - f_old| and max|g - g_old|, records them, counts the iteration and
//                  sets the done flag by the reference's rule (from the second iteration on, both
//                  below tol)                                                        ot.py:166-181
//   k_ot_project   sum_i max(a_i b exp((f_i + g_j - C_ij) / eps), min_val) X_i over a chunk of at
//                  most 16 state components, the plan recomputed and never stored; the source
//                  range split as above; chunk 0 also sums P C and counts P > 1e-6   ot.py:184-212
//   k_ot_finish    partials summed in the order s = 0..S-1, divided by b, back to [N][d]
//   k_ot_stats     the plan statistics reduced over j in a fixed order
// Tau(m, h, c) = -eps (log(max(sum_k m_k exp(e_k - max e), min_val)) + max e), e = (h - c) / eps, is
// evaluated as the reference does, the maximum first and then the sum, so that an unsplit pass
// differs from the NumPy restatement by the order of its sum only.  The division by eps is a
// product with 1 / eps.  Every tau and check launch of a problem whose done flag is set returns at
// entry: f and g stay those of the stopping iteration.  Tails are predicated: no padding particle
// contributes.  No floating-point atomics and no grid-wide barrier: launch boundaries are the
// synchronisation, and two calls on the same input are bitwise equal.
//
// The backward pass (pf_ot_backward) is the reverse sweep over the unrolled damped loop:
//   k_ot_tau_rows / k_ot_tau_cols / k_ot_merge <true>  the replay: iteration k of the problems with
//                  k <= K_b, no check; f^k, g^k, the two tau vectors and, per column of the g pass,
//                  the index of the maximum where the floor inside Tau bound (-1 otherwise) go to Hist
//                  (<true, true>: the forward pass recording its own iterations, gated by the done flag)
//   k_ot_bwd_counts  K_b, the caller's iteration counts clamped to the sweep, the only counts read below
//   k_ot_bwd_load  the incoming gradient to SoA
//   k_ot_bwd_q     Cbar_ij <- q_ij = N X_i . G_j, shaped like k_ot_cost
//   k_ot_bwd_rowacc<NC, false>  the projection: one wave per row i and component chunk; the plan
//                  recomputed, Xbar_i = N sum_j P_ij G_j, and (chunk 0) D_ij = [unfloored] P_ij q_ij / eps,
//                  Cbar_ij <- -D_ij, fbar_i = sum_j D_ij, abar_i = eps fbar_i / a_i
//   k_ot_bwd_cols<false> + k_ot_bwd_merge(0)  gbar_j = -sum_i Cbar_ij
//   k_ot_bwd_rows  the g pass of iteration k, shaped like k_ot_tau_rows: s_ij from the stored tau,
//                  Cbar[i, :] += t s, fbar_i and abar_i updated from the wave's sums
//   k_ot_bwd_cols<true> + k_ot_bwd_merge(1)  the f pass, shaped like k_ot_tau_cols: Cbar += t r,
//                  gbar_j <- gbar_j / 2 - sum_i t_i r_ij merged in the order s = 0..S-1, fbar <- fbar / 2
//   k_ot_bwd_rowacc<NC, true> / k_ot_bwd_cost_cols  the cost: Xbar_i += 2 sum_j Cbar'_ij (x_i - x_j)
//                  (a row pass) + 2 sum_j Cbar'_ji (x_i - x_j) (a column pass), Cbar' = Cbar where C != 0
//   k_ot_bwd_finish, k_ot_bwd_weights  back to [N][d]; the chain through the weight normalisation
// Every (i, j) of Cbar is touched once per launch by one lane, so Cbar needs no atomics either.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pf_dpf_plan.h"

namespace pf {
namespace ot {

constexpr int PB = 256;     // lanes per workgroup of the one-dimensional kernels
constexpr int RW = 4;       // rows (waves) per workgroup of k_ot_tau_rows
constexpr int CB = dpf::CB;          // lanes per workgroup of k_ot_tau_cols and k_ot_project
constexpr int IGRAIN = dpf::IGRAIN;  // granularity of a split of the source range
constexpr int MAXS = dpf::MAXS;      // most partials per output
constexpr int CT = 16;      // rows of C per workgroup of k_ot_cost
constexpr int KC = 64;      // state components per LDS stage of k_ot_cost
constexpr int TT = 128;     // sources per LDS tile of k_ot_tau_cols
constexpr int PC = 16;      // most state components per chunk of k_ot_project
constexpr int PT = 64;      // sources per LDS tile of k_ot_project
constexpr double SPARSITY_THRESHOLD = 1e-6;  // ot.py:211

struct Prob {
  int N, Npad, d, B;
  double* a;     // [B][Npad] source mass
  double* x;     // [B][d][Npad]
  double* x2;    // [B][Npad]
  double* f;     // [B][Npad]
  double* g;     // [B][Npad]
  double* fold;  // [B][Npad] f before the iteration's update
  double* gold;  // [B][Npad]
  double* C;     // [B][N][Npad]
  int* done;     // [B]
  int* iters;    // [B]
};

// The dual history of the backward pass.  Slot q of iteration k (0 = the start, f = g = 0) of
// problem b is v[((b 4 + q) (kcap + 1) + k) ld ..]; am row k - 1 belongs to the g pass of k.  The
// rows are ld apart: Npad in the handle's own buffers, N in a caller's device memory (the layout
// of the host arrays).
enum { HF = 0, HG = 1, HTF = 2, HTG = 3 };
struct Hist {
  double* v;         // [B][4][kcap + 1][ld]: f^k, g^k, tau_f^k, tau_g^k
  int32_t* am;       // [B][kcap][ld]: argmax_i (f^k_i - C_ij) where the column sum was floored, else -1
  const int32_t* K;  // [B]: iterations of problem b
  int kcap;
  int ld;
};
__device__ inline double* hist_at(const Hist& h, int b, int q, int k) {
  return h.v + (((size_t)b * 4 + q) * (size_t)(h.kcap + 1) + k) * (size_t)h.ld;
}
__device__ inline int32_t* hist_am(const Hist& h, int b, int k) {
  return h.am + ((size_t)b * h.kcap + (k - 1)) * (size_t)h.ld;
}

// How a tau launch is gated and whether it records (the template arguments of k_ot_tau_rows,
// k_ot_tau_cols and k_ot_merge):
//   <false>        the forward pass: returns when the problem is done;
//   <true>         the replay of the backward pass: iteration k of the problems with k <= K_b, recorded;
//   <true, true>   the forward pass that records its own history: gated by the done flag, k the
//                  problem's iteration count on the device plus one (never past kcap).
// true when the launch has nothing to do; sets k in the third mode
template <bool REC, bool LIVE>
__device__ inline bool tau_skip(const int* __restrict__ done, const int* __restrict__ iters, const Hist& hs, int b,
                                int& k) {
  if constexpr (LIVE) {
    if (done[b]) return true;
    k = iters[b] + 1;
    return k > hs.kcap;
  } else if constexpr (REC) {
    return k > hs.K[b];
  } else {
    return done[b] != 0;
  }
}

// sum of sh[0..PB) into every lane, in a fixed order; sh is overwritten
__device__ inline double block_sum(double* sh, double v) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int w = PB / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] += sh[t + w];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__device__ inline double block_max(double* sh, double v) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int w = PB / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] = fmax(sh[t], sh[t + w]);
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__device__ inline double tau_value(double sum, double mx, double eps, double min_val) {
  return -eps * (log(fmax(sum, min_val)) + mx);
}

// grid (ceil(N / PB), B).  X [B][N][d], w [B][N] (host layout).  Every workgroup of a problem forms
// the same weight sum in the same order.
__global__ void __launch_bounds__(PB) k_ot_prepare(Prob p, const double* __restrict__ X, const double* __restrict__ w,
                                                   double min_val) {
  __shared__ double sh[PB];
  const int t = threadIdx.x, b = blockIdx.y;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const double* __restrict__ wb = w + (size_t)b * N;
  double s = 0.0;
  for (int i = t; i < N; i += PB) s += fmax(wb[i], min_val);
  const double total = block_sum(sh, s);
  const int i = blockIdx.x * PB + t;
  if (blockIdx.x == 0 && t == 0) {
    p.done[b] = 0;
    p.iters[b] = 0;
  }
  if (i >= N) return;
  const size_t o = (size_t)b * P + i;
  p.a[o] = fmax(wb[i], min_val) / (total + min_val);
  p.f[o] = 0.0;
  p.g[o] = 0.0;
  p.fold[o] = 0.0;
  p.gold[o] = 0.0;
  const double* __restrict__ Xi = X + ((size_t)b * N + i) * d;
  double* __restrict__ xb = p.x + (size_t)b * d * P;
  double sq = 0.0;
  for (int k = 0; k < d; ++k) {
    const double v = Xi[k];
    xb[(size_t)k * P + i] = v;
    sq += v * v;
  }
  p.x2[o] = sq;
}

// grid (ceil(N / PB), ceil(N / CT), B): lane j against the CT rows i of blockIdx.y, whose components
// come through LDS in stages of KC (every lane reads the same x_ik: a broadcast).
__global__ void __launch_bounds__(PB) k_ot_cost(Prob p) {
  __shared__ double xs[KC * CT];
  const int t = threadIdx.x, b = blockIdx.z;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const int j = blockIdx.x * PB + t, i0 = blockIdx.y * CT;
  const int jc = min(j, N - 1);  // lanes past N read particle N - 1 and store nothing
  const double* __restrict__ xb = p.x + (size_t)b * d * P;
  double acc[CT];
#pragma unroll
  for (int r = 0; r < CT; ++r) acc[r] = 0.0;
  for (int k0 = 0; k0 < d; k0 += KC) {
    const int kc = min(KC, d - k0);
    for (int idx = t; idx < kc * CT; idx += PB) {
      const int k = idx / CT, r = idx - k * CT;
      xs[idx] = (i0 + r < N) ? xb[(size_t)(k0 + k) * P + i0 + r] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
      const double xj = xb[(size_t)(k0 + k) * P + jc];
#pragma unroll
      for (int r = 0; r < CT; ++r) acc[r] = fma(xs[k * CT + r], xj, acc[r]);
    }
    __syncthreads();
  }
  if (j >= N) return;
  const double* __restrict__ x2 = p.x2 + (size_t)b * P;
  double* __restrict__ Cb = p.C + (size_t)b * N * P;
  const double x2j = x2[j];
#pragma unroll
  for (int r = 0; r < CT; ++r)
    if (i0 + r < N) Cb[(size_t)(i0 + r) * P + j] = fmax((x2[i0 + r] - 2.0 * acc[r]) + x2j, 0.0);
}

// grid (ceil(N / RW), B), PB lanes: wave w of the workgroup owns row i = blockIdx.x * RW + w.
// REC (the replay of the backward pass): iteration k of the problems with k <= K_b, recorded in hs.
// LIVE: the forward pass recording its own iterations (tau_skip above).
template <bool REC, bool LIVE = false>
__global__ void __launch_bounds__(PB) k_ot_tau_rows(Prob p, double inv_eps, double eps, double min_val, Hist hs,
                                                    int k) {
  const int b = blockIdx.y;
  if (tau_skip<REC, LIVE>(p.done, p.iters, hs, b, k)) return;
  const int lane = threadIdx.x & 63, i = blockIdx.x * RW + (threadIdx.x >> 6);
  const int N = p.N;
  if (i >= N) return;  // the whole wave
  const size_t P = (size_t)p.Npad;
  const double* __restrict__ Ci = p.C + ((size_t)b * N + i) * P;
  const double* __restrict__ gb = p.g + (size_t)b * P;
  const double bj = 1.0 / (double)N;
  double mx = -INFINITY;
#pragma unroll 4
  for (int j = lane; j < N; j += 64) mx = fmax(mx, (gb[j] - Ci[j]) * inv_eps);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  double s = 0.0;
#pragma unroll 4
  for (int j = lane; j < N; j += 64) s += bj * exp((gb[j] - Ci[j]) * inv_eps - mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) {
    const size_t q = (size_t)b * P + i;
    const double fo = p.f[q];
    const double tau = tau_value(s, mx, eps, min_val);
    const double fn = 0.5 * (fo + tau);
    p.fold[q] = fo;
    p.f[q] = fn;
    if constexpr (REC) {
      hist_at(hs, b, HF, k)[i] = fn;
      hist_at(hs, b, HTF, k)[i] = tau;
    }
  }
}

// grid (ceil(N / CB), S, B), CB lanes: lane j over the sources [s chunk, (s + 1) chunk).  With S = 1
// the lane finishes g_j; otherwise it leaves (max, sum) in pm / ps [B][S][Npad] for k_ot_merge.
// REC as in k_ot_tau_rows; the lane also keeps the first source that attains its maximum (pam
// [B][S][Npad] when split).
template <bool REC, bool LIVE = false>
__global__ void __launch_bounds__(CB) k_ot_tau_cols(Prob p, double inv_eps, double eps, double min_val, int chunk,
                                                    int S, double* __restrict__ pm, double* __restrict__ ps, Hist hs,
                                                    int k, int32_t* __restrict__ pam) {
  __shared__ double2 sh[TT];
  const int b = blockIdx.z;
  if (tau_skip<REC, LIVE>(p.done, p.iters, hs, b, k)) return;
  const int t = threadIdx.x, s = blockIdx.y;
  const int N = p.N;
  const size_t P = (size_t)p.Npad;
  const int j = blockIdx.x * CB + t, jc = min(j, N - 1);
  const int i0 = s * chunk, i1 = min(N, i0 + chunk);
  const double* __restrict__ Cj = p.C + (size_t)b * N * P + jc;
  const double* __restrict__ fb = p.f + (size_t)b * P;
  const double* __restrict__ ab = p.a + (size_t)b * P;
  double mx = -INFINITY;
  int32_t am = i0;
  for (int base = i0; base < i1; base += TT) {
    const int cnt = min(TT, i1 - base);
    for (int q = t; q < cnt; q += CB) sh[q] = make_double2(fb[base + q], ab[base + q]);
    __syncthreads();
#pragma unroll 4
    for (int q = 0; q < cnt; ++q) {
      const double e = (sh[q].x - Cj[(size_t)(base + q) * P]) * inv_eps;
      if constexpr (REC) {
        if (e > mx) {
          mx = e;
          am = base + q;
        }
      } else {
        mx = fmax(mx, e);
      }
    }
    __syncthreads();
  }
  double sum = 0.0;
  for (int base = i0; base < i1; base += TT) {
    const int cnt = min(TT, i1 - base);
    for (int q = t; q < cnt; q += CB) sh[q] = make_double2(fb[base + q], ab[base + q]);
    __syncthreads();
#pragma unroll 4
    for (int q = 0; q < cnt; ++q) {
      const double2 fa = sh[q];
      sum += fa.y * exp((fa.x - Cj[(size_t)(base + q) * P]) * inv_eps - mx);
    }
    __syncthreads();
  }
  if (j >= N) return;
  if (S == 1) {
    const size_t q = (size_t)b * P + j;
    const double go = p.g[q];
    const double tau = tau_value(sum, mx, eps, min_val);
    const double gn = 0.5 * (go + tau);
    p.gold[q] = go;
    p.g[q] = gn;
    if constexpr (REC) {
      hist_at(hs, b, HG, k)[j] = gn;
      hist_at(hs, b, HTG, k)[j] = tau;
      hist_am(hs, b, k)[j] = sum > min_val ? -1 : am;
    }
  } else {
    const size_t q = ((size_t)b * S + s) * P + j;
    pm[q] = mx;
    ps[q] = sum;
    if constexpr (REC) pam[q] = am;
  }
}

// grid (ceil(N / PB), B): g_j from the S > 1 partials of column j, merged in the order s = 0..S-1
template <bool REC, bool LIVE = false>
__global__ void __launch_bounds__(PB) k_ot_merge(Prob p, double eps, double min_val, int S,
                                                 const double* __restrict__ pm, const double* __restrict__ ps, Hist hs,
                                                 int k, const int32_t* __restrict__ pam) {
  const int b = blockIdx.y;
  if (tau_skip<REC, LIVE>(p.done, p.iters, hs, b, k)) return;
  const int j = blockIdx.x * PB + threadIdx.x;
  if (j >= p.N) return;
  const size_t P = (size_t)p.Npad;
  double mx = -INFINITY;
  int32_t am = 0;
  for (int s = 0; s < S; ++s) {
    const size_t r = ((size_t)b * S + s) * P + j;
    if constexpr (REC) {
      if (pm[r] > mx) {
        mx = pm[r];
        am = pam[r];
      }
    } else {
      mx = fmax(mx, pm[r]);
    }
  }
  double sum = 0.0;
  for (int s = 0; s < S; ++s) {
    const size_t r = ((size_t)b * S + s) * P + j;
    sum += ps[r] * exp(pm[r] - mx);
  }
  const size_t q = (size_t)b * P + j;
  const double go = p.g[q];
  const double tau = tau_value(sum, mx, eps, min_val);
  const double gn = 0.5 * (go + tau);
  p.gold[q] = go;
  p.g[q] = gn;
  if constexpr (REC) {
    hist_at(hs, b, HG, k)[j] = gn;
    hist_at(hs, b, HTG, k)[j] = tau;
    hist_am(hs, b, k)[j] = sum > min_val ? -1 : am;
  }
}

// grid (B), PB lanes.  hist [B][n_iters][2] = (f_change, g_change) of iteration it >= 1.
__global__ void __launch_bounds__(PB) k_ot_check(Prob p, double tol, int n_iters, double* __restrict__ hist) {
  __shared__ double sh[PB];
  const int b = blockIdx.x;
  if (p.done[b]) return;
  const int t = threadIdx.x, N = p.N;
  const size_t P = (size_t)p.Npad;
  const double* __restrict__ f = p.f + (size_t)b * P;
  const double* __restrict__ fo = p.fold + (size_t)b * P;
  const double* __restrict__ g = p.g + (size_t)b * P;
  const double* __restrict__ go = p.gold + (size_t)b * P;
  double fc = 0.0, gc = 0.0;
#pragma unroll 4
  for (int j = t; j < N; j += PB) {
    fc = fmax(fc, fabs(f[j] - fo[j]));
    gc = fmax(gc, fabs(g[j] - go[j]));
  }
  fc = block_max(sh, fc);
  gc = block_max(sh, gc);
  if (t == 0) {
    const int it = p.iters[b];  // the reference's `iteration`
    if (it > 0) {
      if (it < n_iters) {
        hist[((size_t)b * n_iters + it) * 2] = fc;
        hist[((size_t)b * n_iters + it) * 2 + 1] = gc;
      }
      if (fc < tol && gc < tol) p.done[b] = 1;
    }
    p.iters[b] = it + 1;
  }
}

// grid (ceil(N / CB), ceil(d / PC) S, B), CB lanes: target j, components [c0, c0 + NC) of chunk
// blockIdx.y / S, sources of split s = blockIdx.y % S.  part [B][S][d][Npad]; spart [B][S][2][Npad]
// (sum P C, count P > 1e-6), written by chunk 0 when non-null.
template <int NC>
__global__ void __launch_bounds__(CB) k_ot_project(Prob p, double inv_eps, double min_val, int chunk, int S,
                                                   double* __restrict__ part, double* __restrict__ spart) {
  __shared__ double sf[PT], sab[PT], sx[PT * NC];
  const int t = threadIdx.x;
  const int b = blockIdx.z, ch = blockIdx.y / S, s = blockIdx.y - ch * S;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const int j = blockIdx.x * CB + t, jc = min(j, N - 1);
  const int c0 = ch * PC, nc = min(NC, d - c0);
  const int i0 = s * chunk, i1 = min(N, i0 + chunk);
  const bool stats = spart != nullptr && ch == 0;
  const double* __restrict__ Cj = p.C + (size_t)b * N * P + jc;
  const double* __restrict__ fb = p.f + (size_t)b * P;
  const double* __restrict__ ab = p.a + (size_t)b * P;
  const double* __restrict__ xb = p.x + ((size_t)b * d + c0) * P;
  const double bN = 1.0 / (double)N;
  const double gj = p.g[(size_t)b * P + jc];
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  double pc = 0.0, cnt_big = 0.0;
  for (int base = i0; base < i1; base += PT) {
    const int cnt = min(PT, i1 - base);
    for (int q = t; q < cnt; q += CB) {
      sf[q] = fb[base + q];
      sab[q] = ab[base + q] * bN;
    }
    for (int idx = t; idx < NC * PT; idx += CB) {
      const int c = idx / PT, q = idx - c * PT;
      sx[q * NC + c] = (c < nc && q < cnt) ? xb[(size_t)c * P + base + q] : 0.0;
    }
    __syncthreads();
    for (int q = 0; q < cnt; ++q) {
      const double cij = Cj[(size_t)(base + q) * P];
      const double pij = fmax(sab[q] * exp(((sf[q] + gj) - cij) * inv_eps), min_val);
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = fma(pij, sx[q * NC + c], acc[c]);
      if (stats) {
        pc = fma(pij, cij, pc);
        cnt_big += (pij > SPARSITY_THRESHOLD) ? 1.0 : 0.0;
      }
    }
    __syncthreads();
  }
  if (j >= N) return;
  double* __restrict__ o = part + (((size_t)b * S + s) * d + c0) * P + j;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < nc) o[(size_t)c * P] = acc[c];
  if (stats) {
    spart[(((size_t)b * S + s) * 2) * P + j] = pc;
    spart[(((size_t)b * S + s) * 2 + 1) * P + j] = cnt_big;
  }
}

// grid (ceil(N d / PB), B): X_out [B][N][d] = (sum_s part) / b
__global__ void __launch_bounds__(PB) k_ot_finish(Prob p, int S, const double* __restrict__ part,
                                                  double* __restrict__ X_out) {
  const int b = blockIdx.y;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= (int64_t)N * d) return;
  const int i = (int)(q / d), c = (int)(q - (int64_t)i * d);
  double v = 0.0;
  for (int s = 0; s < S; ++s) v += part[(((size_t)b * S + s) * d + c) * P + i];
  X_out[(size_t)b * N * d + q] = v / (1.0 / (double)N);
}

// grid (B), PB lanes: stats [B][2] = (sum P C, count P > 1e-6)
__global__ void __launch_bounds__(PB) k_ot_stats(Prob p, int S, const double* __restrict__ spart,
                                                 double* __restrict__ stats) {
  __shared__ double sh[PB];
  const int b = blockIdx.x, t = threadIdx.x, N = p.N;
  const size_t P = (size_t)p.Npad;
  double pc = 0.0, cnt = 0.0;
  for (int j = t; j < N; j += PB)
    for (int s = 0; s < S; ++s) {
      pc += spart[(((size_t)b * S + s) * 2) * P + j];
      cnt += spart[(((size_t)b * S + s) * 2 + 1) * P + j];
    }
  pc = block_sum(sh, pc);
  cnt = block_sum(sh, cnt);
  if (t == 0) {
    stats[2 * b] = pc;
    stats[2 * b + 1] = cnt;
  }
}

// ---------------------------------------------------------------------------------------------
// The backward pass.  Bwd holds what the reverse sweep adds to Prob.
struct Bwd {
  double* Cbar;  // [B][N][Npad] the gradient with respect to C, accumulated in place
  double* gx;    // [B][d][Npad] the incoming gradient, SoA
  double* xbar;  // [B][d][Npad] the row sums of the gradient with respect to X
  double* fbar;  // [B][Npad]
  double* gbar;  // [B][Npad]
  double* abar;  // [B][Npad]
  double* part;  // [B][S][Npad] partial column sums
};

// sum over the wave, in a fixed order, into every lane
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (ceil(B / PB)): K_b = the caller's iteration count clamped to 0 .. k_sweep.  The sweep reads
// no other count, so no kernel indexes the history outside the iterations 0 .. k_sweep.
__global__ void __launch_bounds__(PB) k_ot_bwd_counts(const int32_t* __restrict__ its, int32_t* __restrict__ K, int B,
                                                      int k_sweep) {
  const int b = blockIdx.x * PB + threadIdx.x;
  if (b < B) K[b] = min(max(its[b], 0), k_sweep);
}

// grid (ceil(N / PB), B).  G [B][N][d] (host layout) to gx.
__global__ void __launch_bounds__(PB) k_ot_bwd_load(Prob p, Bwd w, const double* __restrict__ G) {
  const int b = blockIdx.y, i = blockIdx.x * PB + threadIdx.x;
  const int N = p.N, d = p.d;
  if (i >= N) return;
  const size_t P = (size_t)p.Npad;
  const double* __restrict__ Gi = G + ((size_t)b * N + i) * d;
  double* __restrict__ gb = w.gx + (size_t)b * d * P;
  for (int k = 0; k < d; ++k) gb[(size_t)k * P + i] = Gi[k];
}

// grid (ceil(N / PB), ceil(N / CT), B): Cbar_ij <- N X_i . G_j, the loops of k_ot_cost
__global__ void __launch_bounds__(PB) k_ot_bwd_q(Prob p, Bwd w) {
  __shared__ double xs[KC * CT];
  const int t = threadIdx.x, b = blockIdx.z;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const int j = blockIdx.x * PB + t, i0 = blockIdx.y * CT;
  const int jc = min(j, N - 1);
  const double* __restrict__ xb = p.x + (size_t)b * d * P;
  const double* __restrict__ gb = w.gx + (size_t)b * d * P;
  double acc[CT];
#pragma unroll
  for (int r = 0; r < CT; ++r) acc[r] = 0.0;
  for (int k0 = 0; k0 < d; k0 += KC) {
    const int kc = min(KC, d - k0);
    for (int idx = t; idx < kc * CT; idx += PB) {
      const int k = idx / CT, r = idx - k * CT;
      xs[idx] = (i0 + r < N) ? xb[(size_t)(k0 + k) * P + i0 + r] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
      const double gj = gb[(size_t)(k0 + k) * P + jc];
#pragma unroll
      for (int r = 0; r < CT; ++r) acc[r] = fma(xs[k * CT + r], gj, acc[r]);
    }
    __syncthreads();
  }
  if (j >= N) return;
  double* __restrict__ Qb = w.Cbar + (size_t)b * N * P;
#pragma unroll
  for (int r = 0; r < CT; ++r)
    if (i0 + r < N) Qb[(size_t)(i0 + r) * P + j] = (double)N * acc[r];
}

// grid (ceil(N / RW), ceil(d / PC), B), PB lanes: wave w of the workgroup owns row i and the
// components [c0, c0 + NC) of chunk blockIdx.y.
// COST = false, the projection: P_ij recomputed from f^K, g^K; xbar_i = N sum_j P_ij G_j; chunk 0
//   turns the q_ij left in Cbar into -D_ij and sets fbar_i and abar_i.
// COST = true: xbar_i += 2 sum_j Cbar'_ij (x_i - x_j).
template <int NC, bool COST>
__global__ void __launch_bounds__(PB) k_ot_bwd_rowacc(Prob p, Bwd w, Hist hs, double inv_eps, double eps,
                                                      double min_val) {
  const int b = blockIdx.z, ch = blockIdx.y;
  const int lane = threadIdx.x & 63, i = blockIdx.x * RW + (threadIdx.x >> 6);
  const int N = p.N, d = p.d;
  if (i >= N) return;  // the whole wave
  const size_t P = (size_t)p.Npad;
  const int c0 = ch * PC, nc = min(NC, d - c0);
  const double* __restrict__ Ci = p.C + ((size_t)b * N + i) * P;
  double* __restrict__ Cbi = w.Cbar + ((size_t)b * N + i) * P;
  const double* __restrict__ vb = (COST ? p.x : w.gx) + ((size_t)b * d + c0) * P;
  double* __restrict__ xo = w.xbar + ((size_t)b * d + c0) * P + i;
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  if constexpr (COST) {
    double xi[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) xi[c] = c < nc ? vb[(size_t)c * P + i] : 0.0;
    for (int j = lane; j < N; j += 64) {
      const double cb = Ci[j] == 0.0 ? 0.0 : Cbi[j];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) acc[c] = fma(cb, xi[c] - vb[(size_t)c * P + j], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double v = wave_sum(acc[c]);
      if (lane == 0 && c < nc) xo[(size_t)c * P] += 2.0 * v;
    }
  } else {
    const int K = hs.K[b];
    const double fi = hist_at(hs, b, HF, K)[i];
    const double* __restrict__ gK = hist_at(hs, b, HG, K);
    const double ai = p.a[(size_t)b * P + i];
    const double ab = ai * (1.0 / (double)N);
    double rs = 0.0;
    for (int j = lane; j < N; j += 64) {
      const double raw = ab * exp(((fi + gK[j]) - Ci[j]) * inv_eps);
      const double pij = fmax(raw, min_val);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) acc[c] = fma(pij, vb[(size_t)c * P + j], acc[c]);
      if (ch == 0) {
        const double D = raw > min_val ? pij * Cbi[j] * inv_eps : 0.0;
        Cbi[j] = -D;
        rs += D;
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double v = wave_sum(acc[c]);
      if (lane == 0 && c < nc) xo[(size_t)c * P] = (double)N * v;
    }
    if (ch == 0) {
      rs = wave_sum(rs);
      if (lane == 0) {
        w.fbar[(size_t)b * P + i] = rs;
        w.abar[(size_t)b * P + i] = eps * rs / ai;
      }
    }
  }
}

// grid (ceil(N / RW), B), PB lanes: the g pass of iteration k for row i.
__global__ void __launch_bounds__(PB) k_ot_bwd_rows(Prob p, Bwd w, Hist hs, int k, double inv_eps, double eps) {
  const int b = blockIdx.y;
  if (k > hs.K[b]) return;
  const int lane = threadIdx.x & 63, i = blockIdx.x * RW + (threadIdx.x >> 6);
  const int N = p.N;
  if (i >= N) return;  // the whole wave
  const size_t P = (size_t)p.Npad;
  const double* __restrict__ Ci = p.C + ((size_t)b * N + i) * P;
  double* __restrict__ Cbi = w.Cbar + ((size_t)b * N + i) * P;
  const double* __restrict__ gbar = w.gbar + (size_t)b * P;
  const double* __restrict__ tg = hist_at(hs, b, HTG, k);
  const int32_t* __restrict__ am = hist_am(hs, b, k);
  const double fi = hist_at(hs, b, HF, k)[i];
  const double ai = p.a[(size_t)b * P + i];
  double dl = 0.0, da = 0.0;
#pragma unroll 4
  for (int j = lane; j < N; j += 64) {
    const int32_t m = am[j];
    const double s = m < 0 ? ai * exp(((fi + tg[j]) - Ci[j]) * inv_eps) : (m == i ? 1.0 : 0.0);
    const double v = (0.5 * gbar[j]) * s;
    Cbi[j] += v;
    dl += v;
    da += m < 0 ? v : 0.0;
  }
  dl = wave_sum(dl);
  da = wave_sum(da);
  if (lane == 0) {
    w.fbar[(size_t)b * P + i] -= dl;
    w.abar[(size_t)b * P + i] -= eps * da / ai;
  }
}

// grid (ceil(N / CB), S, B), CB lanes: lane j over the sources of split s, partial sums to w.part.
// FPASS = true, the f pass of iteration k: (t_i, tau_f_i) broadcast from LDS, Cbar_ij += t_i r_ij.
// FPASS = false: the column sums of Cbar.
template <bool FPASS>
__global__ void __launch_bounds__(CB) k_ot_bwd_cols(Prob p, Bwd w, Hist hs, int k, double inv_eps, int chunk, int S) {
  __shared__ double2 sh[FPASS ? TT : 1];
  const int b = blockIdx.z;
  if constexpr (FPASS) {
    if (k > hs.K[b]) return;
  }
  const int t = threadIdx.x, s = blockIdx.y;
  const int N = p.N;
  const size_t P = (size_t)p.Npad;
  const int j = blockIdx.x * CB + t, jc = min(j, N - 1);
  const int i0 = s * chunk, i1 = min(N, i0 + chunk);
  double* __restrict__ Cbj = w.Cbar + (size_t)b * N * P + jc;
  double sum = 0.0;
  if constexpr (FPASS) {
    const double* __restrict__ Cj = p.C + (size_t)b * N * P + jc;
    const double* __restrict__ fbar = w.fbar + (size_t)b * P;
    const double* __restrict__ tf = hist_at(hs, b, HTF, k);
    const double gj = hist_at(hs, b, HG, k - 1)[jc];
    const double bN = 1.0 / (double)N;
    for (int base = i0; base < i1; base += TT) {
      const int cnt = min(TT, i1 - base);
      for (int q = t; q < cnt; q += CB) sh[q] = make_double2(0.5 * fbar[base + q] * bN, tf[base + q]);
      __syncthreads();
#pragma unroll 4
      for (int q = 0; q < cnt; ++q) {
        const double2 tt = sh[q];
        const size_t o = (size_t)(base + q) * P;
        const double v = tt.x * exp(((gj + tt.y) - Cj[o]) * inv_eps);
        if (j < N) Cbj[o] += v;  // lanes past N would all hit column N - 1
        sum += v;
      }
      __syncthreads();
    }
  } else {
#pragma unroll 4
    for (int i = i0; i < i1; ++i) sum += Cbj[(size_t)i * P];
  }
  if (j < N) w.part[((size_t)b * S + s) * P + j] = sum;
}

// grid (ceil(N / PB), B).  mode 0: gbar_j = -sum_s part.  mode 1 (after the f pass of iteration k):
// gbar_j <- gbar_j / 2 - sum_s part, fbar_j <- fbar_j / 2.  The partials in the order s = 0..S-1.
__global__ void __launch_bounds__(PB) k_ot_bwd_merge(Prob p, Bwd w, Hist hs, int k, int mode, int S) {
  const int b = blockIdx.y;
  if (mode == 1 && k > hs.K[b]) return;
  const int j = blockIdx.x * PB + threadIdx.x;
  if (j >= p.N) return;
  const size_t P = (size_t)p.Npad;
  double sum = 0.0;
  for (int s = 0; s < S; ++s) sum += w.part[((size_t)b * S + s) * P + j];
  const size_t q = (size_t)b * P + j;
  if (mode == 0) {
    w.gbar[q] = -sum;
  } else {
    w.gbar[q] = 0.5 * w.gbar[q] - sum;
    w.fbar[q] = 0.5 * w.fbar[q];
  }
}

// grid (ceil(N / CB), ceil(d / PC) S, B), CB lanes, the shape of k_ot_project: output i, sources j
// of split s: part [B][S][d][Npad] = sum_j Cbar'_ji (x_i - x_j) over the chunk's components.
template <int NC>
__global__ void __launch_bounds__(CB) k_ot_bwd_cost_cols(Prob p, Bwd w, int chunk, int S, double* __restrict__ part) {
  __shared__ double sx[PT * NC];
  const int t = threadIdx.x;
  const int b = blockIdx.z, ch = blockIdx.y / S, s = blockIdx.y - ch * S;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const int i = blockIdx.x * CB + t, ic = min(i, N - 1);
  const int c0 = ch * PC, nc = min(NC, d - c0);
  const int j0 = s * chunk, j1 = min(N, j0 + chunk);
  const double* __restrict__ Ci = p.C + (size_t)b * N * P + ic;
  const double* __restrict__ Cbi = w.Cbar + (size_t)b * N * P + ic;
  const double* __restrict__ xb = p.x + ((size_t)b * d + c0) * P;
  double xi[NC], acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    xi[c] = c < nc ? xb[(size_t)c * P + ic] : 0.0;
    acc[c] = 0.0;
  }
  for (int base = j0; base < j1; base += PT) {
    const int cnt = min(PT, j1 - base);
    for (int idx = t; idx < NC * PT; idx += CB) {
      const int c = idx / PT, q = idx - c * PT;
      sx[q * NC + c] = (c < nc && q < cnt) ? xb[(size_t)c * P + base + q] : 0.0;
    }
    __syncthreads();
    for (int q = 0; q < cnt; ++q) {
      const size_t o = (size_t)(base + q) * P;
      const double cb = Ci[o] == 0.0 ? 0.0 : Cbi[o];
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = fma(cb, xi[c] - sx[q * NC + c], acc[c]);
    }
    __syncthreads();
  }
  if (i >= N) return;
  double* __restrict__ o = part + (((size_t)b * S + s) * d + c0) * P + i;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < nc) o[(size_t)c * P] = acc[c];
}

// grid (ceil(N d / PB), B): gX [B][N][d] = xbar + 2 sum_s part
__global__ void __launch_bounds__(PB) k_ot_bwd_finish(Prob p, Bwd w, int S, const double* __restrict__ part,
                                                      double* __restrict__ gX) {
  const int b = blockIdx.y;
  const int N = p.N, d = p.d;
  const size_t P = (size_t)p.Npad;
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= (int64_t)N * d) return;
  const int i = (int)(q / d), c = (int)(q - (int64_t)i * d);
  double v = 0.0;
  for (int s = 0; s < S; ++s) v += part[(((size_t)b * S + s) * d + c) * P + i];
  gX[(size_t)b * N * d + q] = w.xbar[((size_t)b * d + c) * P + i] + 2.0 * v;
}

// grid (ceil(N / PB), B): gw_i = [w_i > min_val] (abar_i - sum_k abar_k a_k) / (sum max(w, min_val) +
// min_val); every workgroup forms the two sums in the order of k_ot_prepare.
__global__ void __launch_bounds__(PB) k_ot_bwd_weights(Prob p, Bwd w, const double* __restrict__ wt, double min_val,
                                                       double* __restrict__ gw) {
  __shared__ double sh[PB];
  const int t = threadIdx.x, b = blockIdx.y;
  const int N = p.N;
  const size_t P = (size_t)p.Npad;
  const double* __restrict__ wb = wt + (size_t)b * N;
  const double* __restrict__ ab = p.a + (size_t)b * P;
  const double* __restrict__ abar = w.abar + (size_t)b * P;
  double s = 0.0, dot = 0.0;
  for (int i = t; i < N; i += PB) {
    s += fmax(wb[i], min_val);
    dot = fma(abar[i], ab[i], dot);
  }
  const double total = block_sum(sh, s);
  dot = block_sum(sh, dot);
  const int i = blockIdx.x * PB + t;
  if (i >= N) return;
  gw[(size_t)b * N + i] = wb[i] > min_val ? (abar[i] - dot) / (total + min_val) : 0.0;
}

}  // namespace ot
}  // namespace pf
