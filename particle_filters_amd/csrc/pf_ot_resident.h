// The one-launch Sinkhorn solver for N <= 128 (PF_OT_RESIDENT of pf_ot_resample_dev; host side
// pf_ot.hip, shape and LDS layout pf_ot_resident_plan.h).
//
// k_ot_resident, grid (B), RES_THREADS lanes: one workgroup per problem does what the launch sequence
// of pf_ot_kernels.h does, with the cost matrix in LDS and __syncthreads() as the only
// synchronisation (no grid barrier, no atomics, no cooperative launch):
//   the weight normalisation and |x|^2                                               k_ot_prepare
//   C_ij = max((|x_i|^2 - 2 x_i.x_j) + |x_j|^2, 0) into LDS, X read through L2         k_ot_cost
//   per iteration the f pass (a wave per row, lanes along the row), the g pass (lanes along j, the
//   source range split over the waves of a column, partials through LDS), their merge in the order
//   s = 0 .. S - 1, the change of f and g and the stopping rule, decided by wave 0 and read by every
//   lane behind a barrier: workgroup-uniform              k_ot_tau_rows / _cols / _merge / k_ot_check
//   the dual history and the floor argmax, when asked for                    the recording modes
//   the plan P_ij over C in place, its statistics                        k_ot_project / k_ot_stats
//   X_out_j = (sum_i P_ij X_i) / b, a lane per (j, component), i ascending  k_ot_project / k_ot_finish
// Tau is evaluated as there: the maximum first, then the sum.  Every sum runs in an order fixed by N
// alone, so two calls are bitwise equal and problem b of a batch is bitwise that problem alone.  The
// sums are not in the launch sequence's order (its waves and splits differ), so the two solvers
// agree to rounding, not bitwise.  Both passes read C along its rows, consecutive lanes 8 bytes
// apart: conflict-free ds_read_b64 in both 32-lane groups.  One workgroup per CU (up to 154 KiB of
// LDS), sixteen waves, four per SIMD, to overlap the fp64 exp / log chains that bound each pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pf_ot_kernels.h"
#include "pf_ot_resident_plan.h"

namespace pf {
namespace ot {

struct Resident {
  const double* X;  // [B][N][d]
  const double* w;  // [B][N]
  double* X_out;    // [B][N][d]
  double* f;        // [B][npad] the duals of the stopping iteration
  double* g;        // [B][npad]
  int* iters;       // [B]
  double* changes;  // [B][n_iters][2], zeroed by the host
  double* stats;    // [B][2], or null
  Hist rec;         // v null: no history; otherwise cleared by the host, kcap = n_iters
  int N, d, n_iters;
  double eps, inv_eps, min_val, tol;
};

// the sum of v over the workgroup, in a fixed order, into every lane; red [RES_THREADS] is overwritten
__device__ inline double res_block_sum(double* red, double v) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = RES_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ inline double res_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ void __launch_bounds__(RES_THREADS) k_ot_resident(Resident q) {
  extern __shared__ __align__(16) unsigned char lds[];
  const ResidentPlan pl = resident_plan(q.N);
  double* __restrict__ C = (double*)(lds + pl.C);
  double* __restrict__ a = (double*)(lds + pl.a);
  double* __restrict__ f = (double*)(lds + pl.f);
  double* __restrict__ g = (double*)(lds + pl.g);
  double* __restrict__ fold = (double*)(lds + pl.fold);
  double* __restrict__ gold = (double*)(lds + pl.gold);
  double* __restrict__ x2 = (double*)(lds + pl.x2);
  double* pm = (double*)(lds + pl.pm);  // no __restrict__: red aliases them
  double* ps = (double*)(lds + pl.ps);
  int32_t* __restrict__ pam = (int32_t*)(lds + pl.pam);
  int32_t* __restrict__ flag = (int32_t*)(lds + pl.flag);
  double* red = (double*)(lds + pl.red);  // aliases pm .. ps

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.x;
  const int N = q.N, d = q.d, P = pl.npad, sh = P == 64 ? 6 : 7;  // P is 64 or 128
  const double inv_eps = q.inv_eps, eps = q.eps, min_val = q.min_val;
  const double* __restrict__ Xb = q.X + (size_t)b * N * d;
  const double* __restrict__ wb = q.w + (size_t)b * N;

  // the weights, |x|^2, f = g = 0; the tails of the vectors are zero
  const double wi = t < N ? fmax(wb[t], min_val) : 0.0;
  const double total = res_block_sum(red, wi);
  if (t < P) {
    double sq = 0.0;
    if (t < N)
      for (int k = 0; k < d; ++k) {
        const double v = Xb[(size_t)t * d + k];
        sq += v * v;
      }
    a[t] = t < N ? wi / (total + min_val) : 0.0;
    x2[t] = sq;
    f[t] = g[t] = fold[t] = gold[t] = 0.0;
  }
  __syncthreads();

  // the cost matrix; padding columns are zero and never read
  for (int e = t; e < N * P; e += RES_THREADS) {
    const int i = e >> sh, j = e - (i << sh);
    double c = 0.0;
    if (j < N) {
      const double* __restrict__ xi = Xb + (size_t)i * d;
      const double* __restrict__ xj = Xb + (size_t)j * d;
      double acc = 0.0;
      for (int k = 0; k < d; ++k) acc = fma(xi[k], xj[k], acc);
      c = fmax((x2[i] - 2.0 * acc) + x2[j], 0.0);
    }
    C[e] = c;
  }
  __syncthreads();

  const double bj = 1.0 / (double)N;
  const bool rec = q.rec.v != nullptr;
  const int cw = wv % pl.ncw, sp = wv / pl.ncw;  // the g pass: column wave and split of this wave
  const int gj = cw * 64 + lane, gjc = min(gj, N - 1);
  const int i0 = min(N, sp * pl.chunk), i1 = min(N, i0 + pl.chunk);
  int K = 0;
  for (int it = 0; it < q.n_iters; ++it) {
    const int k = it + 1;
    // f_i <- (f_i + Tau(b, g, C[i, :])) / 2
    for (int i = wv; i < N; i += RES_WAVES) {
      const double* __restrict__ Ci = C + (i << sh);
      double mx = -INFINITY;
      for (int j = lane; j < N; j += 64) mx = fmax(mx, (g[j] - Ci[j]) * inv_eps);
      mx = res_wave_max(mx);
      double s = 0.0;
      for (int j = lane; j < N; j += 64) s += bj * exp((g[j] - Ci[j]) * inv_eps - mx);
      s = wave_sum(s);
      if (lane == 0) {
        const double fo = f[i];
        const double tau = tau_value(s, mx, eps, min_val);
        const double fn = 0.5 * (fo + tau);
        fold[i] = fo;
        f[i] = fn;
        if (rec) {
          hist_at(q.rec, b, HF, k)[i] = fn;
          hist_at(q.rec, b, HTF, k)[i] = tau;
        }
      }
    }
    __syncthreads();
    // the g pass: (max, sum, argmax) of column j over the sources [i0, i1)
    {
      double mx = -INFINITY;
      int32_t am = i0;
      for (int i = i0; i < i1; ++i) {
        const double e = (f[i] - C[(i << sh) + gjc]) * inv_eps;
        if (e > mx) {
          mx = e;
          am = i;
        }
      }
      double sum = 0.0;
      for (int i = i0; i < i1; ++i) sum += a[i] * exp((f[i] - C[(i << sh) + gjc]) * inv_eps - mx);
      if (gj < N) {
        pm[sp * P + gj] = mx;
        ps[sp * P + gj] = sum;
        pam[sp * P + gj] = am;
      }
    }
    __syncthreads();
    // g_j <- (g_j + Tau(a, f, C[:, j])) / 2 from the partials; an empty split holds (-inf, 0)
    if (t < N) {
      double mx = -INFINITY;
      int32_t am = 0;
      for (int s = 0; s < pl.S; ++s)
        if (pm[s * P + t] > mx) {
          mx = pm[s * P + t];
          am = pam[s * P + t];
        }
      double sum = 0.0;
      for (int s = 0; s < pl.S; ++s) sum += ps[s * P + t] * exp(pm[s * P + t] - mx);
      const double go = g[t];
      const double tau = tau_value(sum, mx, eps, min_val);
      const double gn = 0.5 * (go + tau);
      gold[t] = go;
      g[t] = gn;
      if (rec) {
        hist_at(q.rec, b, HG, k)[t] = gn;
        hist_at(q.rec, b, HTG, k)[t] = tau;
        hist_am(q.rec, b, k)[t] = sum > min_val ? -1 : am;
      }
    }
    __syncthreads();
    // the changes and the stopping rule (ot.py:166-181), by wave 0
    if (wv == 0) {
      double fc = 0.0, gc = 0.0;
      for (int j = lane; j < N; j += 64) {
        fc = fmax(fc, fabs(f[j] - fold[j]));
        gc = fmax(gc, fabs(g[j] - gold[j]));
      }
      fc = res_wave_max(fc);
      gc = res_wave_max(gc);
      if (lane == 0) {
        int32_t stop = 0;
        if (it > 0) {
          q.changes[((size_t)b * q.n_iters + it) * 2] = fc;
          q.changes[((size_t)b * q.n_iters + it) * 2 + 1] = gc;
          stop = fc < q.tol && gc < q.tol;
        }
        flag[0] = stop;
      }
    }
    __syncthreads();
    K = k;
    if (flag[0]) break;  // every lane reads the same word behind the barrier: uniform
  }

  if (t == 0) q.iters[b] = K;
  if (t < N) {
    q.f[(size_t)b * P + t] = f[t];
    q.g[(size_t)b * P + t] = g[t];
  }

  // the plan over C, in place, and its statistics
  const double bN = 1.0 / (double)N;
  double pc = 0.0, cnt = 0.0;
  for (int e = t; e < N * P; e += RES_THREADS) {
    const int i = e >> sh, j = e - (i << sh);
    if (j < N) {
      const double cij = C[e];
      const double pij = fmax((a[i] * bN) * exp(((f[i] + g[j]) - cij) * inv_eps), min_val);
      pc = fma(pij, cij, pc);
      cnt += (pij > SPARSITY_THRESHOLD) ? 1.0 : 0.0;
      C[e] = pij;
    }
  }
  __syncthreads();
  if (q.stats) {
    pc = res_block_sum(red, pc);
    cnt = res_block_sum(red, cnt);
    if (t == 0) {
      q.stats[2 * b] = pc;
      q.stats[2 * b + 1] = cnt;
    }
  }

  // the barycentric projection: a lane per (component c, target j), the sources in ascending order;
  // a wave's lanes share c, so X_i[c] is one address per wave
  double* __restrict__ Xo = q.X_out + (size_t)b * N * d;
  for (int o = t; o < (d << sh); o += RES_THREADS) {
    const int c = o >> sh, j = o - (c << sh);
    if (j < N) {
      double acc = 0.0;
      for (int i = 0; i < N; ++i) acc = fma(C[(i << sh) + j], Xb[(size_t)i * d + c], acc);
      Xo[(size_t)j * d + c] = acc / bN;
    }
  }
}

}  // namespace ot
}  // namespace pf
