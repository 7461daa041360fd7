// Dense LEDH particle-flow kernel for gfx950 (fp64, wave64): the sensor-network models with
// h(x) = m1 exp(m2 x), where every particle linearises h at its own position (the reference's
// LEDHFlowPF.step, models/LEDH_particle_filter.py:136-179, cited "ledh.py:LINE").
//
// The Jacobian is diagonal, H_i = diag(D), D = m1 m2 exp(m2 eta), so with the tracker's P
//   S  = lam  (D D^T o P) + R          (ledh.py:149, an elementwise scaling of P, never stored unfactored)
//   A v = -1/2 P (D o S^-1 (D o v))    (ledh.py:159; A is never formed)
//   y  = P (D o R^-1 (z - e)),  e = h(eta) - D o eta
//   t1 = y + lam A y + A eta_0,  b = t1 + 2 lam A t1          (ledh.py:165)
//   eta += dlam (A eta + b)                                    (ledh.py:171)
//   theta += log det(I + dlam A) = log det S' - log det S,  S' = (lam - dlam/2)(D D^T o P) + R
// (Sylvester's identity; both are SPD, so the determinant is positive and ledh.py:176-178 cannot fire).
// Per lambda step that is two Cholesky factorisations, two rounds of triangular solves with the
// factor of S (right-hand sides {y, eta_0, eta}, then {t1}) and five products with P.
//
// One 256-thread workgroup runs the whole lambda loop of one particle; its vectors live in LDS and its
// two factors in a global workspace of 2 d^2 doubles (d = 400 is 1.28 MB per factor).
//
// Cholesky: blocked by NB = 16 columns, left-looking.  For block column k the product of the
// finished panels L[k.., 0..k) L[k, 0..k)^T - the d^3/3 part - is taken on v_mfma_f64_16x16x4 in
// 16 x 16 tiles, one wave per tile, with the fragment layout of k_dense_gemm (A lane l holds
// A[l & 15][l >> 4], B lane l holds B[l >> 4][l & 15], results D[(l >> 4) + 4 r][l & 15]); S minus
// that product is the updated column.  Its diagonal tile is factored by one wave in registers and
// published through LDS; the panel below is solved against it one row per thread (plain VALU).
// Triangular solves: blocks of TS = 32 staged in LDS, one wave per right-hand side inside the block,
// one thread per row for the update of the rest.  All sums have a fixed order: two runs are bitwise
// equal, and so are runs with different chunkings of the particles.
//
// A pivot that is not finite and positive sets the particle's failure flag and ends its flow; no
// index depends on a value, so such a particle reads and writes only its own rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pf_edh_dense_kernels.h"

namespace pf {
namespace ledh_dense {

using edh_dense::d4;

constexpr int LB = 256;      // threads per particle
constexpr int NB = 16;       // Cholesky panel width = the MFMA tile
constexpr int TS = 32;       // triangular-solve block
constexpr int NVEC = 10;     // d-vectors in LDS: eta eta0 D y a0 a1 a2 b0 b1 b2
constexpr int LDS_FIXED = NB * (NB + 1) + TS * (TS + 1) + 8;  // doubles: panel tile, solve block, scalars

inline size_t lds_bytes(int d) { return ((size_t)NVEC * d + LDS_FIXED) * sizeof(double); }

struct FlowArgs {
  int n, d, L;             // particles of this launch, state dimension, lambda steps
  int64_t first;           // global index of this launch's particle 0
  double alpha, m1, m2;
  const double* X;         // [N][d] x_{k-1}
  const double* u;         // [d] or null
  const double* v;         // [N][d] or null
  const double* P;         // [d][d] symmetric
  const double* z;         // [d]
  const double* rdiag;     // [d] the flow's R (diagonal, positive)
  double* ws;              // [n][2][d][d] factors of S and S'
  double* Xn;              // [N][d] x_k = eta(lambda = 1)
  double* theta;           // [N]
  int* fail;               // [N] 1 where a pivot failed
  int* nfail;              // [1] number of failed particles of the step (atomic)
  double* trace;           // [L][d] eta of global particle 0 before each lambda step, or null
};

// What the factorisation reads of S = coef (D D^T o P) + diag(rdiag).  A struct by reference, not three
// scalars: with scalars k_ledh_flow compiled to different code and measured 0.5 % slower at d = 400.
struct SpdArgs {
  int d;
  const double* P;      // [d][d] symmetric
  const double* rdiag;  // [d] positive
};

// S(i, j) for i, j < d; the identity outside (padding of the last tile)
__device__ __forceinline__ double s_elem(const SpdArgs& a, const double* D, double coef, int i, int j) {
  if (i >= a.d || j >= a.d) return i == j ? 1.0 : 0.0;
  double s = coef * (D[i] * D[j] * a.P[(size_t)i * a.d + j]);
  if (i == j) s += a.rdiag[i];
  return s;
}

// Lower Cholesky factor of coef (D D^T o P) + diag(rdiag) into W [d][d]; the part of W above the diagonal is
// neither written nor read (the products read columns left of a row's diagonal tile only).
// Returns sum log diag; *bad (LDS) is set on a failed pivot.  Every thread of the block calls it.
__device__ __forceinline__ double chol_factor(const SpdArgs& a, const double* D, double coef, double* W, double* tile, double* sc,
                              int* bad) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = a.d;
  const int ntile = (d + NB - 1) / NB;
  double logdet = 0.0;  // kept by every thread of wave 0 (uniform)
  for (int kt = 0; kt < ntile; ++kt) {
    const int k0 = kt * NB;
    // (a) column block k minus the product of the finished panels
    for (int it = kt + wv; it < ntile; it += LB / 64) {
      const int i0 = it * NB;
      const int ra = i0 + (lane & 15), rb = k0 + (lane & 15);
      const double* pa = W + (size_t)min(ra, d - 1) * d + (lane >> 4);
      const double* pb = W + (size_t)min(rb, d - 1) * d + (lane >> 4);
      const bool oka = ra < d, okb = rb < d;
      d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
      for (int kk = 0; kk < k0; kk += 4) {
        const double fa = oka ? pa[kk] : 0.0;
        const double fb = okb ? pb[kk] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb, acc, 0, 0, 0);
      }
      for (int r = 0; r < 4; ++r) {
        const int m = (lane >> 4) + 4 * r, n = lane & 15;
        const int row = i0 + m, col = k0 + n;
        const double val = s_elem(a, D, coef, row, col) - acc[r];
        if (it == kt)
          tile[m * (NB + 1) + n] = val;
        else if (row < d && col < d)
          W[(size_t)row * d + col] = val;
      }
    }
    __syncthreads();
    // (b) the diagonal tile: lane i of wave 0 holds row i
    if (wv == 0) {
      const int i = lane & 15;
      double row[NB];
#pragma unroll
      for (int c = 0; c < NB; ++c) row[c] = tile[i * (NB + 1) + c];
      bool fl = false;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const double piv = __shfl(row[j], j, 64);
        if (!(piv > 0.0) || !(piv < INFINITY)) fl = true;
        const double ljj = sqrt(piv);
        if (k0 + j < d) logdet += log(ljj);
        row[j] = (i == j) ? ljj : row[j] / ljj;
#pragma unroll
        for (int c = j + 1; c < NB; ++c) {
          const double lcj = __shfl(row[j], c, 64);
          row[c] -= row[j] * lcj;
        }
      }
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        const double val = c <= i ? row[c] : 0.0;
        if (lane < NB) {
          tile[i * (NB + 1) + c] = val;
          if (c <= i && k0 + i < d) W[(size_t)(k0 + i) * d + k0 + c] = val;
        }
      }
      if (fl && lane == 0) *bad = 1;
    }
    __syncthreads();
    // (c) the panel below: row r of L21 solves x L11^T = (updated row), one row per thread
    for (int r = k0 + NB + tid; r < d; r += LB) {
      double* wr = W + (size_t)r * d + k0;
      double x[NB];
#pragma unroll
      for (int c = 0; c < NB; ++c) x[c] = wr[c];
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        double s = x[c];
#pragma unroll
        for (int m = 0; m < c; ++m) s -= x[m] * tile[c * (NB + 1) + m];
        x[c] = s / tile[c * (NB + 1) + c];
      }
#pragma unroll
      for (int c = 0; c < NB; ++c) wr[c] = x[c];
    }
    __syncthreads();
  }
  if (tid == 0) sc[0] = logdet;
  __syncthreads();
  return sc[0];
}

// In place S^-1 on NR vectors of LDS (a0, a1, a2): forward with L, then backward with L^T.
// Always inlined: the vectors and blk are LDS, and only inlined does the compiler address them with DS
// instructions.  Out of line they become generic pointers, and the flat loads of the backward pass
// take bases below blk, which leave the LDS aperture when blk lies near the start of LDS.
template <int NR>
__device__ __forceinline__ void chol_solve(int d, const double* W, double* a0, double* a1, double* a2, double* blk) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 31;
  const int nblk = (d + TS - 1) / TS;
  double* mine = wv == 0 ? a0 : (wv == 1 ? a1 : a2);
  for (int pass = 0; pass < 2; ++pass) {
    for (int bi = 0; bi < nblk; ++bi) {
      const int b0 = (pass == 0 ? bi : nblk - 1 - bi) * TS;
      for (int e = tid; e < TS * TS; e += LB) {
        const int i = e / TS, j = e % TS;
        double val = i == j ? 1.0 : 0.0;
        if (j <= i && b0 + i < d) val = W[(size_t)(b0 + i) * d + b0 + j];
        blk[i * (TS + 1) + j] = val;
      }
      __syncthreads();
      if (wv < NR) {
        double r = b0 + li < d ? mine[b0 + li] : 0.0;
        if (pass == 0) {
          for (int j = 0; j < TS; ++j) {
            const double xj = __shfl(r, j, 64) / blk[j * (TS + 1) + j];
            if (li == j) r = xj;
            if (li > j) r -= blk[li * (TS + 1) + j] * xj;
          }
        } else {
          for (int j = TS - 1; j >= 0; --j) {
            const double xj = __shfl(r, j, 64) / blk[j * (TS + 1) + j];
            if (li == j) r = xj;
            if (li < j) r -= blk[j * (TS + 1) + li] * xj;
          }
        }
        if (lane < TS && b0 + li < d) mine[b0 + li] = r;
      }
      __syncthreads();
      if (pass == 0) {  // rows below the block; their columns b0 .. b0 + TS - 1 exist
        for (int i = b0 + TS + tid; i < d; i += LB) {
          const double* wr = W + (size_t)i * d + b0;
          double s0 = 0.0, s1 = 0.0, s2 = 0.0;
          for (int j = 0; j < TS; ++j) {
            const double l = wr[j];
            s0 += l * a0[b0 + j];
            if (NR > 1) s1 += l * a1[b0 + j];
            if (NR > 2) s2 += l * a2[b0 + j];
          }
          a0[i] -= s0;
          if (NR > 1) a1[i] -= s1;
          if (NR > 2) a2[i] -= s2;
        }
      } else {  // rows above the block, through the transpose
        const int nb = min(TS, d - b0);
        for (int i = tid; i < b0; i += LB) {
          double s0 = 0.0, s1 = 0.0, s2 = 0.0;
          for (int j = 0; j < nb; ++j) {
            const double l = W[(size_t)(b0 + j) * d + i];
            s0 += l * a0[b0 + j];
            if (NR > 1) s1 += l * a1[b0 + j];
            if (NR > 2) s2 += l * a2[b0 + j];
          }
          a0[i] -= s0;
          if (NR > 1) a1[i] -= s1;
          if (NR > 2) a2[i] -= s2;
        }
      }
      __syncthreads();
    }
  }
}

constexpr int SOLVE_RHS = 3;  // right-hand sides of one workgroup of k_chol_solve (chol_solve<3>)

inline size_t solve_lds_bytes(int d) { return ((size_t)SOLVE_RHS * d + TS * (TS + 1)) * sizeof(double); }

// Rows 3 g .. 3 g + 2 of out = B S^-1 from the factor W of S: row r solves S y = B[r][.]^T.  With B null
// the right-hand sides are the unit vectors, so out = S^-1 (symmetric: its columns are stored as rows).
__global__ __launch_bounds__(LB) void k_chol_solve(int d, const double* W, const double* B, double* out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* a0 = lds;
  double* a1 = a0 + d;
  double* a2 = a1 + d;
  double* blk = a2 + d;
  const int c0 = (int)blockIdx.x * SOLVE_RHS;  // < d: the grid has ceil(d / SOLVE_RHS) workgroups
  for (int j = threadIdx.x; j < d; j += LB) {
    a0[j] = B ? B[(size_t)c0 * d + j] : (j == c0 ? 1.0 : 0.0);
    a1[j] = c0 + 1 < d ? (B ? B[(size_t)(c0 + 1) * d + j] : (j == c0 + 1 ? 1.0 : 0.0)) : 0.0;
    a2[j] = c0 + 2 < d ? (B ? B[(size_t)(c0 + 2) * d + j] : (j == c0 + 2 ? 1.0 : 0.0)) : 0.0;
  }
  __syncthreads();
  chol_solve<SOLVE_RHS>(d, W, a0, a1, a2, blk);  // ends with a barrier
  for (int j = threadIdx.x; j < d; j += LB) {
    out[(size_t)c0 * d + j] = a0[j];
    if (c0 + 1 < d) out[(size_t)(c0 + 1) * d + j] = a1[j];
    if (c0 + 2 < d) out[(size_t)(c0 + 2) * d + j] = a2[j];
  }
}

// out_k = P in_k for NR vectors of LDS; P is symmetric, so thread c walks column c (coalesced)
template <int NR>
__device__ void p_times(int d, const double* P, const double* i0, const double* i1, const double* i2, double* o0,
                        double* o1, double* o2) {
  for (int c = threadIdx.x; c < d; c += LB) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < d; ++j) {
      const double p = P[(size_t)j * d + c];
      s0 += p * i0[j];
      if (NR > 1) s1 += p * i1[j];
      if (NR > 2) s2 += p * i2[j];
    }
    o0[c] = s0;
    if (NR > 1) o1[c] = s1;
    if (NR > 2) o2[c] = s2;
  }
  __syncthreads();
}

__global__ __launch_bounds__(LB) void k_ledh_flow(FlowArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, d = a.d;
  double* eta = lds;
  double* eta0 = eta + d;
  double* D = eta0 + d;
  double* y = D + d;
  double* a0 = y + d;
  double* a1 = a0 + d;
  double* a2 = a1 + d;
  double* b0 = a2 + d;
  double* b1 = b0 + d;
  double* b2 = b1 + d;
  double* tile = b2 + d;
  double* blk = tile + NB * (NB + 1);
  double* sc = blk + TS * (TS + 1);
  int* bad = (int*)(sc + 4);

  const int64_t gi = a.first + blockIdx.x;
  double* W0 = a.ws + (size_t)blockIdx.x * 2 * d * d;
  double* W1 = W0 + (size_t)d * d;
  for (int j = tid; j < d; j += LB) {
    const size_t o = (size_t)gi * d + j;
    double e0 = a.alpha * a.X[o];
    if (a.u) e0 += a.u[j];
    if (a.v) e0 += a.v[o];
    eta0[j] = e0;
    eta[j] = e0;
  }
  if (tid == 0) *bad = 0;
  __syncthreads();

  const SpdArgs sa{d, a.P, a.rdiag};
  const double dlam = 1.0 / (double)a.L;
  double lam = 0.0, theta = 0.0;
  bool failed = false;
  for (int step = 0; step < a.L; ++step) {
    lam = fmin(1.0, lam + dlam);
    for (int j = tid; j < d; j += LB) {
      const double x = eta[j];
      if (a.trace && gi == 0) a.trace[(size_t)step * d + j] = x;
      const double hx = a.m1 * exp(a.m2 * x);
      const double Dj = a.m2 * hx;
      D[j] = Dj;
      a0[j] = Dj * ((a.z[j] - (hx - Dj * x)) / a.rdiag[j]);
    }
    __syncthreads();
    const double ld1 = chol_factor(sa, D, lam - 0.5 * dlam, W1, tile, sc, bad);
    const double ld0 = chol_factor(sa, D, lam, W0, tile, sc, bad);
    if (*bad) {  // uniform: read after the barrier that ends chol_factor
      failed = true;
      break;
    }
    theta += 2.0 * (ld1 - ld0);
    p_times<1>(d, a.P, a0, a0, a0, y, y, y);  // y = P (D o R^-1 (z - e))
    for (int j = tid; j < d; j += LB) {
      a0[j] = D[j] * y[j];
      a1[j] = D[j] * eta0[j];
      a2[j] = D[j] * eta[j];
    }
    __syncthreads();
    chol_solve<3>(d, W0, a0, a1, a2, blk);
    for (int j = tid; j < d; j += LB) {
      a0[j] *= D[j];
      a1[j] *= D[j];
      a2[j] *= D[j];
    }
    __syncthreads();
    p_times<3>(d, a.P, a0, a1, a2, b0, b1, b2);  // A y = -b0 / 2, A eta_0 = -b1 / 2, A eta = -b2 / 2
    for (int j = tid; j < d; j += LB) {
      const double t1 = y[j] - 0.5 * lam * b0[j] - 0.5 * b1[j];
      y[j] = t1;
      a0[j] = D[j] * t1;
    }
    __syncthreads();
    chol_solve<1>(d, W0, a0, a0, a0, blk);
    for (int j = tid; j < d; j += LB) a0[j] *= D[j];
    __syncthreads();
    p_times<1>(d, a.P, a0, a0, a0, b0, b0, b0);  // A t1 = -b0 / 2
    for (int j = tid; j < d; j += LB) {
      const double b = y[j] - lam * b0[j];
      eta[j] += dlam * (-0.5 * b2[j] + b);
    }
    __syncthreads();
  }
  for (int j = tid; j < d; j += LB) a.Xn[(size_t)gi * d + j] = eta[j];
  if (tid == 0) {
    a.theta[gi] = theta;
    a.fail[gi] = failed ? 1 : 0;
    if (failed) atomicAdd(a.nfail, 1);
  }
}

}  // namespace ledh_dense
}  // namespace pf
