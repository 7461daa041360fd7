// Dense unscented Kalman tracker for gfx950 (fp64, wave64): the tracker of the sensor-network flows
// (trackers.UnscentedKalmanFilter.predict / update, the reference's models/unscented_kalman_filter.py:
// 95-192, cited "ukf.py:LINE") with its state on the device, runtime shape 1 <= d <= 1024, nz = nx.
//
// g(x) = alpha x (+ u) and h (identity or m1 exp(m2 x)) are elementwise, so the image of a sigma point is
// taken component by component (image(), image_pair()): a later elementwise nonlinear g changes those
// pointwise functions only.
//
// Per predict / update (ukf.py:107-126): sym(P), L = chol(sym(P) + jitter I) with one retry at
// max(jitter, 1e-12) decided on the device (k_ukf_chol returns at entry when the first launch succeeded),
// the sigma points m, m +- gamma L_i, their images Z_k, and then
//   zbar = Z_0 + w sum_i ((Z_i - Z_0) + (Z_{i+d} - Z_0))                  w = 1 / (2 (d + lambda))
// The unscented weights are Wm_0 ~ -1e6, Wm_i ~ +1e6 / 2d for the notebooks' alpha = 1e-3, so the plain
// weighted mean cancels six digits; centred on point 0 with the +- pair added first it does not.  The same
// holds for the covariance sums: with E_k = Z_k - Z_0 and delta = Z_0 - zbar
//   sum_k Wc_k (Z_k - zbar)(Z_k - zbar)^T = w sum_{k>=1} E_k E_k^T + (sum Wc - 2) delta delta^T
//   sum_k Wc_k (X_k - m)(Z_k - zbar)^T    = w sum_{k>=1} DX_k E_k^T           (sum_k DX_k = 0)
// Both are one product kernel over the sigma index (k_ukf_prod):
//   out = base + sum_k w_k A[k][.]^T B[k][.],  A, B [2d + 1][d],  w_0 = w0, w_k = w,
// with row 0 of E holding delta and row 0 of DX zero.  Both operands are K-slow in memory and K = 2d + 1
// is never a multiple of the K chunk.  It runs on v_mfma_f64_16x16x4 with the tiles, the inner loop and the
// fragment map of k_dense_gemm / k_fm_gemm (edh_dense::mfma_chunk, tile_row / tile_col); row 0 is added in the epilogue.
//
// The update's gain K = Pxz S^-1 is a Cholesky factorisation of sym(S) + jitter I and two triangular
// solves per row of Pxz (ledh_dense::k_chol_solve with Pxz as its right-hand sides, three per workgroup);
// K S K^T is two of the existing products.  The factorisation is ledh_dense::chol_factor.
//
// Every sum has a fixed order, so two runs are bitwise equal; no index depends on a value.  A step whose
// factorisation failed leaves the state as it was (k_ukf_commit reads the flags).  Stored covariances
// are exactly symmetric.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pf_edh_dense_kernels.h"
#include "pf_ledh_dense_kernels.h"

namespace pf {
namespace ukf_dense {

using edh_dense::d4;
using edh_dense::GB;
using edh_dense::KC;
using edh_dense::LDT;
using edh_dense::TM;
using edh_dense::TN;
using ledh_dense::LB;
using ledh_dense::NB;

constexpr int NFLAG = 4;  // flags of one predict / update: sigma factor, its retry, factor of S, spare
enum { F_SCALE = 0, F_IDENTITY = 1, F_EXP = 2 };

// the elementwise model function: a x (+ u_j) in NumPy's two roundings, x, or a exp(b x)
struct Fn {
  int kind;
  double a, b;
  const double* u;  // [d] or null (F_SCALE)
};

__device__ __forceinline__ double image(const Fn& f, double x, int j) {
  if (f.kind == F_EXP) return f.a * exp(f.b * x);
  if (f.kind == F_IDENTITY) return x;
  const double y = __dmul_rn(f.a, x);
  return f.u ? __dadd_rn(y, f.u[j]) : y;
}

// The images of the pair x +- c relative to the image z0 of x: f(x + c) - z0, f(x - c) - z0 and their sum,
// each without the rounding of x +- c, which the weight w ~ 1e6 / 2d would otherwise magnify: for the
// affine functions the differences are +- a c and cancel exactly, and a exp(b (x +- c)) - z0 =
// z0 expm1(+- b c), with the sum 4 z0 sinh^2(b c / 2).
struct Pair {
  double ep, em, sum;
};

__device__ __forceinline__ Pair image_pair(const Fn& f, double z0, double c) {
  Pair p;
  if (f.kind == F_EXP) {
    const double bc = f.b * c, sh = sinh(0.5 * bc);
    p.ep = z0 * expm1(bc);
    p.em = z0 * expm1(-bc);
    p.sum = 4.0 * z0 * (sh * sh);
  } else {
    p.ep = f.kind == F_IDENTITY ? c : f.a * c;
    p.em = -p.ep;
    p.sum = 0.0;
  }
  return p;
}

// out = 0.5 (X + X^T)
__global__ void k_ukf_sym(int d, const double* X, double* out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)d * d) return;
  const int i = (int)(e / d), j = (int)(e % d);
  out[e] = 0.5 * (X[e] + X[(size_t)j * d + i]);
}

// Lower Cholesky factor of P + diag(jit) into W; flags[slot] = 1 on a failed pivot.  With pre >= 0 the
// launch returns at entry unless flags[pre] is set: the retry of a failed factorisation.
__global__ __launch_bounds__(LB) void k_ukf_chol(int d, const double* P, const double* ones, const double* jit,
                                                 double* W, int* flags, int pre, int slot) {
  __shared__ double tile[NB * (NB + 1)];
  __shared__ double sc[4];
  __shared__ int bad;
  if (pre >= 0 && flags[pre] == 0) return;  // uniform
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  ledh_dense::chol_factor(ledh_dense::SpdArgs{d, P, jit}, ones, 1.0, W, tile, sc, &bad);  // 1 (1 1 P) + jit; ends with a barrier
  if (threadIdx.x == 0) flags[slot] = bad ? 1 : 0;
}

struct SigmaArgs {
  int d, chunk;      // chunk: columns of L per blockIdx.y
  double gamma;
  Fn f;
  const double* m;   // [d]
  const double* W;   // [d][d] lower factor; the part above the diagonal is not read
  double* E;         // [2d + 1][d] images minus the image of point 0 (row 0 is written by k_ukf_mean)
  double* DX;        // [2d + 1][d] sigma points minus m, or null
  double* part;      // [splits][d] partial sums of the +- pairs
};

// 64 components x 4 groups of sigma pairs per block
__global__ __launch_bounds__(GB) void k_ukf_sigma(SigmaArgs a) {
  __shared__ double sh[GB];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int d = a.d;
  const int j = (int)blockIdx.x * 64 + c;
  const int lo = (int)blockIdx.y * a.chunk, hi = min(d, lo + a.chunk);
  double s = 0.0;
  if (j < d) {
    const double mj = a.m[j];
    const double z0 = image(a.f, mj, j);
    for (int i = lo + g; i < hi; i += 4) {
      const double col = i <= j ? a.gamma * a.W[(size_t)j * d + i] : 0.0;
      const Pair p = image_pair(a.f, z0, col);
      a.E[(size_t)(1 + i) * d + j] = p.ep;
      a.E[(size_t)(1 + d + i) * d + j] = p.em;
      if (a.DX) {
        a.DX[(size_t)(1 + i) * d + j] = col;
        a.DX[(size_t)(1 + d + i) * d + j] = -col;
      }
      s += p.sum;
    }
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  if (g == 0 && j < d) a.part[(size_t)blockIdx.y * d + j] = (sh[c] + sh[64 + c]) + (sh[128 + c] + sh[192 + c]);
}

// zbar = Z_0 + w sum, delta = -w sum into row 0 of E; DX row 0 = 0; resid = z - zbar (z nullable)
__global__ void k_ukf_mean(int d, int S, double w, Fn f, const double* m, const double* part, const double* z,
                           double* zbar, double* E, double* DX, double* resid) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= d) return;
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += part[(size_t)k * d + j];
  const double ws = w * s;
  const double zb = image(f, m[j], j) + ws;
  zbar[j] = zb;
  E[j] = -ws;
  if (DX) DX[j] = 0.0;
  if (z) resid[j] = z[j] - zb;
}

struct ProdArgs {
  int d;
  const double* A;     // [2d + 1][d]
  const double* B;     // [2d + 1][d]
  const double* base;  // [d][d] or null
  double w, w0;        // weights of rows 1 .. 2d and of row 0 (0: row 0 is skipped)
  double* out;         // [d][d]
};

// out[i][j] = base[i][j] + w sum_{k = 1 .. 2d} A[k][i] B[k][j] + w0 A[0][i] B[0][j]
__global__ __launch_bounds__(GB) void k_ukf_prod(ProdArgs a) {
  __shared__ double As[TM * LDT];
  __shared__ double Bs[TN * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int d = a.d, K = 2 * d + 1;
  const int r0 = (int)blockIdx.x * TM, c0 = (int)blockIdx.y * TN;
  d4 acc[2][2];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};

  for (int k0 = 1; k0 < K; k0 += KC) {
    for (int r = 0; r < (TM * KC) / GB; ++r) {  // K is the slow index in memory: rows fastest
      const int e = tid + r * GB;
      const int row = e & (TM - 1), k = e >> 6;
      const int gk = k0 + k, gi = r0 + row, gj = c0 + row;
      double av = 0.0, bv = 0.0;
      if (gk < K) {
        if (gi < d) av = a.A[(size_t)gk * d + gi];
        if (gj < d) bv = a.B[(size_t)gk * d + gj];
      }
      As[row * LDT + k] = av;
      Bs[row * LDT + k] = bv;
    }
    __syncthreads();
    edh_dense::mfma_chunk(As, Bs, wr, wc, lane, acc);
    __syncthreads();
  }
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + edh_dense::tile_row(wr, lane, i, r), col = c0 + edh_dense::tile_col(wc, lane, j);
        if (row < d && col < d) {
          double v = a.w * acc[i][j][r];
          if (a.w0 != 0.0) v += a.w0 * (a.A[row] * a.B[col]);
          if (a.base) v += a.base[(size_t)row * d + col];
          a.out[(size_t)row * d + col] = v;
        }
      }
}

// out = sym(P - X) (ukf.py:189-190)
__global__ void k_ukf_post(int d, const double* P, const double* X, double* out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)d * d) return;
  const int i = (int)(e / d), j = (int)(e % d);
  const size_t t = (size_t)j * d + i;
  out[e] = 0.5 * ((P[e] - X[e]) + (P[t] - X[t]));
}

// the new state replaces the old one unless flags[fa] or flags[fb] (fb < 0: none) is set; past (nullable)
// keeps the mean from before
__global__ void k_ukf_commit(int d, const int* flags, int fa, int fb, const double* mn, const double* Pn, double* m,
                             double* P, double* past) {
  if (flags[fa] != 0 || (fb >= 0 && flags[fb] != 0)) return;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)d * d) return;
  P[e] = Pn[e];
  if (e < d) {
    if (past) past[e] = m[e];
    m[e] = mn[e];
  }
}

// etabar_0 = g(xbar, u, 0) = alpha xbar (+ u) + 0 in NumPy's roundings (no contraction)
__global__ void k_ukf_eta0(int d, double alpha, const double* xbar, const double* u, double* out) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= d) return;
  double y = __dmul_rn(alpha, xbar[j]);
  if (u) y = __dadd_rn(y, u[j]);
  out[j] = __dadd_rn(y, 0.0);
}

}  // namespace ukf_dense
}  // namespace pf
