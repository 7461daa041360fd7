// Device composition of the dense EDH flow map for gfx950 (fp64, wave64): the lambda loop of the
// reference's EDHFlowPF.step (models/EDH_particle_filter.py:216-280, cited "edh.py:LINE") for the
// sensor-network models as one affine map eta_L = M eta_0 + c, built without the host.
//
// h is elementwise, so H = diag(D) (D = 1, or m1 m2 exp(m2 etabar)), and the flow's R = diag(r).
// Per lambda step, at the mean trajectory etabar (edh.py:230-264):
//   e   = h(etabar) - D o etabar
//   S   = lam (D D^T o P) + diag(r)                  SPD; factored S = L L^T, never stored unfactored
//   S^-1                                             d unit right-hand sides, three per workgroup (k_chol_solve)
//   A   = -1/2 (P diag(D)) (S^-1 diag(D))            S^-1 is symmetric: its columns are stored as rows
//   y   = P (D o (z - e) / r)
//   b   = (I + 2 lam A)((I + lam A) y + A etabar)
//   Euler: Phi = I + E, psi = dlam b;  RK4: G = I + E/2 (I + E/3 (I + E/4)), Phi = I + E G,
//   psi = dlam G b, with E = dlam A (edh.compose_flow_map)
//   etabar <- Phi etabar + psi,  M <- Phi M,  c <- Phi c + psi
//
// The d x d products run on v_mfma_f64_16x16x4 in k_fm_gemm, a sibling of k_dense_gemm with the same
// tiles and the same inner loop and fragment map (edh_dense::mfma_chunk, tile_row / tile_col):
//   out = alpha X' Y' + beta I,  X' = X diag(xD),  Y' = (ys Y + yI I) diag(yD),
// so "I + ..." and the diagonal scalings need no pass of their own.  The Cholesky factorisation and the
// triangular solves are those of the dense LEDH flow (ledh_dense::chol_factor / k_chol_solve): the factor
// by one workgroup, the d independent right-hand sides spread over workgroups.  The vector work is a
// one-wave-per-row product with an affine epilogue (k_fm_matvec).  Every sum has a fixed order, so two
// runs are bitwise equal.  A pivot that is not finite and positive sets the step's flag; no index depends
// on a value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pf_edh_dense_kernels.h"
#include "pf_ledh_dense_kernels.h"

namespace pf {
namespace edh_flowmap {

using edh_dense::d4;
using edh_dense::GB;
using edh_dense::KC;
using edh_dense::LDT;
using edh_dense::TM;
using edh_dense::TN;
using ledh_dense::LB;
using ledh_dense::NB;

constexpr int NVEC = 9;  // d-vectors of the composition: eta eta' D t y t1 b psi c'

struct MatArgs {
  int d;
  const double* X;   // [d][d]
  const double* xD;  // [d] scales the columns of X, or null
  const double* Y;   // [d][d]
  const double* yD;  // [d] scales the columns of ys Y + yI I, or null
  double ys, yI;
  double alpha, beta;
  double* out;       // [d][d], neither X nor Y
};

__global__ __launch_bounds__(GB) void k_fm_gemm(MatArgs a) {
  __shared__ double As[TM * LDT];
  __shared__ double Bs[TN * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int d = a.d;
  const int r0 = (int)blockIdx.x * TM, c0 = (int)blockIdx.y * TN;
  d4 acc[2][2];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};

  for (int k0 = 0; k0 < d; k0 += KC) {
    for (int r = 0; r < (TM * KC) / GB; ++r) {
      const int e = tid + r * GB;
      {  // X: K is the fast index in memory
        const int k = e & (KC - 1), row = e >> 4;
        const int gk = k0 + k, gi = r0 + row;
        double av = 0.0;
        if (gk < d && gi < d) {
          av = a.X[(size_t)gi * d + gk];
          if (a.xD) av *= a.xD[gk];
        }
        As[row * LDT + k] = av;
      }
      {  // Y: K is the slow index in memory, the columns fastest
        const int col = e & (TN - 1), k = e >> 6;
        const int gk = k0 + k, gj = c0 + col;
        double bv = 0.0;
        if (gk < d && gj < d) {
          bv = a.ys * a.Y[(size_t)gk * d + gj];
          if (gk == gj) bv += a.yI;
          if (a.yD) bv *= a.yD[gj];
        }
        Bs[col * LDT + k] = bv;
      }
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
          double v = a.alpha * acc[i][j][r];
          if (row == col) v += a.beta;
          a.out[(size_t)row * d + col] = v;
        }
      }
}

// out = s X + I (Euler's Phi)
__global__ void k_fm_axpi(int d, double s, const double* X, double* out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)d * d) return;
  double v = s * X[e];
  if (e / d == e % d) v += 1.0;
  out[e] = v;
}

// M = I, c = 0, eta = etabar_0
__global__ void k_fm_init(int d, const double* eta0, double* M, double* c, double* eta) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)d * d) return;
  M[e] = e / d == e % d ? 1.0 : 0.0;
  if (e < d) {
    c[e] = 0.0;
    eta[e] = eta0[e];
  }
}

// the linearisation at etabar: D, and t = D o (z - e) / r; trace (nullable) keeps etabar
__global__ void k_fm_pre(int d, int obs, double m1, double m2, const double* eta, const double* z, const double* rdiag,
                         double* D, double* t, double* trace) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= d) return;
  const double x = eta[j];
  if (trace) trace[j] = x;
  double hx = x, Dj = 1.0;
  if (obs == edh_dense::OBS_EXP) {
    hx = m1 * exp(m2 * x);
    Dj = m2 * hx;
  }
  const double e = hx - Dj * x;
  D[j] = Dj;
  t[j] = Dj * ((z[j] - e) / rdiag[j]);
}

// lower Cholesky factor of coef (D D^T o P) + diag(r) into W; *fail = 1 on a failed pivot
__global__ __launch_bounds__(LB) void k_fm_chol(int d, double coef, const double* P, const double* D,
                                                const double* rdiag, double* W, int* fail) {
  __shared__ double tile[NB * (NB + 1)];
  __shared__ double sc[4];
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  ledh_dense::chol_factor(ledh_dense::SpdArgs{d, P, rdiag}, D, coef, W, tile, sc, &bad);  // ends with a barrier
  if (threadIdx.x == 0 && bad) *fail = 1;
}

struct VecArgs {
  int d;
  const double* A;    // [d][d], or null (out = ca add)
  const double* in0;  // [d]
  const double* in1;  // [d] or null
  const double* add;  // [d] or null
  double ca, s0, s1;
  double* out;        // [d], none of the inputs
};

// out = ca add + s0 A in0 + s1 A in1, one wave per row: lane-strided partial sums, then a fixed tree
__global__ __launch_bounds__(GB) void k_fm_matvec(VecArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = (int)blockIdx.x * (GB / 64) + (threadIdx.x >> 6);
  if (row >= a.d) return;
  double t0 = 0.0, t1 = 0.0;
  if (a.A) {
    const double* r = a.A + (size_t)row * a.d;
    for (int j = lane; j < a.d; j += 64) {
      const double x = r[j];
      t0 += x * a.in0[j];
      if (a.in1) t1 += x * a.in1[j];
    }
    for (int off = 32; off > 0; off >>= 1) {
      t0 += __shfl_down(t0, off, 64);
      t1 += __shfl_down(t1, off, 64);
    }
  }
  if (lane == 0) {
    double v = a.s0 * t0;
    if (a.in1) v += a.s1 * t1;
    if (a.add) v = a.ca * a.add[row] + v;
    a.out[row] = v;
  }
}

}  // namespace edh_flowmap
}  // namespace pf
