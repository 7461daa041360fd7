// Device side of the kernel particle flow filter (include/pf_kpf.h; host side pf_kpf.hip).
//
// One pseudo-time step of KernelParticleFilter.analyze (models/kernel_particle_filter.py, "kpf.py")
// over the SoA ensemble x [nx][Npad] (fp64):
//   scores   G_i = JH(x_i)^T R^-1 (y - H(x_i)) - B_inv (x_i - x0)                 kpf.py:304-317
//            k_kpf_resid (r = y - H(x)), k_kpf_rinv (z = R^-1 r), k_kpf_score (J^T z - B_inv (x - x0))
//   pairs    k_kpf_pairs_diag / k_kpf_pairs_scalar: the all-pairs RBF sums, split over the source
//            particles m into S partial sums per output                           kpf.py:408-424
//   update   k_kpf_combine (u = sum_s partial / N, s = 0..S-1 in that order), k_kpf_matvec twice
//            (v = B u, w = B_inv (ds v)), k_kpf_move (Mahalanobis clip, x_new)     kpf.py:426-434
// The per-particle kernels run lanes over particles and blockIdx.y over the output component, so
// that an O(nx^2) product per particle is nx short dot products in flight at once, not one lane's
// serial chain: at Np = 200 the one-lane-per-particle form of the scores and the update took
// 0.6 ms of a 0.68 ms step.  Every velocity is formed from the old ensemble (the reference reads
// X and writes X_new), so the evaluation order of the particles does not enter the result.  No
// floating-point atomics: two runs on the same input are bitwise equal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pf_kpf.h"

namespace pf {
namespace kpf {

constexpr int PB = 256;    // lanes per workgroup of the one-dimensional kernels (load, store, move, gsum)
constexpr int CB = 64;     // lanes per workgroup of the (particle, component) kernels
constexpr int MGRAIN = 32; // granularity of a split of the m range
constexpr int MAXS = 16;   // most partial sums per output

struct Params {
  int N, Npad, nx, nz, ok;
  const double* op;    // observation parameters (PF_OBS_* layout of pf_engine.h)
  const double* Rinv;  // [nz][nz]
  const double* y;     // [nz]
  const double* x0;    // [nx]
  const double* B;     // [nx][nx]
  const double* Binv;  // [nx][nx]
  const double* ell;   // [nx]
};

// X [N][nx] (host layout) -> x [nx][Npad]
__global__ void __launch_bounds__(PB) k_kpf_load(const double* __restrict__ X, double* __restrict__ x, int N, int Npad,
                                                 int nx) {
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= (int64_t)N * nx) return;
  const int i = (int)(q / nx), j = (int)(q - (int64_t)i * nx);
  x[(size_t)j * Npad + i] = X[q];
}

// x [nx][Npad] -> X [N][nx]
__global__ void __launch_bounds__(PB) k_kpf_store(const double* __restrict__ x, double* __restrict__ X, int N, int Npad,
                                                  int nx) {
  const int64_t q = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (q >= (int64_t)N * nx) return;
  const int i = (int)(q / nx), j = (int)(q - (int64_t)i * nx);
  X[q] = x[(size_t)j * Npad + i];
}

// r_k = y_k - H(x_i)_k, lane (i, k = blockIdx.y); rw [nz][Npad].  The observation formulas are
// those of obs_jac_block (pf_ledh_kernels.h), at runtime nx / nz.
__global__ void __launch_bounds__(CB) k_kpf_resid(Params p, const double* __restrict__ x, double* __restrict__ rw) {
  const int i = blockIdx.x * CB + threadIdx.x, k = blockIdx.y;
  if (i >= p.N) return;
  const int nx = p.nx, nz = p.nz;
  const size_t P = (size_t)p.Npad;
  double hx;
  if (p.ok == PF_OBS_LINEAR) {  // h = H x + c: params H [nz][nx], c [nz]
    double acc = 0.0;
    for (int e = 0; e < nx; ++e) acc += p.op[(size_t)k * nx + e] * x[e * P + i];
    hx = acc + p.op[(size_t)nz * nx + k];
  } else if (p.ok == PF_OBS_EXP_HALF) {  // h_k = beta_k exp(x_k / 2): params beta [nz], nz == nx
    hx = p.op[k] * exp(0.5 * x[k * P + i]);
  } else {  // ACOUSTIC: h_s = sum_c psi / (|p_c - s|^2 + d0): params psi, d0, sx [nz], sy [nz]
    const double psi = p.op[0], d0 = p.op[1];
    const double sx = p.op[2 + k], sy = p.op[2 + nz + k];
    double acc = 0.0;
    for (int c = 0; c < nx / 4; ++c) {
      const double dx = x[(4 * c) * P + i] - sx, dy = x[(4 * c + 1) * P + i] - sy;
      acc += psi / ((dx * dx + dy * dy) + d0);
    }
    hx = acc;
  }
  rw[k * P + i] = p.y[k] - hx;
}

// z = R^-1 r, lane (i, k = blockIdx.y); zw [nz][Npad]
__global__ void __launch_bounds__(CB) k_kpf_rinv(Params p, const double* __restrict__ rw, double* __restrict__ zw) {
  const int i = blockIdx.x * CB + threadIdx.x, k = blockIdx.y;
  if (i >= p.N) return;
  const size_t P = (size_t)p.Npad;
  double acc = 0.0;
  for (int l = 0; l < p.nz; ++l) acc += p.Rinv[(size_t)k * p.nz + l] * rw[l * P + i];
  zw[k * P + i] = acc;
}

// G_ij = (JH(x_i)^T z_i)_j - (B_inv (x_i - x0))_j, lane (i, j = blockIdx.y) (kpf.py:316); J^T z is
// formed from the observation's formulas without a Jacobian in memory.
__global__ void __launch_bounds__(CB) k_kpf_score(Params p, const double* __restrict__ x, const double* __restrict__ zw,
                                                  double* __restrict__ G) {
  const int i = blockIdx.x * CB + threadIdx.x, j = blockIdx.y;
  if (i >= p.N) return;
  const int nx = p.nx, nz = p.nz;
  const size_t P = (size_t)p.Npad;
  double jz = 0.0;
  if (p.ok == PF_OBS_LINEAR) {
    for (int k = 0; k < nz; ++k) jz += p.op[(size_t)k * nx + j] * zw[k * P + i];
  } else if (p.ok == PF_OBS_EXP_HALF) {
    jz = (0.5 * p.op[j] * exp(0.5 * x[j * P + i])) * zw[j * P + i];
  } else if ((j & 2) == 0) {  // the acoustic h reads the positions only (columns 4c, 4c + 1)
    const double psi = p.op[0], d0 = p.op[1];
    const int c = j >> 2;
    const double px = x[(4 * c) * P + i], py = x[(4 * c + 1) * P + i];
    for (int k = 0; k < nz; ++k) {
      const double dx = px - p.op[2 + k], dy = py - p.op[2 + nz + k];
      const double den = (dx * dx + dy * dy) + d0;
      jz += ((-2.0 * psi * ((j & 1) ? dy : dx)) / (den * den)) * zw[k * P + i];
    }
  }
  double pr = 0.0;
  for (int e = 0; e < nx; ++e) pr += p.Binv[(size_t)j * nx + e] * (x[e * P + i] - p.x0[e]);
  G[j * P + i] = jz - pr;
}

// gsum_i = sum_j G_ij, what the scalar kernel's first term reads (kpf.py:417); lanes over particles
__global__ void __launch_bounds__(PB) k_kpf_gsum(const double* __restrict__ G, double* __restrict__ gsum, int N,
                                                 int Npad, int nx) {
  const int i = blockIdx.x * PB + threadIdx.x;
  if (i >= N) return;
  double gs = 0.0;
  for (int j = 0; j < nx; ++j) gs += G[(size_t)j * Npad + i];
  gsum[i] = gs;
}

// Diagonal kernel (kpf.py:421-424), the hot path: lane (i, j) sums, over the source particles m of
// split blockIdx.z, exp(-d^2 / (2 l_j^2)) (G_mj - d / l_j^2) with d = x_ij - x_mj taken directly.
// (x_mj, G_mj) stream through LDS in tiles of blockDim.x pairs; every lane reads the same pair, so
// the reads broadcast.  A tile's tail and the lanes past N are predicated: no padding particle
// contributes.  part [S][nx][Npad].  Dynamic LDS: blockDim.x * 16 bytes.
__global__ void __launch_bounds__(256) k_kpf_pairs_diag(const double* __restrict__ x, const double* __restrict__ G,
                                                        const double* __restrict__ ell, double* __restrict__ part,
                                                        int N, int Npad, int nx, int chunk) {
  extern __shared__ double2 kpf_tile[];
  const int t = threadIdx.x, bs = blockDim.x;
  const int j = blockIdx.y, s = blockIdx.z;
  const int i = blockIdx.x * bs + t;
  const double* __restrict__ xj = x + (size_t)j * Npad;
  const double* __restrict__ Gj = G + (size_t)j * Npad;
  const double inv = 1.0 / ell[j], inv2 = inv * inv;
  const double xi = (i < N) ? xj[i] : 0.0;
  const int m0 = s * chunk, m1 = min(N, m0 + chunk);
  double acc = 0.0;
  for (int base = m0; base < m1; base += bs) {
    const int m = base + t;
    if (m < m1) kpf_tile[t] = make_double2(xj[m], Gj[m]);
    __syncthreads();
    const int cnt = min(bs, m1 - base);
#pragma unroll 4
    for (int q = 0; q < cnt; ++q) {
      const double2 sm = kpf_tile[q];
      const double d = xi - sm.x;
      const double u = d * inv;
      const double k = exp(-0.5 * (u * u));
      acc = fma(k, sm.y - d * inv2, acc);
    }
    __syncthreads();
  }
  if (i < N) part[((size_t)s * nx + j) * Npad + i] = acc;
}

// Scalar kernel (kpf.py:408-419, 141-158): lane i sums, over the source particles m of split
// blockIdx.y, k_im (sum_j G_mj - (1 / l^2) sum_j (x_ij - x_mj)) with k_im = exp(-|x_i - x_m|^2 /
// (2 l^2)): the reference's arithmetic, its "sum of all gradient components" divergence included.
// Tiles of TM source particles ([nx][TM] and their gsum) stream through LDS; four of them share
// each read of x_ij.  part [S][Npad].  Dynamic LDS: (nx + 1) * TM * 8 bytes, TM a multiple of 4.
__global__ void __launch_bounds__(64) k_kpf_pairs_scalar(const double* __restrict__ x, const double* __restrict__ gsum,
                                                         const double* __restrict__ ell, double* __restrict__ part,
                                                         int N, int Npad, int nx, int chunk, int TM) {
  extern __shared__ double kpf_sm[];
  double* __restrict__ xm = kpf_sm;                    // [nx][TM]
  double* __restrict__ gm = kpf_sm + (size_t)nx * TM;  // [TM]
  const int t = threadIdx.x, bs = blockDim.x;
  const int s = blockIdx.y;
  const int i = blockIdx.x * bs + t;
  const int ic = min(i, N - 1);  // lanes past N read particle N - 1 and store nothing
  const double l = ell[0];
  const double inv2 = 1.0 / (l * l);
  const int m0 = s * chunk, m1 = min(N, m0 + chunk);
  double acc = 0.0;
  for (int base = m0; base < m1; base += TM) {
    const int cnt = min(TM, m1 - base);
    for (int idx = t; idx < nx * TM; idx += bs) {
      const int j = idx / TM, q = idx - j * TM;
      xm[idx] = (q < cnt) ? x[(size_t)j * Npad + base + q] : 0.0;
    }
    for (int q = t; q < TM; q += bs) gm[q] = (q < cnt) ? gsum[base + q] : 0.0;
    __syncthreads();
    for (int q0 = 0; q0 < cnt; q0 += 4) {
      double r2[4] = {0.0, 0.0, 0.0, 0.0}, dsum[4] = {0.0, 0.0, 0.0, 0.0};
      for (int j = 0; j < nx; ++j) {
        const double xi = x[(size_t)j * Npad + ic];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const double d = xi - xm[j * TM + q0 + a];
          r2[a] = fma(d, d, r2[a]);
          dsum[a] += d;
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
        if (q0 + a < cnt) {  // a tile's tail holds no particle
          const double k = exp((-0.5 * r2[a]) * inv2);
          acc = fma(k, gm[q0 + a] - inv2 * dsum[a], acc);
        }
    }
    __syncthreads();
  }
  if (i < N) part[(size_t)s * Npad + i] = acc;
}

// u_ij = (sum_s part[s]) / N in the order s = 0..S-1, lane (i, j = blockIdx.y); the scalar kernel's
// one value per particle is broadcast to every component (kpf.py:418-419).  U [nx][Npad].
__global__ void __launch_bounds__(CB) k_kpf_combine(const double* __restrict__ part, int S, int scalar,
                                                    double* __restrict__ U, int N, int Npad, int nx) {
  const int i = blockIdx.x * CB + threadIdx.x, j = blockIdx.y;
  if (i >= N) return;
  const size_t P = (size_t)Npad;
  double u = 0.0;
  for (int s = 0; s < S; ++s) u += scalar ? part[s * P + i] : part[((size_t)s * nx + j) * P + i];
  U[j * P + i] = u / (double)N;
}

// out_e = sum_j A[e][j] (scale in_j), lane (i, e = blockIdx.y): v = B u with scale 1 (kpf.py:426),
// w = B_inv (ds v) with scale ds[step] (kpf.py:428, 321)
__global__ void __launch_bounds__(CB) k_kpf_matvec(const double* __restrict__ A, const double* __restrict__ in,
                                                   double* __restrict__ out, const double* __restrict__ ds_all,
                                                   int step, int N, int Npad, int nx) {
  const int i = blockIdx.x * CB + threadIdx.x, e = blockIdx.y;
  if (i >= N) return;
  const size_t P = (size_t)Npad;
  const double sc = ds_all ? ds_all[step] : 1.0;
  double acc = 0.0;
  for (int j = 0; j < nx; ++j) acc += A[(size_t)e * nx + j] * (sc * in[j * P + i]);
  out[e * P + i] = acc;
}

// The clipped update, lanes over particles (kpf.py:428-434): move = sqrt((ds v)^T w), the step
// scaled to c_move_max where it is larger, x_new into the other buffer; n_clip[step] counts the
// scaled particles (one integer atomic per wave).
__global__ void __launch_bounds__(PB) k_kpf_move(const double* __restrict__ x, double* __restrict__ xn,
                                                 const double* __restrict__ V, const double* __restrict__ W,
                                                 const double* __restrict__ ds_all, int step, double cmax,
                                                 int32_t* __restrict__ n_clip, int N, int Npad, int nx) {
  const int i = blockIdx.x * PB + threadIdx.x;
  const size_t P = (size_t)Npad;
  bool clipped = false;
  if (i < N) {
    const double ds = ds_all[step];
    double q = 0.0;
    for (int e = 0; e < nx; ++e) q += (ds * V[e * P + i]) * W[e * P + i];
    const double move = sqrt(q);
    clipped = move > cmax;  // false for a NaN move, as in the reference
    const double step_len = clipped ? ds * (cmax / fmax(move, 1e-12)) : ds;
    for (int e = 0; e < nx; ++e) xn[e * P + i] = x[e * P + i] + step_len * V[e * P + i];
  }
  const unsigned long long b = __ballot(clipped);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&n_clip[step], (int32_t)__popcll(b));
}

}  // namespace kpf
}  // namespace pf
