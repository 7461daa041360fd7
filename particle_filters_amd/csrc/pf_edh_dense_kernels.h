// Dense EDH particle-flow kernels for gfx950 (fp64, wave64): the sensor-network models with a
// large state (d = 64 .. 1024), g(x) = alpha x, an elementwise h and an elementwise likelihood.
//
// The EDH flow linearises h at the tracker-driven mean trajectory only (pf_edh_kernels.h), so the
// whole lambda integration of every particle is one affine map eta_L = M eta_0 + c, composed on the
// host (particle_filters_amd/edh.py).  What is left per particle is dense [N x d] by [d x d] algebra,
// done here on the fp64 matrix cores (v_mfma_f64_16x16x4) by one tiled product kernel
//   C[R x Cn] = A[R x K] B^T[K x Cn],   both operands K-contiguous in LDS,
// with four operand loaders / epilogues (k_dense_gemm<MODE>):
//   G_MAP  A = alpha x + u + v = eta_0 formed in the tile load, B = M;  x_k = C + c stored
//   G_QX   A = x_k - alpha x,   B = W = chol(Q)^-1;  row sums of squares |W (x_k - alpha x)|^2
//   G_QV   A = u + v,           B = W;               row sums of squares |W (eta_0 - alpha x)|^2
//   G_COV  A^T = diag(w) Xc, B^T = Xc (K = the particle index, split over blockIdx.z);  partial
//          covariances, summed in split order by k_cov_combine (two runs are bitwise equal)
// The products of G_QX / G_QV are never stored: a block writes the sum of squares of its 64 columns
// per row, and k_logw adds the column tiles in order.
//
// f64 16x16x4 fragments: A lane l holds A[l & 15][l >> 4], B lane l holds B[l >> 4][l & 15], and the
// 4 results of lane l are D[(l >> 4) + 4 r][l & 15], r = 0..3.  The inner loop over one staged K chunk and
// the map from an accumulator element to its place in the tile are mfma_chunk and tile_row / tile_col, shared with the
// two sibling products whose operands lie differently in memory (k_fm_gemm, k_ukf_prod).
//
// Weights (edh.py:287-297), l_i = log(w_i + 1e-300) - q_x/2 + log p(z | x_k) + q_v/2, then
// max-subtraction, normalisation, ESS and the decision ess < ratio N on the device (k_normalise);
// systematic resampling as searchsorted(cumsum(w / sum w), (U + i) / N, 'right') clamped to N - 1
// (k_cdf, k_gather); weighted mean and covariance (_weighted_stats, symmetrised).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pf {
namespace edh_dense {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int TM = 64, TN = 64;  // output tile of a 256-thread block: 2 x 2 waves of 32 x 32
constexpr int KC = 16;           // K chunk staged through LDS
constexpr int LDT = KC + 1;      // padded LDS row
constexpr int GB = 256;
constexpr int RB = 1024;         // the single-block reductions (normalise, cdf)
constexpr int MB = 256;          // mean partials: 64 columns x 4 row groups

enum { G_MAP = 0, G_QX = 1, G_QV = 2, G_COV = 3 };
enum { OBS_IDENTITY = 0, OBS_EXP = 1 };
enum { LIKE_GAUSSIAN = 0, LIKE_POISSON = 1 };

struct GemmArgs {
  int N, d;
  double alpha;
  const double* X;     // [N][d] x_{k-1}; G_COV: the particles
  const double* Xn;    // [N][d] x_k (G_QX)
  const double* u;     // [d] or null
  const double* v;     // [N][d] or null
  const double* B;     // [d][d] M or W, row-major (row j multiplies the K index)
  const double* c;     // [d] (G_MAP)
  const double* w;     // [N] (G_COV)
  const double* mean;  // [d] (G_COV)
  double* out;         // G_MAP [N][d]; G_QX / G_QV [column tiles][N]; G_COV [splits][d][d]
  int chunk;           // G_COV: particles per split, a multiple of KC
};

// One K chunk of a block's 64 x 64 tile from As [TM][LDT] and Bs [TN][LDT] (both K-contiguous): wave
// (wr, wc) of the block's 2 x 2 owns the 32 x 32 quadrant acc[i][j] of 16 x 16 fragments.
__device__ __forceinline__ void mfma_chunk(const double* As, const double* Bs, int wr, int wc, int lane,
                                           d4 (&acc)[2][2]) {
#pragma unroll
  for (int kk = 0; kk < KC; kk += 4) {
    double fa[2], fb[2];
    for (int i = 0; i < 2; ++i) fa[i] = As[(wr * 32 + i * 16 + (lane & 15)) * LDT + kk + (lane >> 4)];
    for (int j = 0; j < 2; ++j) fb[j] = Bs[(wc * 32 + j * 16 + (lane & 15)) * LDT + kk + (lane >> 4)];
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
  }
}

// where acc[i][j][r] of a lane of wave (wr, wc) lies in the block's tile
__device__ __forceinline__ int tile_row(int wr, int lane, int i, int r) { return wr * 32 + i * 16 + (lane >> 4) + 4 * r; }
__device__ __forceinline__ int tile_col(int wc, int lane, int j) { return wc * 32 + j * 16 + (lane & 15); }

template <int MODE>
__global__ __launch_bounds__(GB) void k_dense_gemm(GemmArgs a) {
  __shared__ double As[TM * LDT];
  __shared__ double Bs[TN * LDT];
  __shared__ double rs[TM * 2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int N = a.N, d = a.d;
  const int R = MODE == G_COV ? d : N;  // output rows; the columns are d in every mode
  int k_lo = 0, k_hi = d;
  if (MODE == G_COV) {
    k_lo = (int)blockIdx.z * a.chunk;
    k_hi = min(N, k_lo + a.chunk);
  }
  const int r0 = (int)blockIdx.x * TM, c0 = (int)blockIdx.y * TN;
  d4 acc[2][2];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};

  for (int k0 = k_lo; k0 < k_hi; k0 += KC) {
    for (int r = 0; r < (TM * KC) / GB; ++r) {
      const int e = tid + r * GB;
      double av = 0.0, bv = 0.0;
      if (MODE == G_COV) {  // K (the particle) is the slow index in memory: rows fastest
        const int row = e & (TM - 1), k = e >> 6;
        const int gp = k0 + k, gi = r0 + row, gj = c0 + row;
        if (gp < k_hi) {
          const double* xp = a.X + (size_t)gp * d;
          if (gi < d) av = a.w[gp] * (xp[gi] - a.mean[gi]);
          if (gj < d) bv = xp[gj] - a.mean[gj];
        }
        As[row * LDT + k] = av;
        Bs[row * LDT + k] = bv;
      } else {
        const int k = e & (KC - 1), row = e >> 4;
        const int gk = k0 + k, gi = r0 + row, gj = c0 + row;
        if (gk < d) {
          if (gi < N) {
            const size_t o = (size_t)gi * d + gk;
            if (MODE == G_MAP) {
              av = a.alpha * a.X[o];
              if (a.u) av += a.u[gk];
              if (a.v) av += a.v[o];
            } else if (MODE == G_QX) {
              av = a.Xn[o] - a.alpha * a.X[o];
            } else {
              if (a.u) av += a.u[gk];
              if (a.v) av += a.v[o];
            }
          }
          if (gj < d) bv = a.B[(size_t)gj * d + gk];
        }
        As[row * LDT + k] = av;
        Bs[row * LDT + k] = bv;
      }
    }
    __syncthreads();
    mfma_chunk(As, Bs, wr, wc, lane, acc);
    __syncthreads();
  }

  if (MODE == G_QX || MODE == G_QV) {
    for (int i = 0; i < 2; ++i)
      for (int r = 0; r < 4; ++r) {
        double s = acc[i][0][r] * acc[i][0][r] + acc[i][1][r] * acc[i][1][r];
        for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
        if ((lane & 15) == 0) rs[tile_row(wr, lane, i, r) * 2 + wc] = s;
      }
    __syncthreads();
    if (tid < TM && r0 + tid < N) a.out[(size_t)blockIdx.y * N + r0 + tid] = rs[tid * 2] + rs[tid * 2 + 1];
    return;
  }
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + tile_row(wr, lane, i, r), col = c0 + tile_col(wc, lane, j);
        if (row < R && col < d) {
          if (MODE == G_MAP)
            a.out[(size_t)row * d + col] = acc[i][j][r] + a.c[col];
          else
            a.out[((size_t)blockIdx.z * d + row) * d + col] = acc[i][j][r];
        }
      }
}

// cov = sum over the splits in order / sum(w), then 0.5 (C + C^T) (edh.py:323-327)
__global__ void k_cov_combine(const double* part, int S, int d, const double* wsum, double* cov) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)d * d) return;
  const int r = (int)(e / d), c = (int)(e % d);
  double s1 = 0.0, s2 = 0.0;
  for (int s = 0; s < S; ++s) {
    s1 += part[((size_t)s * d + r) * d + c];
    s2 += part[((size_t)s * d + c) * d + r];
  }
  cov[e] = 0.5 * (s1 / wsum[0] + s2 / wsum[0]);
}

struct LogwArgs {
  int N, d, ctiles, obs, like;
  double m1, m2;
  const double* Xn;    // [N][d] x_k
  const double* z;     // [d]
  const double* rdiag; // [d] diagonal of R (LIKE_GAUSSIAN)
  const double* qx;    // [ctiles][N]
  const double* qv;    // [ctiles][N] or null (no noise and no control: eta_0 = g(x))
  const double* w;     // [N] previous weights
  const double* theta; // [N] log-determinant term of the dense LEDH flow, or null (EDH)
  double* logw;        // [N]
};

// one wave per particle: the elementwise log-likelihood as a row reduction, then the log-weight
__global__ __launch_bounds__(GB) void k_logw(LogwArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (GB / 64) + (threadIdx.x >> 6);
  if (i >= a.N) return;
  const double* x = a.Xn + (size_t)i * a.d;
  double s = 0.0;
  for (int j = lane; j < a.d; j += 64) {
    const double hx = a.obs == OBS_EXP ? a.m1 * exp(a.m2 * x[j]) : x[j];
    if (a.like == LIKE_POISSON) {
      const double lam = fmin(fmax(hx, 1e-10), 1e10);  // np.clip(lam, 1e-10, 1e10)
      s += a.z[j] * log(lam) - lam;                    // the log(max(1, j)) term is common to all particles
    } else {
      const double r = a.z[j] - hx;
      s -= 0.5 * r * r / a.rdiag[j];
    }
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) {
    double qx = 0.0, qv = 0.0;
    for (int t = 0; t < a.ctiles; ++t) qx += a.qx[(size_t)t * a.N + i];
    if (a.qv)
      for (int t = 0; t < a.ctiles; ++t) qv += a.qv[(size_t)t * a.N + i];
    double l = log(a.w[i] + 1e-300);
    if (a.theta) l += a.theta[i];  // ledh.py:186
    a.logw[i] = l + (-0.5 * qx + s + 0.5 * qv);
  }
}

// fixed-order block reductions over RB threads
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int o = RB / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  return sh[0];
}
__device__ __forceinline__ double block_max(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int o = RB / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] = fmax(sh[t], sh[t + o]);
    __syncthreads();
  }
  return sh[0];
}

// info[0] = ESS, info[1] = resample decision (0 / 1), info[2] = 1 when no weight is alive
__global__ __launch_bounds__(RB) void k_normalise(const double* logw, double* w, int N, double ratio, double* info) {
  __shared__ double sh[RB];
  const int t = threadIdx.x;
  double m = -INFINITY;
  bool bad = false;
  for (int i = t; i < N; i += RB) {
    const double l = logw[i];
    if (l != l) bad = true;
    m = fmax(m, l);
  }
  m = block_max(m, sh);
  const double nbad = block_sum(bad ? 1.0 : 0.0, sh);
  double s = 0.0;
  for (int i = t; i < N; i += RB) {
    const double e = exp(logw[i] - m);
    w[i] = e;
    s += e;
  }
  s = block_sum(s, sh);
  const bool dead = nbad > 0.0 || !(m > -INFINITY) || !(m < INFINITY) || !(s > 0.0) || !(s < INFINITY);
  double s1 = 0.0;
  for (int i = t; i < N; i += RB) {
    const double wi = w[i] / s;
    w[i] = wi;
    s1 += wi;
  }
  s1 = block_sum(s1, sh);  // effective_sample_size renormalises (edh.py:54-55)
  double s2 = 0.0;
  for (int i = t; i < N; i += RB) {
    const double wi = w[i] / s1;
    s2 += wi * wi;
  }
  s2 = block_sum(s2, sh);
  if (t == 0) {
    const double ess = 1.0 / s2;
    info[0] = ess;
    info[1] = (!dead && ratio > 0.0 && ess < ratio * (double)N) ? 1.0 : 0.0;
    info[2] = dead ? 1.0 : 0.0;
  }
}

// inclusive fp64 CDF of w / sum(w) (edh.py:40-42); skipped when the step does not resample
__global__ __launch_bounds__(RB) void k_cdf(const double* w, int N, const double* info, double* cdf) {
  __shared__ double sh[RB];
  __shared__ double offs[RB];
  if (info[1] == 0.0) return;
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < N; i += RB) s += w[i];
  s = block_sum(s, sh);
  const int per = (N + RB - 1) / RB;
  const int lo = min(N, t * per), hi = min(N, lo + per);
  double c = 0.0;
  for (int i = lo; i < hi; ++i) c += w[i] / s;
  __syncthreads();
  offs[t] = c;
  __syncthreads();
  if (t == 0) {
    double run = 0.0;
    for (int k = 0; k < RB; ++k) {
      const double v = offs[k];
      offs[k] = run;
      run += v;
    }
  }
  __syncthreads();
  c = offs[t];
  for (int i = lo; i < hi; ++i) {
    c += w[i] / s;
    cdf[i] = c;
  }
}

// ancestor of slot i: searchsorted(cdf, (U + i) / N, 'right') clamped to N - 1, or i itself when
// the step does not resample; one wave copies one d-wide row
__global__ __launch_bounds__(GB) void k_gather(const double* Xn, const double* wn, const double* cdf, const double* U,
                                               const double* info, int N, int d, double* X, double* w) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (GB / 64) + (threadIdx.x >> 6);
  if (i >= N) return;
  int src = (int)i;
  const bool res = info[1] != 0.0;
  if (res) {
    const double pos = (U[0] + (double)i) / (double)N;
    int lo = 0, hi = N;  // first index with cdf > pos
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] > pos) hi = mid; else lo = mid + 1;
    }
    src = min(lo, N - 1);
  }
  const double* xs = Xn + (size_t)src * d;
  double* xd = X + (size_t)i * d;
  for (int j = lane; j < d; j += 64) xd[j] = xs[j];
  if (lane == 0) w[i] = res ? 1.0 / (double)N : wn[i];
}

// weighted mean (edh.py:323-324): partial sums over a chunk of particles, 64 columns per block
__global__ __launch_bounds__(MB) void k_mean_part(const double* X, const double* w, int N, int d, int chunk,
                                                  double* part, double* wpart) {
  __shared__ double sh[MB];
  __shared__ double shw[MB];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int j = (int)blockIdx.x * 64 + c;
  const int lo = (int)blockIdx.y * chunk, hi = min(N, lo + chunk);
  double s = 0.0, sw = 0.0;
  for (int i = lo + g; i < hi; i += 4) {
    const double wi = w[i];
    sw += wi;
    if (j < d) s += wi * X[(size_t)i * d + j];
  }
  sh[threadIdx.x] = s;
  shw[threadIdx.x] = sw;
  __syncthreads();
  if (g == 0) {
    if (j < d) part[(size_t)blockIdx.y * d + j] = (sh[c] + sh[64 + c]) + (sh[128 + c] + sh[192 + c]);
    if (blockIdx.x == 0 && c == 0) wpart[blockIdx.y] = (shw[0] + shw[64]) + (shw[128] + shw[192]);
  }
}

// mean = sum of the partials in order / sum(w); wsum[0] = sum(w) for the covariance's weights
__global__ void k_mean_combine(const double* part, const double* wpart, int S, int d, double* mean, double* wsum) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  double sw = 0.0;
  for (int s = 0; s < S; ++s) sw += wpart[s];
  if (j == 0) wsum[0] = sw;
  if (j >= d) return;
  double m = 0.0;
  for (int s = 0; s < S; ++s) m += part[(size_t)s * d + j];
  mean[j] = m / sw;
}

}  // namespace edh_dense
}  // namespace pf
