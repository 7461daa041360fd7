// Device process noise of the dense sensor-network flows (fp64, wave64, gfx950): V = zeta chol(Q)^T with
// the standard normals zeta generated in the operand load from the project's Philox counters, so the
// [N x d] normals are never in memory.
//
// k_dense_noise is a fifth product of the family of pf_edh_dense_kernels.h (64 x 64 output tiles,
// v_mfma_f64_16x16x4, K staged in chunks of KC through LDS; mfma_chunk / tile_row / tile_col are that
// header's):
//   V[i][j] = (mean[j] +) sum_{k <= j} zeta[i][k] L[j][k]
//   A  zeta[i][k] = element f & 3 of normal4<double>(seed, f >> 2, 0, epoch, stream), f = i d + k: the fp64
//      Box-Muller of philox.h in flat (particle, dim) order, which oracle/philox.normals restates.  f does
//      not depend on N or on the grid, so row i of V is the same whatever N is.  Where d % 4 == 0 a group
//      of four counters lies in one row and one call feeds four consecutive k (64 rows x 4 groups = one
//      call per thread per chunk); otherwise groups straddle rows and every element picks its own.
//   B  L row-major, lower triangular: column tile c0 stops its K loop at min(d, c0 + TN), and inside the
//      diagonal tile an element above the diagonal is a zero that is never read.
// K ascends in fixed chunks, so every V[i][j] is bitwise reproducible and independent of N and the grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pf_edh_dense_kernels.h"
#include "philox.h"

namespace pf {
namespace edh_dense {

struct NoiseArgs {
  int N, d;
  uint64_t seed;
  uint32_t epoch, stream;  // the Philox counter's epoch and stream (STREAM_PROCESS, STREAM_INIT)
  const double* L;         // [d][d] lower Cholesky factor, row-major
  const double* mean;      // [d] or null
  double* out;             // [N][d]
};

__global__ __launch_bounds__(GB) void k_dense_noise(NoiseArgs a) {
  __shared__ double As[TM * LDT];
  __shared__ double Bs[TN * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int N = a.N, d = a.d;
  const int r0 = (int)blockIdx.x * TM, c0 = (int)blockIdx.y * TN;
  const int k_hi = min(d, c0 + TN);  // L[j][k] = 0 for k > j
  const bool grouped = (d & 3) == 0;
  d4 acc[2][2];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};

  for (int k0 = 0; k0 < k_hi; k0 += KC) {
    if (grouped) {  // N d <= 2^30: f fits 32 bits
      const int row = tid >> 2, k = (tid & 3) * 4;
      const int gi = r0 + row, gk = k0 + k;
      Normal4<double> q{{0.0, 0.0, 0.0, 0.0}};
      if (gi < N && gk < d) q = normal4<double>(a.seed, (uint32_t)(((int64_t)gi * d + gk) >> 2), 0, a.epoch, a.stream);
      for (int c = 0; c < 4; ++c) As[row * LDT + k + c] = q.v[c];
    } else {
      for (int r = 0; r < (TM * KC) / GB; ++r) {
        const int e = tid + r * GB;
        const int k = e & (KC - 1), row = e >> 4;
        const int gi = r0 + row, gk = k0 + k;
        double av = 0.0;
        if (gi < N && gk < d) {
          const int64_t f = (int64_t)gi * d + gk;
          av = pick4(normal4<double>(a.seed, (uint32_t)(f >> 2), 0, a.epoch, a.stream), (int)(f & 3));
        }
        As[row * LDT + k] = av;
      }
    }
    for (int r = 0; r < (TN * KC) / GB; ++r) {
      const int e = tid + r * GB;
      const int k = e & (KC - 1), row = e >> 4;
      const int gj = c0 + row, gk = k0 + k;
      Bs[row * LDT + k] = (gj < d && gk <= gj) ? a.L[(size_t)gj * d + gk] : 0.0;
    }
    __syncthreads();
    mfma_chunk(As, Bs, wr, wc, lane, acc);
    __syncthreads();
  }

  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + tile_row(wr, lane, i, r), col = c0 + tile_col(wc, lane, j);
        if (row < N && col < d) a.out[(size_t)row * d + col] = a.mean ? a.mean[col] + acc[i][j][r] : acc[i][j][r];
      }
}

// p[0 .. n) = v (the uniform weights of a device initial draw)
__global__ void k_fill(double* p, int n, double v) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) p[i] = v;
}

}  // namespace edh_dense
}  // namespace pf
