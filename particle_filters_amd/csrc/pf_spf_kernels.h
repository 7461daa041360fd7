// Kernels of the stochastic particle flow filter (include/pf_spf.h): every Euler-Maruyama step of
// one pf_spf_advance in a single launch, fp64.
//
// Layout.  One particle per lane, one instantiation per padded dimension NP = 4 ceil(n / 4)
// (4, 8, .. 64).  A step is x <- c + A x + G zeta.  The lane holds the NP sums of the new state in
// registers (acc[i], i a compile-time index: every loop over rows is fully unrolled) and walks the
// columns j = 0 .. n-1 in a run-time loop: x_j comes from the lane's own column of the LDS state
// tile xs[j][lane] (bank-conflict free, private to the lane: no barrier guards it), the column
// A[:, j] from the step's parameter block in LDS, read at a wave-uniform address (a broadcast
// ds_read_b128 feeds two rows; a column's reads are issued together, ahead of its multiply-adds:
// read-then-use pairs left one read in flight and were 1.6 x slower at n = 40).  The noise goes
// the same way by column groups of four: four normals per Philox call (or four host normals),
// then the 4 x 4 blocks of G on and below the diagonal, the row block a compile-time index guarded
// by a wave-uniform branch.  After the last column the sums are written back to the tile.  The
// state is read from HBM once before the first step and written once after the last.
//
// Parameters.  The packed block of a step (SpfLayout: A transposed [n][NP], c [NP], G as 4 x 4
// blocks of its lower block triangle, column block major, each block [col][row]) is the same for
// every lane and is staged through an LDS double buffer: at the top of step s the workgroup copies
// step s + 1's block into the other buffer, then computes step s; one barrier per step orders the
// copy of s + 1 before its use and the reads of s before the buffer is overwritten at s + 2.  At
// n = 64 a block is 6336 doubles (49.5 KB; with G square it would be 64.5 KB and two buffers plus
// one wave's state tile would not fit the 160 KB), so two buffers and a 64-lane state tile take
// 131 KB.  LDS, not uniform loads from global memory: a lane's fused multiply-add takes its matrix
// operand from a VGPR either way unless the whole wave shares it, and the scalar data cache that
// would serve shared operands is 16 KB, a third of one step's block at n = 64, with every wave of
// the chip streaming through it; the LDS copy is one coalesced pass per workgroup and step.
//
// Padding.  Rows n .. NP-1 of A^T, c and G are zero, columns >= n are never visited (the column
// loop ends at n; G's padded columns are zero and meet finite normals only), so a padded sum is
// never read and a non-finite state component cannot reach a real one through the padding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace pf {
namespace spf {

// device layout of one step's parameter block, in doubles
struct SpfLayout {
  int n, NP, NB;
  __host__ __device__ SpfLayout(int n_) : n(n_), NP((n_ + 3) / 4 * 4), NB((n_ + 3) / 4) {}
  __host__ __device__ int at(int j, int i) const { return j * NP + i; }  // A[i][j]
  __host__ __device__ int c0() const { return n * NP; }
  __host__ __device__ int g0() const { return n * NP + NP; }
  // 4 x 4 block (row block ib >= column block jb), blocks of a column block contiguous
  __host__ __device__ int gblock(int ib, int jb) const { return g0() + 16 * (jb * NB - jb * (jb - 1) / 2 + (ib - jb)); }
  __host__ __device__ int size() const { return g0() + 16 * (NB * (NB + 1) / 2); }
};

// X0[i] = m0 + L0 zeta_i (pf_spf_draw_prior): one particle per thread, the row accumulated in
// place in column order, as the step kernel's noise.  L0 [n][n] row-major, lower triangular.
__global__ void __launch_bounds__(256) k_spf_prior(double* __restrict__ X, const double* __restrict__ m0,
                                                   const double* __restrict__ L0, int64_t N, int n, uint64_t seed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int NB = (n + 3) / 4;
  double* x = X + i * n;
  for (int r = 0; r < n; ++r) x[r] = m0[r];
  for (int jb = 0; jb < NB; ++jb) {
    const Normal4<double> z = normal4<double>(seed, (uint32_t)(i * NB + jb), 0u, 0u, STREAM_INIT);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = 4 * jb + c;
      if (j < n)
        for (int r = j; r < n; ++r) x[r] = fma(L0[r * n + j], z.v[c], x[r]);
    }
  }
}

// All the steps of one pf_spf_advance.  Dynamic LDS: 2 * SpfLayout(n).size() doubles of parameter
// buffers, then the state tile [NP][blockDim.x].  P: device copy of the packed blocks
// [n_steps][size()]; Z: null, or host normals [n_steps][N][n].
template <int NP>
__global__ void __launch_bounds__(256) k_spf_advance(double* __restrict__ X, const double* __restrict__ P,
                                                     const double* __restrict__ Z, int64_t N, int n, int n_steps,
                                                     uint32_t epoch0, uint64_t seed) {
  extern __shared__ double2 spf_lds2[];
  double* lds = reinterpret_cast<double*>(spf_lds2);
  constexpr int NB = NP / 4;
  const SpfLayout L(n);
  const int PB = L.size(), tid = threadIdx.x, BS = blockDim.x;
  double* xs = lds + 2 * PB + tid;  // xs[j * BS]: this lane's component j
  const int64_t i = (int64_t)blockIdx.x * BS + tid;
  const bool active = i < N;

  for (int e = tid; e < PB / 2; e += BS)  // PB is even: NP is a multiple of 4
    reinterpret_cast<double2*>(lds)[e] = reinterpret_cast<const double2*>(P)[e];
  if (active)
    for (int j = 0; j < n; ++j) xs[j * BS] = X[i * n + j];
  __syncthreads();

  for (int s = 0; s < n_steps; ++s) {
    const double* cur = lds + (s & 1) * PB;
    if (s + 1 < n_steps) {
      double2* nxt = reinterpret_cast<double2*>(lds + ((s + 1) & 1) * PB);
      const double2* src = reinterpret_cast<const double2*>(P + (int64_t)(s + 1) * PB);
      for (int e = tid; e < PB / 2; e += BS) nxt[e] = src[e];
    }
    if (active) {
      double acc[NP];
#pragma unroll
      for (int r = 0; r < NP; r += 2) {
        const double2 c = *reinterpret_cast<const double2*>(cur + L.c0() + r);
        acc[r] = c.x;
        acc[r + 1] = c.y;
      }
#pragma unroll 1
      for (int j = 0; j < n; ++j) {
        const double xj = xs[j * BS];
        const double2* a = reinterpret_cast<const double2*>(cur + j * NP);
        double2 v[NP / 2];  // the whole column first: the reads are in flight together
#pragma unroll
        for (int r = 0; r < NP / 2; ++r) v[r] = a[r];
#pragma unroll
        for (int r = 0; r < NP / 2; ++r) {
          acc[2 * r] = fma(v[r].x, xj, acc[2 * r]);
          acc[2 * r + 1] = fma(v[r].y, xj, acc[2 * r + 1]);
        }
      }
      const double* zrow = Z ? Z + ((int64_t)s * N + i) * n : nullptr;
#pragma unroll 1
      for (int jb = 0; jb < NB; ++jb) {
        Normal4<double> z;
        if (zrow) {
#pragma unroll
          for (int c = 0; c < 4; ++c) z.v[c] = 4 * jb + c < n ? zrow[4 * jb + c] : 0.0;
        } else {
          z = normal4<double>(seed, (uint32_t)(i * NB + jb), 0u, epoch0 + (uint32_t)s, STREAM_PROCESS);
        }
        const double* gcol = cur + L.gblock(jb, jb);
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) {
          if (ib >= jb) {  // wave-uniform
            const double2* g = reinterpret_cast<const double2*>(gcol + 16 * (ib - jb));
            double2 v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = g[q];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              acc[4 * ib + 0] = fma(v[2 * c].x, z.v[c], acc[4 * ib + 0]);
              acc[4 * ib + 1] = fma(v[2 * c].y, z.v[c], acc[4 * ib + 1]);
              acc[4 * ib + 2] = fma(v[2 * c + 1].x, z.v[c], acc[4 * ib + 2]);
              acc[4 * ib + 3] = fma(v[2 * c + 1].y, z.v[c], acc[4 * ib + 3]);
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < NP; ++r) xs[r * BS] = acc[r];
    }
    __syncthreads();
  }
  if (active)
    for (int j = 0; j < n; ++j) X[i * n + j] = xs[j * BS];
}

}  // namespace spf
}  // namespace pf
