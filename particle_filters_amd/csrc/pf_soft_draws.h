// The Gumbel draws of the soft resampler (include/pf_engine.h, "The draws" of the pf_soft_* block):
// the problem descriptor that carries the Philox key and counter words, and the map from a Philox
// call to the uniforms and Gumbels of a source pair.  Shared by pf_soft_kernels.h and the baseline
// resampler of pf_rnn_kernels.h, which must form the same draws.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pf_dpf_plan.h"
#include "philox.h"

namespace pf {
namespace soft {

struct Prob {
  int N, Npad, d, B;
  uint32_t k0, k1;  // the Philox key: (lo32(seed), hi32(seed))
  uint32_t epoch;
  uint32_t batch_base;
};

// host: the descriptor of B problems of N particles with the draws of (seed, epoch, batch_base + b)
inline Prob make_prob(int N, int d, int B, uint64_t seed, uint32_t epoch, uint32_t batch_base) {
  return Prob{N, dpf::npad(N), d, B, (uint32_t)seed, (uint32_t)(seed >> 32), epoch, batch_base};
}

// the fourth counter word of problem b
__device__ __forceinline__ uint32_t stream_word(const Prob& p, int b) {
  return STREAM_GUMBEL + 256u * (p.batch_base + (uint32_t)b);
}

// u = (2 m + 1) 2^-53 with the 52-bit m = (hi >> 6) : (lo >> 6): exact in fp64, strictly inside (0, 1)
__host__ __device__ __forceinline__ double soft_uniform(uint32_t hi, uint32_t lo) {
  const uint64_t m = ((uint64_t)(hi >> 6) << 26) | (uint64_t)(lo >> 6);
  return (double)(2 * m + 1) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ double gumbel(double u) { return -log(-log(u)); }

// the Philox call of output row i and the source pair jp = j >> 1: (x, y) serve j even, (z, w) j odd
__device__ __forceinline__ u32x4 pair_words(const Prob& p, uint32_t w3, uint32_t jp, uint32_t i) {
  return philox4x32_10(u32x4{jp, i, p.epoch, w3}, p.k0, p.k1);
}

}  // namespace soft
}  // namespace pf
