// The split of the source range shared by the all-pairs kernels of the OT and the soft resampler
// (pf_ot_kernels.h: k_ot_tau_cols, k_ot_project; pf_soft_kernels.h: k_soft_pass, k_soft_entropy,
// k_soft_bwd_pass).  One 64-lane workgroup owns 64 outputs and a chunk of the N sources; the S
// partials per output are merged by a second kernel.  The split is part of the summation order, so
// it fixes the bits of every result: a pure host function of N alone (a problem's bits do not
// depend on the batch it is solved in), checked stand-alone by tests/host/pf_dpf_plan_host_check.cpp.
#pragma once
#include <algorithm>
#include <cstdint>

namespace pf {
namespace dpf {

constexpr int CB = 64;      // lanes (outputs) per workgroup of the split kernels
constexpr int IGRAIN = 32;  // granularity of a split of the source range (even: pairs never straddle)
constexpr int MAXS = 64;    // most partials per output

// the row stride of the padded [Npad] device arrays: N up to whole workgroups
inline int npad(int N) { return (N + CB - 1) / CB * CB; }

struct Split {
  int tiles;  // ceil(N / CB): workgroups along the outputs
  int S;      // chunks of the source range, 1 .. MAXS
  int chunk;  // sources per chunk, a multiple of IGRAIN
};

// Split the sources until about 8 waves per SIMD are in flight (8192 workgroups of one wave: each
// wave's loads, or its fp64 log and exp calls, are a dependent chain).
// forced >= 1 asks for that many chunks instead (tests: 1 is the unsplit order).
inline Split make_split(int64_t N, int forced) {
  Split s{};
  const int n = (int)N;
  s.tiles = (n + CB - 1) / CB;
  const int S = std::min({(n + IGRAIN - 1) / IGRAIN, forced >= 1 ? forced : std::max(1, 8192 / std::min(8192, s.tiles)),
                          MAXS});
  s.chunk = ((n + S - 1) / S + IGRAIN - 1) / IGRAIN * IGRAIN;
  s.S = (n + s.chunk - 1) / s.chunk;
  return s;
}

}  // namespace dpf
}  // namespace pf
