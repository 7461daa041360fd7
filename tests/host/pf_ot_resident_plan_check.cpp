// Stand-alone check of the LDS plan of the one-launch Sinkhorn solver (csrc/pf_ot_resident_plan.h), the
// one statement of the layout that k_ot_resident and the host share.  Its own main, host code only,
// built with AddressSanitizer and UndefinedBehaviorSanitizer by `make hostcheck`; no device.
//
// For every N in 1 .. 128: the regions are 8-byte aligned, inside [0, total) and pairwise disjoint (red
// excepted, which must lie inside pm .. ps: the declared alias); total <= 163840 bytes; npad is
// pf_dpf_plan.h's; the g pass's waves cover every (column, source) once: ncw column waves of 64, S
// splits of `chunk` rows with S chunk >= N, ncw S = RES_WAVES.  The index arithmetic of the kernel is
// walked on a buffer of `total` bytes, so an index outside a region is a sanitizer report.  N = 0,
// N = 129 and larger are refused.  The plan does not depend on d (X is read through L2), so the
// extremes of d have nothing to add to it: the kernel's largest index in d, (d << 7) at d = 1024, is
// checked to stay in an int.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../particle_filters_amd/csrc/pf_dpf_plan.h"
#include "../../particle_filters_amd/csrc/pf_ot_resident_plan.h"

using namespace pf::ot;

#define CHECK(c)                                                                    \
  do {                                                                              \
    if (!(c)) {                                                                     \
      std::fprintf(stderr, "N = %d: check failed: %s (line %d)\n", N, #c, __LINE__); \
      return 1;                                                                     \
    }                                                                               \
  } while (0)

static int check(int N) {
  const ResidentPlan p = resident_plan(N);
  CHECK(p.fits);
  CHECK(p.N == N && p.npad == pf::dpf::npad(N) && (p.npad == 64 || p.npad == 128));
  CHECK(p.ncw * 64 == p.npad && p.ncw * p.S == RES_WAVES && p.S * p.chunk >= N && p.chunk >= 1);
  CHECK(p.total <= RES_LDS_MAX);
  const uint32_t vec = (uint32_t)p.npad * 8, part = (uint32_t)p.S * p.npad;
  const std::vector<std::pair<uint32_t, uint32_t>> regions = {
      {p.C, (uint32_t)N * vec}, {p.a, vec}, {p.f, vec}, {p.g, vec}, {p.fold, vec}, {p.gold, vec}, {p.x2, vec},
      {p.pm, part * 8}, {p.ps, part * 8}, {p.pam, part * 4}, {p.flag, 8}};
  for (size_t i = 0; i < regions.size(); ++i) {
    CHECK(regions[i].first % 8 == 0 && regions[i].first + regions[i].second <= p.total);
    for (size_t j = i + 1; j < regions.size(); ++j)
      CHECK(regions[i].first + regions[i].second <= regions[j].first ||
            regions[j].first + regions[j].second <= regions[i].first);
  }
  CHECK(p.red % 8 == 0 && p.red >= p.pm && p.red + (uint32_t)RES_THREADS * 8 <= p.ps + part * 8 && p.ps == p.pm + part * 8);

  // the kernel's indices, on a buffer of exactly `total` bytes
  std::vector<unsigned char> lds(p.total, 0);
  double* C = (double*)(lds.data() + p.C);
  double* pm = (double*)(lds.data() + p.pm);
  int32_t* pam = (int32_t*)(lds.data() + p.pam);
  double* red = (double*)(lds.data() + p.red);
  const int sh = p.npad == 64 ? 6 : 7;
  for (int e = 0; e < N * p.npad; ++e) {
    const int i = e >> sh, j = e - (i << sh);
    CHECK(i < N && j < p.npad);
    C[e] += 1.0;
  }
  std::vector<int> seen((size_t)N * N, 0);
  for (int wv = 0; wv < RES_WAVES; ++wv)
    for (int lane = 0; lane < 64; ++lane) {
      const int cw = wv % p.ncw, sp = wv / p.ncw, gj = cw * 64 + lane;
      const int i0 = N < sp * p.chunk ? N : sp * p.chunk, i1 = N < i0 + p.chunk ? N : i0 + p.chunk;
      if (gj >= N) continue;
      for (int i = i0; i < i1; ++i) {
        C[(i << sh) + gj] += 1.0;
        ++seen[(size_t)i * N + gj];
      }
      pm[sp * p.npad + gj] = 1.0;
      pam[sp * p.npad + gj] = 1;
    }
  for (int v : seen) CHECK(v == 1);
  for (int t = 0; t < RES_THREADS; ++t) red[t] = 1.0;
  ((int32_t*)(lds.data() + p.flag))[0] = 1;
  return 0;
}

int main() {
  int n = 0;
  for (int N = 1; N <= RES_MAXN; ++N, ++n)
    if (check(N)) return 1;
  for (int N : {0, -1, 129, 130, 1 << 20}) {
    CHECK(!resident_plan(N).fits);
    ++n;
  }
  {
    const int N = RES_MAXN;
    CHECK((int64_t)pf::dpf::MAXS >= 1 && ((int64_t)1024 << 7) + RES_THREADS < INT32_MAX);
  }
  std::printf("%d cases ok\n", n);
  return 0;
}
