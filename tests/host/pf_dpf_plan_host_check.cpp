// Stand-alone host check (own main; AddressSanitizer + UndefinedBehaviorSanitizer, no device) of the
// source-range split of the OT and the soft resampler (particle_filters_amd/csrc/pf_dpf_plan.h).  The
// split is part of the summation order of every result, so make_split is compared, for every N in
// 1 .. 70000 and 2^24 and every forced count the tests use, with the expressions pf_ot_create and
// pf_soft_create spelled out before the header existed (transcribed below); its invariants are
// asserted; and the values the docstrings of the GPU tests rely on are pinned.
//   make -C particle_filters_amd/csrc hostcheck   ->  build/pf_dpf_plan_host_check
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../particle_filters_amd/csrc/pf_dpf_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

using pf::dpf::make_split;
using pf::dpf::Split;

// the create functions' own lines, with their constants
static Split transcription(int N, int forced) {
  constexpr int CB = 64, IGRAIN = 32, MAXS = 64;
  Split h{};
  h.tiles = (N + CB - 1) / CB;
  const int S = std::min({(N + IGRAIN - 1) / IGRAIN, forced >= 1 ? forced : std::max(1, 8192 / std::min(8192, h.tiles)),
                          MAXS});
  h.chunk = ((N + S - 1) / S + IGRAIN - 1) / IGRAIN * IGRAIN;
  h.S = (N + h.chunk - 1) / h.chunk;
  return h;
}

static void check_one(int N, int forced) {
  const Split s = make_split(N, forced), t = transcription(N, forced);
  CHECK(s.tiles == t.tiles && s.S == t.S && s.chunk == t.chunk);
  CHECK(1 <= s.S && s.S <= 64);
  CHECK(s.chunk % 32 == 0);
  CHECK((int64_t)(s.S - 1) * s.chunk < N && N <= (int64_t)s.S * s.chunk);
  CHECK(s.tiles == (N + 63) / 64);
  if (g_failed) std::printf("  at N = %d, forced = %d\n", N, forced);
}

int main() {
  static_assert(pf::dpf::CB == 64 && pf::dpf::IGRAIN == 32 && pf::dpf::MAXS == 64, "the constants of the kernels");
  for (int forced : {0, 1, 2, 3, 7, 64, 100}) {
    for (int N = 1; N <= 70000 && !g_failed; ++N) check_one(N, forced);
    check_one(1 << 24, forced);
  }
  // (N, forced) -> (tiles, chunk, S)
  const struct { int N, forced, tiles, chunk, S; } pins[] = {
      {1, 0, 1, 32, 1},          {33, 0, 1, 32, 2},       {65, 0, 2, 32, 3},       {300, 0, 5, 32, 10},
      {300, 1, 5, 320, 1},       {300, 2, 5, 160, 2},     {300, 3, 5, 128, 3},     {2048, 0, 32, 32, 64},
      {2049, 0, 33, 64, 33},     {2500, 0, 40, 64, 40},   {2500, 1, 40, 2528, 1},  {10000, 0, 157, 224, 45},
      {1 << 24, 0, 262144, 16777216, 1}};
  for (const auto& p : pins) {
    const Split s = make_split(p.N, p.forced);
    CHECK(s.tiles == p.tiles && s.chunk == p.chunk && s.S == p.S);
    if (g_failed) std::printf("  at pin N = %d, forced = %d: (%d, %d, %d)\n", p.N, p.forced, s.tiles, s.chunk, s.S);
  }
  CHECK(pf::dpf::npad(1) == 64 && pf::dpf::npad(64) == 64 && pf::dpf::npad(65) == 128 &&
        pf::dpf::npad(1 << 24) == 1 << 24);
  if (g_failed) return 1;
  std::printf("ok\n");
  return 0;
}
