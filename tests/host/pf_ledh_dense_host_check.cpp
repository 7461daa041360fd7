// Stand-alone host check (own main; AddressSanitizer + UndefinedBehaviorSanitizer, no device) of the
// chunk plan of the dense LEDH flow (particle_filters_amd/csrc/pf_ledh_dense_plan.h): 64-bit sizes at
// the limits, a cap below one particle's workspace, exact multiples and a remainder chunk of one.
//   make -C particle_filters_amd/csrc hostcheck   ->  build/pf_ledh_dense_host_check
#include <cstdint>
#include <cstdio>

#include "../../particle_filters_amd/csrc/pf_ledh_dense_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

// the launches cover 0 .. N - 1 exactly once, in order, each within the chunk
static bool covers(const pf::LedhDensePlan& p, int64_t N) {
  int64_t first = 0, launches = 0;
  while (first < N) {
    const int64_t n = p.chunk < N - first ? p.chunk : N - first;
    if (n < 1 || n > p.chunk) return false;
    first += n;
    ++launches;
  }
  return first == N && launches == p.launches;
}

int main() {
  pf::LedhDensePlan p{};
  const int64_t GiB = (int64_t)1 << 30;
  // the limits: one particle is 16 * 1024^2 = 16 MiB, N d^2 8 is 2^43
  CHECK(pf::ledh_dense_plan(1048576, 1024, GiB, &p));
  CHECK(p.per_particle == 16777216 && p.chunk == 64 && p.launches == 16384 && p.ws_bytes == GiB);
  CHECK(covers(p, 1048576));
  CHECK(pf::ledh_dense_plan(1048576, 1024, pf::LEDH_DENSE_WS_CAP, &p) && p.chunk == 64);
  // a cap that would hold every particle: the product passes 2^32 (and 2^44) without wrapping
  CHECK(pf::ledh_dense_plan(1048576, 1024, INT64_MAX, &p));
  CHECK(p.chunk == 1048576 && p.launches == 1 && p.ws_bytes == (int64_t)1048576 * 16777216);
  // a cap below one particle's workspace
  CHECK(!pf::ledh_dense_plan(1048576, 1024, 16777215, &p));
  CHECK(!pf::ledh_dense_plan(5, 33, 16 * 33 * 33 - 1, &p));
  CHECK(pf::ledh_dense_plan(5, 33, 16 * 33 * 33, &p) && p.chunk == 1 && p.launches == 5);
  CHECK(!pf::ledh_dense_plan(5, 33, 0, &p));
  CHECK(!pf::ledh_dense_plan(5, 33, -1, &p));
  // exact multiples
  CHECK(pf::ledh_dense_plan(64, 400, 16 * (int64_t)400 * 400 * 16, &p));
  CHECK(p.chunk == 16 && p.launches == 4 && p.ws_bytes == 16 * (int64_t)400 * 400 * 16 && covers(p, 64));
  CHECK(pf::ledh_dense_plan(200, 144, GiB, &p) && p.chunk == 200 && p.launches == 1);
  CHECK(p.ws_bytes == 200 * (int64_t)16 * 144 * 144);
  // a remainder chunk of one, and the tests' forced chunks of 7 at N = 65, d = 33
  CHECK(pf::ledh_dense_plan(65, 33, 16 * 33 * 33 * 8, &p) && p.chunk == 8 && p.launches == 9 && covers(p, 65));
  CHECK(pf::ledh_dense_plan(65, 33, 16 * 33 * 33 * 7 + 100, &p) && p.chunk == 7 && p.launches == 10 && covers(p, 65));
  CHECK(pf::ledh_dense_plan(1, 1, 16, &p) && p.chunk == 1 && p.launches == 1 && p.ws_bytes == 16);
  // ranges
  CHECK(!pf::ledh_dense_plan(0, 4, GiB, &p));
  CHECK(!pf::ledh_dense_plan(1048577, 4, GiB, &p));
  CHECK(!pf::ledh_dense_plan(4, 0, GiB, &p));
  CHECK(!pf::ledh_dense_plan(4, 1025, GiB, &p));
  CHECK(!pf::ledh_dense_plan(4, 4, GiB, nullptr));
  if (g_failed) return 1;
  std::printf("ok\n");
  return 0;
}
