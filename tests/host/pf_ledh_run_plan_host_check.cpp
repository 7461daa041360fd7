// Stand-alone host check (own main; AddressSanitizer + UndefinedBehaviorSanitizer, no device) of the
// run bookkeeping of the LEDH / EDH engine flows (particle_filters_amd/csrc/pf_ledh_run_plan.h): the
// mean ring against a brute-force model and against the pointer rotation it replaced, the chunk
// starts, the arena layout at hand-computed shapes and past 2^32 bytes, and the EKF slots.
//   make -C particle_filters_amd/csrc hostcheck   ->  build/pf_ledh_run_plan_host_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../particle_filters_amd/csrc/pf_ledh_run_plan.h"

using namespace pf::ledh;

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

// The ring over a run of T steps.  label[b] is the step whose mean buffer b holds (-1: the latest
// mean before the run, which is in buffer 0 = mean_prev; -2: nothing a step may read).
static void check_ring(int64_t T) {
  int64_t label[3] = {-1, -2, -2};
  MeanRing r;
  // the rotation run_impl held in raw pointers before this header: shp, shc, mw, spare
  int shp = 0, shc = 0, mw = 1;
  const int spare = 2;
  std::vector<int> given((size_t)T);  // the shift launch t gave step t
  for (int64_t t = 0; t < T; ++t) {
    CHECK(r.prev_shift == shp && r.shift == shc && r.write == mw);
    CHECK(label[r.shift] == (t - 2 > -1 ? t - 2 : -1));
    given[(size_t)t] = r.shift;
    if (t > 0) {
      CHECK(r.prev_shift == given[(size_t)t - 1]);
      CHECK(r.write != r.shift && r.write != r.prev_shift);
      label[r.write] = t - 1;
    }
    r.advance(t);
    if (t > 0) {
      const int freed = shp != shc ? shp : spare;
      shp = shc;
      shc = mw;
      mw = freed;
    }
  }
  // the tail reduces step T - 1
  CHECK(r.prev_shift == shp && r.write == mw);
  CHECK(r.prev_shift == given[(size_t)T - 1]);
  CHECK(r.write != r.prev_shift);
  label[r.write] = T - 1;
  int src[3] = {-1, -1, -1};
  r.commit(src);
  int seen[3] = {0, 0, 0};
  for (int i = 0; i < 3; ++i) {
    CHECK(src[i] >= 0 && src[i] < 3);
    if (src[i] >= 0 && src[i] < 3) ++seen[src[i]];
  }
  CHECK(seen[0] == 1 && seen[1] == 1 && seen[2] == 1);
  CHECK(label[src[0]] == T - 1);
  CHECK(src[1] < src[2]);  // the other two keep their order
  // the swaps it replaced: mw == 1: swap(prev, mean); mw == 2: swap(prev, mean3), swap(mean, mean3)
  int old[3] = {0, 1, 2};
  if (mw == 1) {
    old[0] = 1, old[1] = 0;
  } else if (mw == 2) {
    old[0] = 2, old[1] = 0, old[2] = 1;
  }
  CHECK(src[0] == old[0] && src[1] == old[1] && src[2] == old[2]);
}

static void check_chunks(int64_t T) {
  const std::vector<int64_t> c = run_chunk_starts(T);
  CHECK(!c.empty() && c[0] == 0);
  int64_t want = 2, covered = 0;
  for (size_t k = 0; k < c.size(); ++k) {
    const int64_t end = k + 1 < c.size() ? c[k + 1] : T;
    CHECK(c[k] == covered);  // no gap, no overlap
    CHECK(end > c[k]);       // strictly increasing
    const int64_t n = end - c[k];
    if (k + 1 < c.size()) CHECK(n == want);
    else CHECK(n >= 1 && n <= want);  // the last one clipped
    covered = end;
    want = 2 * want < 16 ? 2 * want : 16;
  }
  CHECK(covered == T);
}

// the sum run_impl computed before this header
static uint64_t old_total(int nx, int nz, uint64_t T, uint64_t tsz, bool has_U, bool ekf, bool edh, bool tabled) {
  const uint64_t ne = 2 * (uint64_t)nx + 3 * (uint64_t)nx * nx + (uint64_t)nz * nz;
  const uint64_t b[] = {T * nx * nx * 8, T * nz * 8, has_U ? T * nx * 8 : 0, T * nx * 8, T * nx * nx * 8, T * 8, T * 4,
                        ekf ? ne * 8 : 0, edh ? T * nx * 8 : 0, tabled ? T * tsz * 8 : 0};
  uint64_t need = 0;
  for (uint64_t q : b) need += (q + 255) / 256 * 256;
  return need;
}

static void check_arena_invariants(const RunArena& a) {
  uint64_t end = 0;
  char* const base = reinterpret_cast<char*>((uintptr_t)4096);  // never dereferenced
  for (int i = 0; i < RUN_PIECES; ++i) {
    CHECK(a.off[i] % 256 == 0);
    CHECK(a.off[i] >= end);  // ordered, no overlap
    if (a.bytes[i]) {
      end = a.off[i] + a.bytes[i];
      CHECK(a.at<char>(base, (RunPiece)i) == base + a.off[i]);
    } else {
      CHECK(a.at<char>(base, (RunPiece)i) == nullptr);
      if (i + 1 < RUN_PIECES) CHECK(a.off[i + 1] == a.off[i]);  // takes no space
    }
  }
  CHECK(a.total >= end && a.total % 256 == 0 && a.total - end < 256);
}

int main() {
  for (int64_t T = 1; T <= 40; ++T) check_ring(T);
  for (int64_t T = 1; T <= 100; ++T) check_chunks(T);
  {
    const std::vector<int64_t> c = run_chunk_starts(31);
    CHECK(c.size() == 5 && c[1] == 2 && c[2] == 6 && c[3] == 14 && c[4] == 30);
    CHECK(run_chunk_starts(0).empty());
  }

  // EKF slots: x0 | P0 | Qt | Rt | x_final | P_final
  {
    constexpr EkfSlots e(40, 10);
    static_assert(e.ne == 2 * 40 + 3 * 1600 + 100, "ne = 2 nx + 3 nx^2 + nz^2");
    CHECK(e.x0 == 0 && e.P0 == 40 && e.Qt == 1640 && e.Rt == 3240 && e.x_final == 3340 && e.P_final == 3380);
    CHECK(e.ne == 4980);
    constexpr EkfSlots s(1, 1);
    CHECK(s.x0 == 0 && s.P0 == 1 && s.Qt == 2 && s.Rt == 3 && s.x_final == 4 && s.P_final == 5 && s.ne == 6);
    constexpr EkfSlots m(16, 25);
    CHECK(m.ne == 2 * 16 + 3 * 256 + 625);
  }

  // arena at nx = 40, nz = 10, L = 8, T = 3: the table is 50 + 8 * 551 + 1640 = 6098 doubles, and by
  // hand P 38400, Z 256, U 1024, means 1024, covs 38400, ess 256, flags 256, EKF 39936 (4980
  // doubles), past means 1024, tables 146432 bytes
  {
    const uint64_t tsz = 6098;
    const RunArena ledh = run_arena(40, 10, 3, tsz, false, false, false, true);
    CHECK(ledh.total == 225024);
    CHECK(run_arena(40, 10, 3, tsz, false, true, false, true).total == 264960);
    CHECK(run_arena(40, 10, 3, tsz, false, false, true, true).total == 226048);
    CHECK(run_arena(40, 10, 3, tsz, false, true, true, true).total == 265984);
    CHECK(run_arena(40, 10, 3, tsz, true, true, true, true).total == 267008);
    CHECK(run_arena(40, 10, 3, tsz, false, false, false, false).total == 78592);  // per-particle flow: no tables
    for (int m = 0; m < 16; ++m) {
      const bool u = m & 1, ekf = m & 2, edh = m & 4, tab = m & 8;
      const RunArena a = run_arena(40, 10, 3, tsz, u, ekf, edh, tab);
      CHECK(a.total == old_total(40, 10, 3, tsz, u, ekf, edh, tab));
      check_arena_invariants(a);
      CHECK((a.bytes[RUN_U] != 0) == u && (a.bytes[RUN_EKF] != 0) == ekf && (a.bytes[RUN_XBAR] != 0) == edh &&
            (a.bytes[RUN_TABLES] != 0) == tab);
    }
    CHECK(ledh.off[RUN_P] == 0 && ledh.off[RUN_Z] == 38400 && ledh.off[RUN_U] == 38656 &&
          ledh.off[RUN_MEANS] == 38656 && ledh.off[RUN_COVS] == 39680 && ledh.off[RUN_ESS] == 78080 &&
          ledh.off[RUN_FLAGS] == 78336 && ledh.off[RUN_TABLES] == 78592);
    // odd shapes: every piece rounds up
    for (int64_t T = 1; T <= 9; ++T) {
      const RunArena a = run_arena(1, 1, T, 7, true, true, true, true);
      check_arena_invariants(a);
      CHECK(a.total == old_total(1, 1, (uint64_t)T, 7, true, true, true, true));
    }
    // 64-bit sizes: T = 2^20 at nx = 40 puts P alone past 2^33 bytes
    const int64_t big = (int64_t)1 << 20;
    const RunArena b = run_arena(40, 10, big, tsz, true, true, true, true);
    check_arena_invariants(b);
    CHECK(b.bytes[RUN_P] == 13421772800ull && b.bytes[RUN_TABLES] == 51153731584ull);
    CHECK(b.off[RUN_Z] == 13421772800ull);
    CHECK(b.total == old_total(40, 10, (uint64_t)big, tsz, true, true, true, true));
    CHECK(b.total > ((uint64_t)1 << 36));
  }
  if (g_failed) return 1;
  std::printf("ok\n");
  return 0;
}
