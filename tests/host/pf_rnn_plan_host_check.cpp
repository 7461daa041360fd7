// Stand-alone host check (own main; AddressSanitizer + UndefinedBehaviorSanitizer, no device) of the shape
// plan of the RNN resampler's recurrence (particle_filters_amd/csrc/pf_rnn_plan.h): over a sweep of
// (N, d, H, L, cell) up to the limits of pf_rnn_create the LDS request fits a CU, the padded sizes cover H,
// the tiles cover N, the fragments of every matrix are disjoint and fill the fragment buffer, the
// reference's own configurations are resident and the largest one streams.  With the arguments
// "N d H L cell" it prints one line instead, "HT KS RS threads tiles resident lds_bytes frag_doubles" of
// make_plan for that shape (tests/test_dpf_rnn_host.py asks it what each parity case exercises).
//   make -C particle_filters_amd/csrc hostcheck   ->  build/pf_rnn_plan_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../particle_filters_amd/csrc/pf_rnn_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

using namespace pf::rnn;

// "N d H L cell" (cell: lstm or gru): the plan of one shape, for tests that ask what a case exercises
static int print_plan(char** v) {
  const long N = std::atol(v[0]);
  const int d = std::atoi(v[1]), H = std::atoi(v[2]), L = std::atoi(v[3]);
  const bool lstm = !std::strcmp(v[4], "lstm");
  if (N < 1 || N > 16384 || d < 1 || d > 1024 || H < 1 || H > MAXH || L < 1 || L > MAXL || (!lstm && std::strcmp(v[4], "gru"))) {
    std::fprintf(stderr, "usage: N d H L lstm|gru, within the limits of pf_rnn_create\n");
    return 2;
  }
  const Plan p = make_plan(N, d, H, L, lstm ? CELL_LSTM : CELL_GRU);
  std::printf("%d %d %d %d %d %d %zu %zu\n", p.HT, p.KS, p.RS, p.threads, p.tiles, p.resident ? 1 : 0, p.lds_bytes,
              p.frag_doubles);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 6) return print_plan(argv + 1);
  if (argc != 1) {
    std::fprintf(stderr, "usage: no arguments (the sweep), or N d H L lstm|gru\n");
    return 2;
  }
  const long Ns[] = {1, 3, 15, 16, 17, 33, 100, 1000, 16384};
  const int ds[] = {1, 5, 1024};
  for (long N : Ns)
    for (int d : ds)
      for (int H = 1; H <= MAXH; ++H)
        for (int L = 1; L <= MAXL; ++L)
          for (int cell : {CELL_LSTM, CELL_GRU})
            for (int forced : {0, 1}) {
              const Plan p = make_plan(N, d, H, L, cell, true, true, forced != 0);
              CHECK(p.lds_bytes <= LDS_CU_BYTES && p.lds_bytes > 0);
              CHECK(p.Hp >= H && p.Hp - H < 16 && p.Hp == 16 * p.HT);
              CHECK(4 * p.KS >= H && 4 * p.KS - H < 4 && 4 * p.KS <= p.Hp);
              CHECK(p.threads == 64 * p.HT * p.RS && p.threads <= 512 && 4 % p.RS == 0);
              CHECK(p.HT >= 3 ? p.RS == 1 : p.HT * p.RS == 4);  // small H: four waves, one per SIMD
              CHECK((long)p.tiles * RT >= N && (long)(p.tiles - 1) * RT < N);
              CHECK(p.F0 == 1 + d);
              CHECK(p.state_doubles == (size_t)2 * L * p.Hp * HS);
              CHECK(p.frag_doubles == frag_offset(p, 2 * L - 1, 0, 0, 0));
              if (forced) CHECK(!p.resident);
              CHECK(p.lds_bytes == (p.state_doubles + (p.resident ? p.frag_doubles : 0)) * sizeof(double));
              if (!forced && !p.resident) CHECK((p.state_doubles + p.frag_doubles) * sizeof(double) > LDS_CU_BYTES);
            }
  // every fragment of a plan is addressed once: the offsets are a permutation of the multiples of 64
  for (int H : {1, 5, 24, 40, 64, 65, 100, 128})
    for (int L : {1, 3, 4}) {
      const Plan p = make_plan(17, 2, H, L, CELL_GRU);
      std::vector<int> seen(p.frag_doubles / 64, 0);
      for (int m = 0; m < 2 * L - 1; ++m)
        for (int t = 0; t < p.HT; ++t)
          for (int ks = 0; ks < p.KS; ++ks)
            for (int s = 0; s < SLOTS; ++s) {
              const size_t o = frag_offset(p, m, t, ks, s);
              CHECK(o % 64 == 0 && o / 64 < seen.size());
              if (o / 64 < seen.size()) ++seen[o / 64];
            }
      for (int v : seen) CHECK(v == 1);
    }
  CHECK(make_plan(10, 3, 8, 1, CELL_LSTM, true, false).F0 == 1);
  CHECK(make_plan(10, 3, 8, 1, CELL_LSTM, false, true).F0 == 3);
  // the reference's own configurations keep their weights on chip
  for (int cell : {CELL_LSTM, CELL_GRU}) {
    for (int H = 1; H <= 32; ++H)
      for (int L = 1; L <= 2; ++L) CHECK(make_plan(100, 1, H, L, cell).resident);
    CHECK(make_plan(100, 1, 64, 1, cell).resident);
    CHECK(make_plan(1000, 4, 64, 1, cell).resident);
    CHECK(!make_plan(100, 1, 128, 4, cell).resident);
    CHECK(!make_plan(100, 1, 64, 2, cell).resident);
  }
  if (g_failed) return 1;
  std::printf("ok\n");
  return 0;
}
