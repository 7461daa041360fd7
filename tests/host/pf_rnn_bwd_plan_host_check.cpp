// Stand-alone host check (own main; AddressSanitizer + UndefinedBehaviorSanitizer, no device) of the plan of
// the RNN resampler's backward pass (particle_filters_amd/csrc/pf_rnn_bwd_plan.h): over a sweep of
// (N, d, B, H, L, cell) the LDS request fits a CU, residency is what the sizes say, the chunks of the
// weight-gradient reduction cover the timesteps once, the history blocks are a bijection onto
// 0 .. blocks - 1, the Keras sizes are those pf_rnn_set_weights checks, and the workspace is the sum of
// its parts.  With the arguments "N d B H L cell" it prints one line instead:
// "resident lds_bytes wg_tc wg_chunks workspace_bytes".
//   make -C particle_filters_amd/csrc hostcheck   ->  build/pf_rnn_bwd_plan_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../particle_filters_amd/csrc/pf_rnn_bwd_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

using namespace pf::rnn;

static int print_plan(char** v) {
  const long N = std::atol(v[0]);
  const int d = std::atoi(v[1]), B = std::atoi(v[2]), H = std::atoi(v[3]), L = std::atoi(v[4]);
  const bool lstm = !std::strcmp(v[5], "lstm");
  if (N < 1 || N > 16384 || d < 1 || d > 1024 || B < 1 || H < 1 || H > MAXH || L < 1 || L > MAXL ||
      (!lstm && std::strcmp(v[5], "gru"))) {
    std::fprintf(stderr, "usage: N d B H L lstm|gru, within the limits of pf_rnn_create\n");
    return 2;
  }
  const int cell = lstm ? CELL_LSTM : CELL_GRU;
  const BwdPlan q = make_bwd_plan(make_plan(N, d, H, L, cell), N, d, B, H, L, cell);
  std::printf("%d %zu %d %d %zu\n", q.resident ? 1 : 0, q.lds_bytes, q.wg_tc, q.wg_chunks, q.workspace_bytes);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 7) return print_plan(argv + 1);
  if (argc != 1) {
    std::fprintf(stderr, "usage: no arguments (the sweep), or N d B H L lstm|gru\n");
    return 2;
  }
  const long Ns[] = {1, 3, 7, 8, 9, 16, 17, 33, 100, 511, 512, 513, 1000, 16384};
  for (long N : Ns)
    for (int d : {1, 5, 1024})
      for (int B : {1, 3})
        for (int H = 1; H <= MAXH; ++H)
          for (int L = 1; L <= MAXL; ++L)
            for (int cell : {CELL_LSTM, CELL_GRU})
              for (int forced : {0, 1}) {
                const Plan p = make_plan(N, d, H, L, cell, true, true, forced != 0);
                const BwdPlan q = make_bwd_plan(p, N, d, B, H, L, cell, forced != 0);
                const size_t W4 = (size_t)SLOTS * p.Hp;
                CHECK(q.lds_bytes <= LDS_CU_BYTES && q.lds_bytes > 0);
                CHECK(q.stage_doubles == (size_t)6 * p.Hp * HS);
                if (forced) CHECK(!q.resident);
                CHECK(q.lds_bytes == (q.stage_doubles + (q.resident ? 2 * p.frag_doubles : 0)) * sizeof(double));
                if (!forced && !q.resident) CHECK((q.stage_doubles + 2 * p.frag_doubles) * sizeof(double) > LDS_CU_BYTES);
                CHECK(q.wg_tc >= 1 && q.wg_chunks >= 1 && q.wg_chunks <= WG_MAX_CHUNKS);
                CHECK((long)q.wg_tc * q.wg_chunks >= N && (long)q.wg_tc * (q.wg_chunks - 1) < N);
                CHECK(q.blocks == (size_t)B * p.tiles * N * L);
                CHECK(q.hist_doubles == q.blocks * RT * p.Hp && q.dz_doubles == 4 * q.hist_doubles);
                CHECK(q.c_doubles == (cell == CELL_LSTM ? q.hist_doubles : 0));
                CHECK(q.mats == 2 * L - 1 && q.part_doubles == (size_t)B * q.mats * q.wg_chunks * p.Hp * W4);
                int64_t sizes[3 * MAXL + 2];
                const int G = cell == CELL_LSTM ? 4 : 3;
                size_t all = keras_sizes(N, p.F0, H, L, cell, sizes), sum = 0;
                for (int k = 0; k < 3 * L + 2; ++k) sum += (size_t)sizes[k];
                CHECK(all == sum && all == q.out_doubles);
                CHECK(sizes[0] == (int64_t)(p.F0 + N) * G * H && sizes[1] == (int64_t)H * G * H);
                CHECK(sizes[2] == (cell == CELL_LSTM ? 4 : 6) * H && sizes[3 * L] == (int64_t)H * N && sizes[3 * L + 1] == N);
                CHECK(q.workspace_bytes ==
                      8 * (q.hist_doubles + q.c_doubles + q.dz_doubles + p.frag_doubles + q.part_doubles + q.sums_doubles +
                           q.w0i_doubles + q.k0x_doubles + q.dense_doubles + q.pair_doubles + q.vec_doubles + q.out_doubles));
              }
  // the history blocks of a plan are addressed once each
  for (long N : {1L, 17L, 33L})
    for (int L : {1, 3}) {
      const int B = 2, tiles = (int)((N + RT - 1) / RT);
      std::vector<int> seen((size_t)B * tiles * N * L, 0);
      for (int b = 0; b < B; ++b)
        for (int tile = 0; tile < tiles; ++tile)
          for (long t = 0; t < N; ++t)
            for (int l = 0; l < L; ++l) {
              const size_t o = hist_block(tiles, N, L, b, tile, t, l);
              CHECK(o < seen.size());
              if (o < seen.size()) ++seen[o];
            }
      for (int v : seen) CHECK(v == 1);
    }
  // the benchmark's network keeps both sets of fragments on chip; the largest streams
  for (int cell : {CELL_LSTM, CELL_GRU}) {
    CHECK(make_bwd_plan(make_plan(100, 1, 32, 1, cell), 100, 1, 1, 32, 1, cell).resident);
    CHECK(!make_bwd_plan(make_plan(100, 1, 128, 4, cell), 100, 1, 1, 128, 4, cell).resident);
  }
  if (g_failed) return 1;
  std::printf("ok\n");
  return 0;
}
