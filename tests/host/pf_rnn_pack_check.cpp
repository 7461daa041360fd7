// Stand-alone host check (own main; AddressSanitizer + UndefinedBehaviorSanitizer, no device, no HIP)
// of the index maps of the RNN resampler's weight packing (particle_filters_amd/csrc/pf_rnn_plan.h:
// pack_src_W0x, pack_src_W0i, pack_src_binit, pack_src_frag, pack_fragT_from_frag), which k_rnn_pack
// and k_rnn_pack_T evaluate on the device, one thread per destination element.
//
// The layout is stated here a second time, as the packing loops of pf_rnn_set_weights and of the
// host transposition the backward pass used before the maps existed - copied, and not to be
// "simplified" onto the maps.  For every hidden size H = 1 .. 128, layer count L = 1 .. 4, both
// cells, the three feature settings and N in {1, 5, 17} (d = 2) the Keras arrays are filled with
// distinct values and W0x, W0i, binit, frag and fragT are built twice, by the loops and by
// evaluating the maps for every destination element:
//   * the two agree in every byte;
//   * a map never points outside its source array;
//   * a destination element is zero or comes from one source element (the GRU's z and r biases: the
//     sum of two of the same array), and every element of every cell array feeds exactly one
//     element of the forward buffers; fragT is a permutation of elements of frag and zeros.
// The fragments do not depend on the feature setting or on N, so they are built for the first of
// those per (H, L, cell) and the three small buffers for all of them.
//   make -C particle_filters_amd/csrc hostcheck   ->  build/pf_rnn_pack_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../particle_filters_amd/csrc/pf_rnn_plan.h"

static long g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (g_failed < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

using namespace pf::rnn;
typedef std::vector<double> Vec;

// ---- the layout as the loops state it (pf_rnn_set_weights, and the host transposition) ----
static int slot_of(int cell, int gate, bool rec) { return (cell == CELL_GRU && rec && gate == 2) ? 3 : gate; }

static void pack_loops(const Plan& p, int N, int H, int L, int cell, const std::vector<Vec>& arrays, bool frags,
                       Vec& W0x, Vec& W0i, Vec& binit, Vec& frag, Vec& fragT) {
  const int G = cell == CELL_LSTM ? 4 : 3, GH = G * H, Hp = p.Hp, W4 = SLOTS * Hp;
  W0x.assign((size_t)p.F0 * W4, 0.0), W0i.assign((size_t)N * W4, 0.0), binit.assign((size_t)L * W4, 0.0);
  frag.assign(frags ? p.frag_doubles : 0, 0.0), fragT.assign(frags ? p.frag_doubles : 0, 0.0);
  for (int l = 0; l < L; ++l) {
    const double *K = arrays[3 * l].data(), *R = arrays[3 * l + 1].data(), *bias = arrays[3 * l + 2].data();
    for (int g = 0; g < G; ++g)
      for (int u = 0; u < H; ++u) {
        const size_t col = (size_t)slot_of(cell, g, false) * Hp + u;
        if (cell == CELL_LSTM) {
          binit[(size_t)l * W4 + col] = bias[g * H + u];
        } else if (g < 2) {
          binit[(size_t)l * W4 + col] = bias[g * H + u] + bias[3 * H + g * H + u];
        } else {
          binit[(size_t)l * W4 + col] = bias[g * H + u];
          binit[(size_t)l * W4 + (size_t)slot_of(cell, g, true) * Hp + u] = bias[3 * H + g * H + u];
        }
        if (l == 0) {
          for (int f = 0; f < p.F0; ++f) W0x[(size_t)f * W4 + col] = K[(size_t)f * GH + g * H + u];
          for (int i = 0; i < N; ++i) W0i[(size_t)i * W4 + col] = K[(size_t)(p.F0 + i) * GH + g * H + u];
        }
      }
    if (!frags) continue;
    for (int which = (l == 0 ? 1 : 0); which < 2; ++which) {  // 0: input kernel, 1: recurrent kernel
      const double* M = which ? R : K;
      const int m = which ? 2 * l : 2 * l - 1;
      for (int tile = 0; tile < p.HT; ++tile)
        for (int ks = 0; ks < p.KS; ++ks)
          for (int g = 0; g < G; ++g) {
            double* f = frag.data() + frag_offset(p, m, tile, ks, slot_of(cell, g, which == 1));
            for (int lane = 0; lane < 64; ++lane) {
              const int k = 4 * ks + (lane >> 4), u = 16 * tile + (lane & 15);
              if (k < H && u < H) f[lane] = M[(size_t)k * GH + g * H + u];
            }
          }
    }
  }
  if (!frags) return;
  for (int m = 0; m < 2 * L - 1; ++m)
    for (int tile = 0; tile < p.HT; ++tile)
      for (int ks = 0; ks < p.KS; ++ks)
        for (int slot = 0; slot < SLOTS; ++slot) {
          double* f = fragT.data() + frag_offset(p, m, tile, ks, slot);
          for (int lane = 0; lane < 64; ++lane) {
            const int k = 16 * tile + (lane & 15), u = 4 * ks + (lane >> 4);
            if (k < 4 * p.KS) f[lane] = frag[frag_offset(p, m, u / 16, k / 4, slot) + 16 * (k % 4) + u % 16];
          }
        }
}

// ---- the same by the maps ----
struct Uses {
  std::vector<std::vector<int>> n;  // per array, per element: destinations it feeds
};

template <class Map>
static void pack_by_map(const PackNet& net, const std::vector<Vec>& arrays, size_t count, Map map, Vec& out, Uses& uses) {
  out.assign(count, -1.0);
  for (size_t e = 0; e < count; ++e) {
    const PackSrc s = map(net, (int64_t)e);
    if (s.arr < 0) {
      CHECK(s.arr == -1);
      out[e] = 0.0;
      continue;
    }
    const bool ok = s.arr < (int)arrays.size() && s.idx >= 0 && s.idx < (int64_t)arrays[s.arr].size() &&
                    s.idx2 < (int64_t)arrays[s.arr].size() && s.idx2 != s.idx;
    CHECK(ok);
    if (!ok) continue;
    const Vec& a = arrays[s.arr];
    out[e] = s.idx2 >= 0 ? a[s.idx] + a[s.idx2] : a[s.idx];
    ++uses.n[s.arr][s.idx];
    if (s.idx2 >= 0) ++uses.n[s.arr][s.idx2];
  }
}

static bool same_bytes(const Vec& a, const Vec& b) {
  return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(double)));
}

static void check_case(int N, int d, int H, int L, int cell, bool uw, bool up, bool frags) {
  const Plan p = make_plan(N, d, H, L, cell, uw, up);
  const PackNet net = pack_net(p, N, H, L, cell);
  const int G = cell == CELL_LSTM ? 4 : 3, W4 = SLOTS * p.Hp;
  // the Keras arrays, every element another value, none of them zero
  std::vector<Vec> arrays(3 * L + 2);
  double next = 1.0;
  for (int k = 0; k < 3 * L + 2; ++k) {
    size_t n;
    if (k < 3 * L)
      n = k % 3 == 0 ? (size_t)(k == 0 ? p.F0 + N : H) * G * H : k % 3 == 1 ? (size_t)H * G * H : (size_t)(cell == CELL_LSTM ? 4 : 6) * H;
    else
      n = k == 3 * L ? (size_t)H * N : (size_t)N;
    arrays[k].resize(n);
    for (double& v : arrays[k]) v = (next += 1.0) + 0.5;
  }
  Vec W0x, W0i, binit, frag, fragT;
  pack_loops(p, N, H, L, cell, arrays, frags, W0x, W0i, binit, frag, fragT);
  Uses uses;
  uses.n.resize(arrays.size());
  for (size_t k = 0; k < arrays.size(); ++k) uses.n[k].assign(arrays[k].size(), 0);
  Vec m0x, m0i, mb, mf;
  pack_by_map(net, arrays, (size_t)p.F0 * W4, pack_src_W0x, m0x, uses);
  pack_by_map(net, arrays, (size_t)N * W4, pack_src_W0i, m0i, uses);
  pack_by_map(net, arrays, (size_t)L * W4, pack_src_binit, mb, uses);
  CHECK(same_bytes(m0x, W0x));
  CHECK(same_bytes(m0i, W0i));
  CHECK(same_bytes(mb, binit));
  // layer 0's kernel and every bias: each element feeds exactly one destination
  for (int k = 0; k < 3 * L; ++k)
    if (k == 0 || k % 3 == 2)
      for (int c : uses.n[k]) CHECK(c == 1);
  if (!frags) return;
  pack_by_map(net, arrays, p.frag_doubles, pack_src_frag, mf, uses);
  CHECK(same_bytes(mf, frag));
  for (int k = 1; k < 3 * L; ++k)  // the recurrent kernels, and the input kernels of the layers above 0
    if (k % 3 != 2)
      for (int c : uses.n[k]) CHECK(c == 1);
  // fragT: a permutation of elements of frag, and zeros
  Vec mT(p.frag_doubles, -1.0);
  std::vector<int> taken(p.frag_doubles, 0);
  for (size_t e = 0; e < p.frag_doubles; ++e) {
    const int64_t s = pack_fragT_from_frag(net, (int64_t)e);
    CHECK(s >= -1 && s < (int64_t)p.frag_doubles);
    if (s < -1 || s >= (int64_t)p.frag_doubles) continue;
    mT[e] = s >= 0 ? mf[s] : 0.0;
    if (s >= 0) ++taken[s];
  }
  CHECK(same_bytes(mT, fragT));
  for (size_t e = 0; e < p.frag_doubles; ++e) {
    CHECK(taken[e] <= 1);
    if (mf[e] != 0.0) CHECK(taken[e] == 1);  // no weight is lost in the transposition
  }
}

int main() {
  const int d = 2, Ns[3] = {1, 5, 17};
  const bool feats[3][2] = {{true, true}, {true, false}, {false, true}};
  long cases = 0;
  for (int H = 1; H <= MAXH; ++H)
    for (int L = 1; L <= MAXL; ++L)
      for (int cell = CELL_LSTM; cell <= CELL_GRU; ++cell)
        for (int f = 0; f < 3; ++f)
          for (int n = 0; n < 3; ++n) {
            check_case(Ns[n], d, H, L, cell, feats[f][0], feats[f][1], f == 0 && n == 2);
            ++cases;
          }
  // the gates a slot takes, spelled out: GRU slot 2 is the input half of h, slot 3 the recurrent half
  CHECK(pack_gate(CELL_GRU, 2, false) == 2 && pack_gate(CELL_GRU, 2, true) == -1);
  CHECK(pack_gate(CELL_GRU, 3, false) == -1 && pack_gate(CELL_GRU, 3, true) == 2);
  CHECK(pack_gate(CELL_LSTM, 3, false) == 3 && pack_gate(CELL_LSTM, 3, true) == 3);
  if (g_failed) {
    std::printf("%ld checks failed\n", g_failed);
    return 1;
  }
  std::printf("%ld cases ok\n", cases);
  return 0;
}
