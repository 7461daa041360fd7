// Stand-alone host check (own main; AddressSanitizer + UndefinedBehaviorSanitizer, no device) of the
// host algebra pf_edh_dense_create runs before it touches a device: pf::chol_lower followed by
// pf::lower_inverse (particle_filters_amd/csrc/pf_host.h), W = chol(Q)^-1.
//   make -C particle_filters_amd/csrc hostcheck   ->  build/pf_edh_dense_host_check
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../particle_filters_amd/csrc/pf_host.h"

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

static bool eq(const std::vector<double>& a, std::initializer_list<double> b) {
  return a.size() == b.size() && std::equal(a.begin(), a.end(), b.begin());
}

int main() {
  std::vector<double> L, W;
  // exact dyadic cases
  const double A[4] = {4, 2, 2, 5};  // L = [[2, 0], [1, 2]]
  CHECK(pf::chol_lower(A, 2, 0.0, L));
  pf::lower_inverse(L.data(), 2, W);
  CHECK(eq(W, {0.5, 0, -0.25, 0.5}));
  const double I1[1] = {4};
  CHECK(pf::chol_lower(I1, 1, 0.0, L));
  pf::lower_inverse(L.data(), 1, W);
  CHECK(eq(W, {0.5}));
  const double T3[9] = {1, 0, 0, 2, 4, 0, -1, 2, 2};  // a lower-triangular factor given directly
  pf::lower_inverse(T3, 3, W);
  CHECK(eq(W, {1, 0, 0, -0.5, 0.25, 0, 1, -0.25, 0.5}));
  // sizes around the product kernel's tiles: W L = I and W Q W^T = I to rounding, upper triangle zero
  for (int n : {1, 3, 16, 17, 65, 144}) {
    std::vector<double> Q((size_t)n * n);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        const double dd = (double)(i - j);
        Q[(size_t)i * n + j] = std::exp(-dd * dd / 8.0) + (i == j ? 1e-3 : 0.0);  // the sensor network's kernel
      }
    CHECK(pf::chol_lower(Q.data(), n, 0.0, L));
    pf::lower_inverse(L.data(), n, W);
    CHECK(W.size() == (size_t)n * n);
    double worst = 0.0, upper = 0.0, wmax = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += W[(size_t)i * n + k] * L[(size_t)k * n + j];
        worst = std::fmax(worst, std::fabs(s - (i == j ? 1.0 : 0.0)));
        if (j > i) upper = std::fmax(upper, std::fabs(W[(size_t)i * n + j]));
        wmax = std::fmax(wmax, std::fabs(W[(size_t)i * n + j]));
      }
    CHECK(upper == 0.0);
    CHECK(worst <= 1e-12 * std::fmax(1.0, wmax) * n);  // |W| |L| n eps, |L| <= ~1
  }
  if (g_failed) return 1;
  std::printf("ok\n");
  return 0;
}
