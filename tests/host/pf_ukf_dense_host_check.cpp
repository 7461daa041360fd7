// Stand-alone host check (own main; AddressSanitizer + UndefinedBehaviorSanitizer, no device) of the host
// algebra of the dense UKF tracker (particle_filters_amd/csrc/pf_ukf_dense_plan.h): the unscented-transform
// constants against their definitions, the parameters that give no transform, and the split of the sigma
// pairs over workgroups at every dimension.
//   make -C particle_filters_amd/csrc hostcheck   ->  build/pf_ukf_dense_host_check
#include <cmath>
#include <cstdio>
#include <limits>

#include "../../particle_filters_amd/csrc/pf_ukf_dense_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fmax(1.0, std::fabs(b)); }

int main() {
  pf::UkfPlan p{};
  // the notebooks' transform at d = 144: lambda = 1e-6 144 - 144, gamma = 1e-3 12, w = 1 / (2 1.44e-4)
  CHECK(pf::ukf_plan(144, 1e-3, 2.0, 0.0, &p));
  CHECK(near(p.lambda, 1.44e-4 - 144.0) && near(p.gamma, 0.012) && near(p.w, 1.0 / 2.88e-4));
  CHECK(near(p.w0, 2.0 - 1e-6));
  // the weights of unscented_kalman_filter.py:95-104 sum to one (mean) and to 2 + w0 (covariance)
  for (int d : {1, 2, 17, 400, 1024}) {
    for (double alpha : {1e-3, 0.5, 1.0}) {
      CHECK(pf::ukf_plan(d, alpha, 2.0, 0.0, &p));
      const double s = alpha * alpha * (double)d;
      const double wm0 = p.lambda / s, wc0 = wm0 + (1.0 - alpha * alpha + 2.0);
      // the sums cancel six digits at alpha = 1e-3: the tolerance scales with the largest weight
      CHECK(std::fabs(wm0 + 2.0 * d * p.w - 1.0) <= 1e-9 * std::fmax(1.0, std::fabs(wm0)));
      CHECK(std::fabs((wc0 + 2.0 * d * p.w - 2.0) - p.w0) <= 1e-9 * std::fmax(1.0, std::fabs(wm0)));
      CHECK(near(p.gamma * p.gamma, s));
    }
  }
  CHECK(pf::ukf_plan(4, 1.0, 0.0, 3.0, &p) && near(p.lambda, 3.0) && near(p.gamma, std::sqrt(7.0)) &&
        near(p.w, 1.0 / 14.0) && near(p.w0, -1.0));
  // no usable transform
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  CHECK(!pf::ukf_plan(0, 1e-3, 2.0, 0.0, &p));
  CHECK(!pf::ukf_plan(4, 0.0, 2.0, 0.0, &p));
  CHECK(!pf::ukf_plan(4, 1.0, 2.0, -4.0, &p));
  CHECK(!pf::ukf_plan(4, 1.0, 2.0, -5.0, &p));
  CHECK(!pf::ukf_plan(4, nan, 2.0, 0.0, &p));
  CHECK(!pf::ukf_plan(4, 1.0, inf, 0.0, &p));
  CHECK(!pf::ukf_plan(4, 1.0, 2.0, nan, &p));
  CHECK(!pf::ukf_plan(4, 1e-200, 2.0, 0.0, &p));  // alpha^2 underflows to zero
  CHECK(!pf::ukf_plan(4, 1e200, 2.0, 0.0, &p));   // and overflows
  // the splits cover 0 .. d - 1 exactly, at most 16 of them, none empty
  for (int d = 1; d <= 1024; ++d) {
    CHECK(pf::ukf_plan(d, 1e-3, 2.0, 0.0, &p));
    CHECK(p.splits >= 1 && p.splits <= 16 && p.chunk >= 1);
    CHECK((long)p.splits * p.chunk >= d && (long)(p.splits - 1) * p.chunk < d);
  }
  if (g_failed) return 1;
  std::printf("ok\n");
  return 0;
}
