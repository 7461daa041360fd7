// Host algebra of the dense UKF tracker (pf_ukf_dense_* in pf_edh_dense.hip): the unscented-transform
// constants in the reference's expressions (unscented_kalman_filter.py:95-104) and the split of the sigma
// pairs over workgroups.  Host code only, no HIP: tests/host/pf_ukf_dense_host_check.cpp runs it alone.
#pragma once
#include <algorithm>
#include <cmath>

namespace pf {

struct UkfPlan {
  double lambda, gamma;  // alpha^2 (d + kappa) - d, sqrt(d + lambda)
  double w;              // Wm_i = Wc_i = 1 / (2 (d + lambda)), i >= 1
  double w0;             // sum_k Wc_k - 2 = beta - alpha^2: the weight of delta delta^T in the centred sums
  int splits, chunk;     // k_ukf_sigma: columns of the factor per blockIdx.y (part of the summation order)
};

// false when the parameters give no usable transform (d + lambda must be finite and positive)
inline bool ukf_plan(int d, double alpha, double beta, double kappa, UkfPlan* p) {
  if (d < 1 || !std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(kappa)) return false;
  // d + lambda is taken directly, not as d + (alpha^2 (d + kappa) - d), which loses ten digits at 1e-3
  const double s = alpha * alpha * ((double)d + kappa);
  p->lambda = s - (double)d;
  if (!(s > 0.0) || !std::isfinite(s)) return false;
  p->gamma = std::sqrt(s);
  p->w = 1.0 / (2.0 * s);
  p->w0 = (1.0 - alpha * alpha + beta) - 1.0;
  if (!std::isfinite(p->w) || !std::isfinite(p->w0)) return false;
  const int S = std::min(16, (d + 63) / 64);
  p->chunk = (d + S - 1) / S;
  p->splits = (d + p->chunk - 1) / p->chunk;
  return true;
}

}  // namespace pf
