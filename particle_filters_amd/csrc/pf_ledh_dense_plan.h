// Chunk plan of the dense LEDH flow (pf_ledh_dense_step / pf_ledh_dense_run): a resident particle
// needs a workspace of 2 d^2 doubles (its two Cholesky factors), the host caps the workspace and
// runs the particles in chunks by successive launches.  Pure host code with 64-bit sizes (N d^2 8
// passes 2^32 long before N = 1048576, d = 1024); tests/host/pf_ledh_dense_host_check.cpp.
#pragma once
#include <stdint.h>

namespace pf {

constexpr int64_t LEDH_DENSE_WS_CAP = (int64_t)1 << 30;  // default cap, bytes

struct LedhDensePlan {
  int64_t per_particle;  // workspace bytes of one particle, 16 d^2
  int64_t chunk;         // particles per launch
  int64_t launches;      // ceil(N / chunk)
  int64_t ws_bytes;      // chunk * per_particle <= cap
};

// false when the arguments are out of range or the cap does not hold one particle's workspace
inline bool ledh_dense_plan(int64_t N, int64_t d, int64_t cap_bytes, LedhDensePlan* p) {
  if (!p || N < 1 || N > 1048576 || d < 1 || d > 1024 || cap_bytes < 1) return false;
  const int64_t per = 16 * d * d;
  const int64_t fit = cap_bytes / per;
  if (fit < 1) return false;
  p->per_particle = per;
  p->chunk = fit < N ? fit : N;
  p->launches = (N + p->chunk - 1) / p->chunk;
  p->ws_bytes = p->chunk * per;
  return true;
}

}  // namespace pf
