/*
 * pf_spf.h — C ABI of the MI355X stochastic particle flow filter (libpf_hip.so).
 *
 * Replaces the particle loop of the reference's run_generalized_spf
 * (models/Stochastic_particle_filter.py, cited "spf.py:LINE"): the Euler-Maruyama steps in the
 * homotopy parameter (spf.py:362-404).  For the linear-Gaussian model the function accepts, a step
 * is the same affine map for every particle plus Gaussian noise,
 *     x <- A_k x + c_k + G_k zeta,      zeta ~ N(0, I),  G_k lower triangular,
 * and the caller folds the model (H, R, z, P0, m0), the schedule and the step matrices
 * (spf.py:366-391) into (A_k, c_k, G_k); the Python mirror particle_filters_amd/stochastic_pf.py
 * does that with the reference's NumPy expressions and binds these entries with ctypes.  The device
 * never sees the observation dimension.
 *
 * Arithmetic is fp64 (the reference's).  All the steps of one pf_spf_advance are one launch with
 * the particle state kept on chip.  Device draws are Philox4x32-10 with the fp64 Box-Muller
 * (philox.h normal4<double>); with n4 = 4 * ceil(n / 4) the four normals for dims 4j .. 4j+3 of
 * particle i come from counter (i * n4 / 4 + j, 0, epoch, stream): epoch 0 on STREAM_INIT for the
 * prior, epoch k + 1 on STREAM_PROCESS for step k.  A result therefore depends neither on the grid
 * nor on how the steps are split over calls, and two calls on the same input are bitwise equal.
 * Conventions (status codes, pf_last_error, ownership, one handle = one device + one stream,
 * not re-entrant) are those of pf_engine.h.  No C++ exception leaves a call: a failed host
 * allocation is reported as PF_E_HIP.
 */
#ifndef PF_SPF_H
#define PF_SPF_H

#include <stdint.h>

#include "pf_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pf_spf_opts {
  int64_t n_particles; /* N */
  int32_t n;           /* state dimension, 1 .. 64 */
  int32_t device;
} pf_spf_opts;

typedef struct pf_spf_handle pf_spf_handle;

/* PF_E_ARG for a null pointer, n_particles < 1 or N * n4 / 4 >= 2^32 (the Philox group index);
 * PF_E_UNSUPPORTED for n outside 1 .. 64 — all checked before any device is touched.  The
 * particles of a new handle are zero. */
pf_status pf_spf_create(const pf_spf_opts* opts, pf_spf_handle** out);
void pf_spf_destroy(pf_spf_handle* h);

/* 1 when the step kernel has the dimension: 1 <= n <= 64. */
int32_t pf_spf_supported(int32_t n);

/* X [N][n] from the host. */
pf_status pf_spf_set_particles(pf_spf_handle* h, const double* X);

/* X0 = m0 + L0 zeta on the device (spf.py:338-339 with device draws): m0 [n], L0 [n][n] lower
 * triangular (entries above the diagonal are not read). */
pf_status pf_spf_draw_prior(pf_spf_handle* h, const double* m0, const double* L0, uint64_t seed);

/* Steps k0 .. k0 + n_steps - 1 on the handle's particles, one launch.
 *   params [n_steps][n*n + n + n*n]: per step A [n][n], c [n], G [n][n] row-major (G lower
 *   triangular; entries above the diagonal are not read);
 *   Z nullable [n_steps][N][n]: host normals used in place of the device draws (seed is then
 *   ignored); k0 only numbers the draws (epoch k0 + s + 1 for the s-th step of the call).
 * n_steps = 0 is a no-op.  The call returns after the launch has completed. */
pf_status pf_spf_advance(pf_spf_handle* h, const double* params, int64_t k0, int64_t n_steps, uint64_t seed,
                         const double* Z);

/* X_out [N][n] to the host. */
pf_status pf_spf_get_particles(pf_spf_handle* h, double* X_out);

/* Lanes per workgroup of the handle's step launch (256, 128 or 64; 0 for a null handle): the
 * largest whose state tile fits the 160 KB of LDS beside the two parameter buffers, halved while
 * there are fewer than 512 workgroups.  It cannot change a result; tests read it to know which
 * geometry they ran. */
int32_t pf_spf_workgroup(pf_spf_handle* h);

/* The handle's hipStream_t (as void*), for event timing; and a wait for it. */
void* pf_spf_stream(pf_spf_handle* h);
pf_status pf_spf_synchronize(pf_spf_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* PF_SPF_H */
