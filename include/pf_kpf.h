/*
 * pf_kpf.h — C ABI of the MI355X kernel particle flow filter (libpf_hip.so).
 *
 * Replaces the particle loop of the reference's KernelParticleFilter.analyze
 * (models/kernel_particle_filter.py, cited "kpf.py:LINE"): the scores (kpf.py:304-317), the
 * all-pairs RBF velocity of the diagonal (kpf.py:421-424) and scalar (kpf.py:408-419) kernels and
 * the clipped update (kpf.py:426-434), once per pseudo-time step.  The prior statistics
 * (kpf.py:288-294, 352-370) and the step-size schedule (kpf.py:390-445: it depends on the
 * configuration only) are the caller's; the Python mirror particle_filters_amd/kernel_pf.py
 * computes them with the reference's NumPy expressions and binds these entries with ctypes.
 *
 * Arithmetic is fp64 (the reference's).  Two calls on the same input give bitwise equal output.
 * Conventions (status codes, pf_last_error, ownership, one handle = one device + one stream,
 * not re-entrant) are those of pf_engine.h.
 */
#ifndef PF_KPF_H
#define PF_KPF_H

#include <stdint.h>

#include "pf_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* KPFConfig.kernel_type (kpf.py:237) */
#define PF_KPF_DIAGONAL 0 /* matrix-valued kernel, one 1-D RBF per state dimension */
#define PF_KPF_SCALAR 1   /* isotropic RBF of the Euclidean distance, broadcast to every dimension */

typedef struct pf_kpf_opts {
  int64_t n_particles; /* Np: rows of the ensemble given to pf_kpf_analyze */
  int32_t kernel_type; /* PF_KPF_DIAGONAL | PF_KPF_SCALAR */
  int32_t device;
} pf_kpf_opts;

typedef struct pf_kpf_handle pf_kpf_handle;

/* Model(H, JH, R) (kpf.py:210-226): nx, nz, obs_kind, obs_params and R of the description are
 * used; its transition fields and Q are ignored (the filter has no forecast step).  R is inverted
 * here, once (PF_E_NOT_PD if it is not positive definite).  PF_E_ARG for a null pointer,
 * n_particles < 1 or a bad kernel type — checked before any device is touched;
 * PF_E_UNSUPPORTED for an observation kind or shape pf_kpf_model_supported refuses. */
pf_status pf_kpf_create(const pf_model_desc* model, const pf_kpf_opts* opts, pf_kpf_handle** out);
void pf_kpf_destroy(pf_kpf_handle* h);

/* 1 when the score kernel has the observation: PF_OBS_LINEAR, PF_OBS_EXP_HALF (nz == nx) or
 * PF_OBS_ACOUSTIC (nx a multiple of 4), 1 <= nx, nz <= 1024. */
int32_t pf_kpf_model_supported(int32_t nx, int32_t nz, int32_t obs_kind);

/* One analysis (kpf.py:324-447) as a single stream-ordered sequence of launches; the call returns
 * after the results have reached the host.
 *   X [N][nx] prior ensemble, y [nz], x0 [nx] prior mean, B [nx][nx] (localised) prior covariance,
 *   B_inv [nx][nx], lengthscales [nx] (the scalar kernel reads lengthscales[0]),
 *   ds [n_steps] the pseudo-time steps (n_steps >= 0), c_move_max the Mahalanobis move limit.
 *   X_out [N][nx] posterior ensemble; n_clipped (nullable) [n_steps]: particles whose step was
 *   scaled down to c_move_max (kpf.py:429-432), per pseudo-time step. */
pf_status pf_kpf_analyze(pf_kpf_handle* h, const double* X, const double* y, const double* x0, const double* B,
                         const double* B_inv, const double* lengthscales, const double* ds, int64_t n_steps,
                         double c_move_max, double* X_out, int32_t* n_clipped);

/* The handle's hipStream_t (as void*), for event timing; and a wait for it. */
void* pf_kpf_stream(pf_kpf_handle* h);
pf_status pf_kpf_synchronize(pf_kpf_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* PF_KPF_H */
