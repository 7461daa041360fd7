/*
 * pf_edh.h — C ABI of the MI355X EDH (exact Daum-Huang) particle-flow filter (libpf_hip.so).
 *
 * Replaces the per-particle flow loop of the reference's EDHFlowPF
 * (/root/reference/models/EDH_particle_filter.py, cited "edh.py:LINE"): EDHConfig 58-64,
 * init_from_gaussian 173-180, step 182-317.  The Python mirror particle_filters_amd/edh.py
 * binds these entries with ctypes.
 *
 * An EDH handle IS a pf_ledh_handle: pf_ledh_init (init_from_gaussian), pf_ledh_finish
 * (resample + _weighted_stats), pf_ledh_get_particles / get_weights / set_state,
 * pf_ledh_run_ekf (device EKF tracker), pf_ledh_stream / synchronize and pf_ledh_destroy
 * accept it unchanged.  Only the flow differs, and it needs one more tracker quantity than
 * LEDH's: the past posterior mean x_{k-1|k-1} (tracker.get_past_mean(), edh.py:213), from which
 * the shared linearisation trajectory etabar starts.  pf_ledh_step / pf_ledh_run therefore
 * refuse an EDH handle (PF_E_ARG); use pf_edh_step / pf_edh_run.
 *
 * Arithmetic is fp64 (the reference's).  Conventions (status codes, ownership, one handle =
 * one device + one stream, not re-entrant) are those of pf_engine.h.
 */
#ifndef PF_EDH_H
#define PF_EDH_H

#include <stdint.h>

#include "pf_ledh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* EDHConfig.flow_integrator (edh.py:63): "rk4" (default) or "euler" (edh.py:271-280) */
#define PF_EDH_RK4 0
#define PF_EDH_EULER 1

typedef struct pf_edh_opts {
  int64_t n_particles;       /* EDHConfig.n_particles (edh.py:60) */
  int32_t n_lambda;          /* EDHConfig.n_lambda_steps (edh.py:61), clamped to >= 1 (edh.py:216) */
  double resample_ess_ratio; /* EDHConfig.resample_ess_ratio (edh.py:62); 0 disables resampling */
  uint64_t seed;             /* Philox key for PF_NOISE_DEVICE / device init / device resampling */
  int32_t device;
  int32_t integrator;        /* PF_EDH_RK4 | PF_EDH_EULER */
} pf_edh_opts;

/* EDHFlowPF.__init__ (edh.py:138-171): same model description as pf_ledh_create. */
pf_status pf_edh_create(const pf_model_desc* model, const pf_edh_opts* opts, pf_ledh_handle** out);

/* One flow step up to the weights (edh.py:185-297): P [nx][nx] = the tracker's predicted covariance
 * (symmetrised here, edh.py:197), xbar [nx] = its past mean x_{k-1|k-1} (edh.py:213), z [nz],
 * u [nx] or NULL, noise PF_NOISE_* with v [N][nx] for PF_NOISE_HOST.  info (nullable): ESS of the
 * normalised weights and the resample decision (edh.py:304-306), applied by pf_ledh_finish.
 * cond_S (nullable, [L][nz][nz]): S(lambda_j) for the condition-number diagnostics (edh.py:238-243). */
pf_status pf_edh_step(pf_ledh_handle* h, const double* P, const double* xbar, const double* z, const double* u,
                      int32_t noise, const double* v, pf_ledh_info* info, double* cond_S);

/* The whole T loop on the device with no host synchronisation inside T: Ps [T][nx][nx] tracker
 * covariances, Xbars [T][nx] the tracker's past means, Z [T][nz], U [T][nx] or NULL.  Noise
 * PF_NOISE_NONE, PF_NOISE_DEVICE (resampling uniforms from Philox) or PF_NOISE_HOST: the replayed
 * draws set by pf_ledh_set_run_replay for a run of exactly this T — step t's process noise V_t
 * [N][nx] and resampling uniform U_t, where U_t is read only on steps that resample, so the caller
 * lays the uniforms out with the decisions it expects and checks the returned flags against them.
 * A failed launch or grid-barrier timeout inside the run leaves the handle uninitialised
 * (PF_E_NOT_INITIALIZED on the next call).  Outputs as pf_ledh_run. */
pf_status pf_edh_run(pf_ledh_handle* h, const double* Ps, const double* Xbars, const double* Z, const double* U,
                     int64_t T, int32_t noise, double* means, double* covs, double* ess, uint8_t* flags);

/* 1 for a handle made by pf_edh_create. */
int32_t pf_edh_is_edh(pf_ledh_handle* h);

/* ---------------------------------------------------------------------------------------------
 * Dense EDH path: the sensor-network models (linear-Gaussian d = 64, skewed-t / Poisson d = 144, 400).
 * g(x, u, v) = alpha x + u + v, h elementwise (identity or m1 exp(m2 x)), the likelihood elementwise
 * (Gaussian with diagonal R, or the Poisson counts of the skewed-t notebook), log p(x_k | x_{k-1}) =
 * log N(x_k; alpha x_{k-1}, Q) with dense Q.  The flow of edh.py:213-280 linearises h at the tracker's
 * mean trajectory only, so the caller composes it into one affine map eta_L = M eta_0 + c per step on
 * the host and the device does the per-particle dense algebra (csrc/pf_edh_dense_kernels.h).
 * A pf_edh_dense_handle is a runtime-shape handle of its own (1 <= nx <= 1024), not a pf_ledh_handle.
 * Status codes, ownership and errors as in pf_engine.h. */
#define PF_EDH_OBS_IDENTITY 0 /* h(x) = x */
#define PF_EDH_OBS_EXP 1      /* h(x) = m1 exp(m2 x) */
#define PF_EDH_LIKE_GAUSSIAN 0 /* log N(z; h(x), diag(R_diag)) */
#define PF_EDH_LIKE_POISSON 1  /* sum z log lam - lam, lam = clip(h(x), 1e-10, 1e10) */

typedef struct pf_edh_dense_model {
  int32_t nx;
  int32_t obs_kind;      /* PF_EDH_OBS_* */
  int32_t like_kind;     /* PF_EDH_LIKE_* */
  int32_t _pad;
  double alpha;          /* g(x) = alpha x */
  double m1, m2;         /* PF_EDH_OBS_EXP */
  const double* R_diag;  /* [nx], positive; PF_EDH_LIKE_GAUSSIAN only (NULL otherwise) */
  const double* Q;       /* [nx][nx] SPD: chol(Q) and its inverse are formed on the host at create */
} pf_edh_dense_model;

typedef struct pf_edh_dense_opts {
  int64_t n_particles;       /* 1 .. 1048576 */
  double resample_ess_ratio; /* EDHConfig.resample_ess_ratio; 0 disables resampling */
  int32_t device;
  int32_t _pad;
} pf_edh_dense_opts;

typedef struct pf_edh_dense_handle pf_edh_dense_handle;

/* PF_E_ARG (bad sizes / kinds / R_diag) and PF_E_NOT_PD (Q) are reported before a device is touched. */
pf_status pf_edh_dense_create(const pf_edh_dense_model* model, const pf_edh_dense_opts* opts,
                              pf_edh_dense_handle** out);
void pf_edh_dense_destroy(pf_edh_dense_handle* h);

/* particles [N][nx], weights [N] (finite, non-negative); get_* download the current state. */
pf_status pf_edh_dense_set_state(pf_edh_dense_handle* h, const double* particles, const double* weights);
pf_status pf_edh_dense_get_particles(pf_edh_dense_handle* h, double* particles);
pf_status pf_edh_dense_get_weights(pf_edh_dense_handle* h, double* weights);

/* One step up to the weights (edh.py:199-298): eta_0 = alpha x + u + v, x_k = M eta_0 + c, the weights
 * of edh.py:287-298.  M [nx][nx], c [nx], z [nx], u [nx] or NULL, noise PF_NOISE_NONE, PF_NOISE_HOST
 * with v [N][nx], or PF_NOISE_DEVICE armed by pf_edh_dense_set_noise (below).  info (nullable): ESS and
 * the resample decision, applied by pf_edh_dense_finish.
 * PF_E_NAN when no weight is alive; the state before the step is kept. */
pf_status pf_edh_dense_step(pf_edh_dense_handle* h, const double* M, const double* c, const double* z,
                            const double* u, int32_t noise, const double* v, pf_ledh_info* info);

/* Systematic resampling with the uniform U[0] if the step decided so (edh.py:304-309; U may be NULL
 * otherwise), then _weighted_stats (edh.py:312, 321-328): mean [nx], cov [nx][nx]. */
pf_status pf_edh_dense_finish(pf_edh_dense_handle* h, const double* U, double* mean, double* cov);

/* The replayed draws of the next pf_edh_dense_run of exactly this T: V [T][N][nx] (PF_NOISE_HOST; NULL
 * for PF_NOISE_NONE and PF_NOISE_DEVICE) and the resampling uniforms U [T].  The contract is
 * pf_edh_run's: U[t] is read only on steps that resample. */
pf_status pf_edh_dense_set_run_replay(pf_edh_dense_handle* h, const double* V, const double* U, int64_t T);

/* T steps enqueued with no host synchronisation inside T: Ms [T][nx][nx], cs [T][nx], Z [T][nx],
 * U [T][nx] controls or NULL.  Outputs means [T][nx], covs [T][nx][nx], ess [T], flags [T].
 * PF_E_NAN if a step had no live weight (the handle is then uninitialised). */
pf_status pf_edh_dense_run(pf_edh_dense_handle* h, const double* Ms, const double* cs, const double* Z,
                           const double* U, int64_t T, int32_t noise, double* means, double* covs, double* ess,
                           uint8_t* flags);

/* ---------------------------------------------------------------------------------------------
 * Dense LEDH flow on the same handle (PF_EDH_OBS_EXP only): the reference's LEDHFlowPF.step
 * (models/LEDH_particle_filter.py:93-214, "ledh.py:LINE") for h(x) = m1 exp(m2 x), where every particle
 * linearises h at its own position (csrc/pf_ledh_dense_kernels.h).  P [nx][nx] is the tracker's predicted
 * covariance, symmetrised by the caller (ledh.py:106); R_diag [nx] is the diagonal of the flow's R
 * (positive; the constructor's R, not the likelihood's).  The particles run in chunks whose Cholesky
 * workspace (16 nx^2 bytes each) stays under 1 GiB.  Argument errors (n_lambda < 1, R_diag, an identity
 * handle) are PF_E_ARG before a device is touched. */

/* One step up to the weights (ledh.py:105-195); pf_edh_dense_finish completes it.  z, u, noise, v, info as
 * pf_edh_dense_step.  eta0_trace (nullable, [n_lambda][nx]): particle 0 before each lambda step, for the
 * condition numbers of ledh.py:152-157.  PF_E_NOT_PD when a pivot of some particle's S is not finite and
 * positive, PF_E_NAN when no weight is alive; the state before the step is kept in both cases. */
pf_status pf_ledh_dense_step(pf_edh_dense_handle* h, const double* P, const double* R_diag, const double* z,
                             const double* u, int32_t n_lambda, int32_t noise, const double* v, pf_ledh_info* info,
                             double* eta0_trace);

/* T steps enqueued with no host synchronisation inside T: Ps [T][nx][nx], Z [T][nx], U [T][nx] controls or
 * NULL; the draws are those of pf_edh_dense_set_run_replay, with its contract.  Outputs as pf_edh_dense_run.
 * PF_E_NOT_PD / PF_E_NAN if a step failed (the handle is then uninitialised). */
pf_status pf_ledh_dense_run(pf_edh_dense_handle* h, const double* Ps, const double* R_diag, const double* Z,
                            const double* U, int64_t T, int32_t n_lambda, int32_t noise, double* means, double* covs,
                            double* ess, uint8_t* flags);

/* ---------------------------------------------------------------------------------------------
 * Device composition of the EDH map on the same handle (csrc/pf_edh_flowmap_kernels.h): the lambda loop of
 * edh.py:216-280 for H = diag(D) and a diagonal flow R, so the caller passes the tracker's quantities, not
 * the map.  P [nx][nx] is the tracker's predicted covariance, symmetrised by the caller (edh.py:197);
 * etabar0 [nx] = g(x_{k-1|k-1}, u, 0) (edh.py:213); R_diag [nx] the diagonal of the flow's R (finite and
 * positive); integrator PF_EDH_RK4 or PF_EDH_EULER.  Argument errors (n_lambda < 1, the integrator, R_diag)
 * are PF_E_ARG before a device is touched.  The workspace (seven nx^2 buffers) is made at the first call. */

/* One step up to the weights; pf_edh_dense_finish completes it.  z, u, noise, v, info as pf_edh_dense_step.
 * etabar_trace (nullable, [n_lambda][nx]): etabar before each lambda step, for the condition numbers of
 * edh.py:238-243.  PF_E_NOT_PD when a pivot of S is not finite and positive, PF_E_NAN when no weight is
 * alive; the state before the step is kept in both cases. */
pf_status pf_edh_dense_flow_step(pf_edh_dense_handle* h, const double* P, const double* etabar0,
                                 const double* R_diag, const double* z, const double* u, int32_t n_lambda,
                                 int32_t integrator, int32_t noise, const double* v, pf_ledh_info* info,
                                 double* etabar_trace);

/* T steps enqueued with no host synchronisation inside T: Ps [T][nx][nx], etabar0s [T][nx], Z [T][nx],
 * U [T][nx] controls or NULL; the draws are those of pf_edh_dense_set_run_replay, with its contract.
 * Outputs as pf_edh_dense_run; last_trace (nullable, [n_lambda][nx]) is the last step's etabar trace.
 * PF_E_NOT_PD / PF_E_NAN if a step failed (the handle is then uninitialised). */
pf_status pf_edh_dense_flow_run(pf_edh_dense_handle* h, const double* Ps, const double* etabar0s,
                                const double* R_diag, const double* Z, const double* U, int64_t T, int32_t n_lambda,
                                int32_t integrator, int32_t noise, double* means, double* covs, double* ess,
                                uint8_t* flags, double* last_trace);

/* ---------------------------------------------------------------------------------------------
 * Device process noise on the same handle (csrc/pf_noise_dense_kernels.h): v = zeta chol(Q)^T, zeta the fp64
 * Box-Muller normals of the Philox counter (f >> 2, 0, epoch, STREAM_PROCESS), element f & 3, f = i nx + k
 * (csrc/philox.h), Q the model's.  The draw lands where an uploaded PF_NOISE_HOST v would, so a
 * PF_NOISE_DEVICE step is the PF_NOISE_HOST step on the numbers pf_edh_dense_noise_draws returns. */

/* Arms PF_NOISE_DEVICE for the next step or run on this handle, whichever dense entry it is
 * (pf_edh_dense_step / _run, _flow_step / _flow_run, _flow_step_tracked / _flow_run_tracked,
 * pf_ledh_dense_step / _run): a step draws with epoch, a run of T draws step t with epoch + t.  The entry
 * consumes it.  PF_NOISE_DEVICE without it, or with epoch + T above 2^32 - 1, is PF_E_ARG before anything
 * is enqueued.  The resampling uniforms stay the caller's (pf_edh_dense_finish, _set_run_replay with V NULL). */
pf_status pf_edh_dense_set_noise(pf_edh_dense_handle* h, uint64_t seed, uint32_t epoch);

/* V [N][nx]: the process noise a step armed with (seed, epoch) uses.  Changes no state. */
pf_status pf_edh_dense_noise_draws(pf_edh_dense_handle* h, uint64_t seed, uint32_t epoch, double* V);

/* init_from_gaussian (edh.py:173-180) with the draw on the device: particles = mean0 + zeta chol(cov0)^T on
 * STREAM_INIT (chol on the host; PF_E_NOT_PD for a cov0 that is not positive definite, the state is then
 * kept), uniform weights, and the weighted mean [nx] and cov [nx][nx] of the new state. */
pf_status pf_edh_dense_init_gaussian(pf_edh_dense_handle* h, const double* mean0, const double* cov0, uint64_t seed,
                                     uint32_t epoch, double* mean, double* cov);

/* M [nx][nx], c [nx] of the last device-composed step (tests and debugging); PF_E_ARG when there is none. */
pf_status pf_edh_dense_get_map(pf_edh_dense_handle* h, double* M, double* c);

/* The handle's stream (hipStream_t), for event timing; all entries are ordered on it. */
void* pf_edh_dense_stream(pf_edh_dense_handle* h);
pf_status pf_edh_dense_synchronize(pf_edh_dense_handle* h);

/* ---------------------------------------------------------------------------------------------
 * Dense UKF tracker with its state on the device (csrc/pf_ukf_dense_kernels.h): the additive-noise UKF of
 * models/unscented_kalman_filter.py:95-192 ("ukf.py:LINE") for g(x) = g_alpha x (+ u), h elementwise
 * (PF_EDH_OBS_*), dense symmetric Q and R, nz = nx, 1 <= nx <= 1024.  The weighted sums are centred on
 * sigma point 0, so the results are closer to exact arithmetic than the reference's plain sums, not
 * bitwise its own.  A factorisation that fails is retried once with max(jitter, 1e-12) (ukf.py:119-122,
 * the sigma points only); PF_E_NOT_PD when that fails too, or when S is not positive definite. */
typedef struct pf_ukf_dense_model {
  int32_t nx;
  int32_t obs_kind;           /* PF_EDH_OBS_* */
  double g_alpha;             /* g(x) = g_alpha x */
  double m1, m2;              /* PF_EDH_OBS_EXP */
  double alpha, beta, kappa;  /* the unscented transform; alpha^2 (nx + kappa) must be positive */
  double jitter;              /* finite, >= 0 */
  const double* Q;            /* [nx][nx] symmetric */
  const double* R;            /* [nx][nx] symmetric: the UKF's own R */
} pf_ukf_dense_model;

typedef struct pf_ukf_dense_handle pf_ukf_dense_handle;

/* PF_E_ARG (bad sizes, kinds or parameters) is reported before a device is touched. */
pf_status pf_ukf_dense_create(const pf_ukf_dense_model* model, int32_t device, pf_ukf_dense_handle** out);
void pf_ukf_dense_destroy(pf_ukf_dense_handle* t);

/* mean [nx], cov [nx][nx]; set_state also makes mean the past mean. */
pf_status pf_ukf_dense_set_state(pf_ukf_dense_handle* t, const double* mean, const double* cov);
pf_status pf_ukf_dense_get_state(pf_ukf_dense_handle* t, double* mean, double* cov);

/* predict (ukf.py:129-152; u [nx] or NULL) advances the state and records the mean from before it as the
 * past mean; update (ukf.py:154-192) takes z [nx].  After PF_E_NOT_PD the state from before the call is
 * kept. */
pf_status pf_ukf_dense_predict(pf_ukf_dense_handle* t, const double* u);
pf_status pf_ukf_dense_update(pf_ukf_dense_handle* t, const double* z);
pf_status pf_ukf_dense_get_past_mean(pf_ukf_dense_handle* t, double* past_mean);

/* T predict / update pairs enqueued at once, one synchronisation at the end: Z [T][nx], U [T][nx] or NULL.
 * Outputs (each nullable): Ps [T][nx][nx] the predicted covariances, xbars [T][nx] the past means,
 * means [T][nx] and covs [T][nx][nx] the posteriors.  On PF_E_NOT_PD the state is the one before the call
 * and pf_last_error names the first failing step. */
pf_status pf_ukf_dense_sequence(pf_ukf_dense_handle* t, const double* Z, const double* U, int64_t T, double* Ps,
                                double* xbars, double* means, double* covs);

/* pf_edh_dense_flow_run driven by a device tracker: per step, on the filter handle's stream, the tracker's
 * predict (no control, as UKFTracker.predict), etabar_0 = alpha xbar + u, the flow map from the tracker's
 * device P, the particle step and the tracker's update with Z[t].  Nothing but what pf_edh_dense_flow_run
 * moves is uploaded or downloaded inside T.  Both handles must be on one device and share nx (PF_E_ARG).
 * A tracker or flow failure (PF_E_NOT_PD / PF_E_NAN) leaves the filter handle uninitialised and the
 * tracker as it was before the call. */
pf_status pf_edh_dense_flow_run_tracked(pf_edh_dense_handle* h, pf_ukf_dense_handle* tracker, const double* R_diag,
                                        const double* Z, const double* U, int64_t T, int32_t n_lambda,
                                        int32_t integrator, int32_t noise, double* means, double* covs, double* ess,
                                        uint8_t* flags, double* last_trace);

/* One step of the same chain up to the weights, the tracker's update included; pf_edh_dense_finish
 * completes it.  z, u, noise, v, info, etabar_trace as pf_edh_dense_flow_step; P_pred (nullable,
 * [nx][nx]) receives the tracker's predicted covariance.  On PF_E_NOT_PD / PF_E_NAN the particles and the
 * tracker are as before the call. */
pf_status pf_edh_dense_flow_step_tracked(pf_edh_dense_handle* h, pf_ukf_dense_handle* tracker,
                                         const double* R_diag, const double* z, const double* u, int32_t n_lambda,
                                         int32_t integrator, int32_t noise, const double* v, pf_ledh_info* info,
                                         double* etabar_trace, double* P_pred);

#ifdef __cplusplus
}
#endif
#endif /* PF_EDH_H */
