/*
 * pf_engine.h — C ABI of the MI355X SIR particle-filter engine (libpf_hip.so).
 *
 * Plain C types only (pointers + sizes); no torch / HIP types cross this line.
 * Every entry point returns a pf_status (PF_OK == 0); pf_last_error() gives a
 * thread-local message for the last failure.  Host arrays are caller-owned and
 * copied in/out; device buffers are owned by the handle.  One handle = one
 * device + one HIP stream, not re-entrant; separate handles may be driven from
 * separate threads.
 *
 * Each entry replaces a piece of the reference's Python filter
 * (/root/reference/models/particle_filter.py, cited "pf.py:LINE"); the Python
 * mirror particle_filters_amd/particle_filter.py binds them via ctypes (see
 * INTEGRATION.md for the binding a maintainer of the reference would add).
 */
#ifndef PF_ENGINE_H
#define PF_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t pf_status;
#define PF_OK 0
#define PF_E_NOT_INITIALIZED 1 /* -> AssertionError("Filter not initialized.") pf.py:142,231,252 */
#define PF_E_ARG 2             /* bad shape / argument -> ValueError */
#define PF_E_NOT_PD 3          /* Cholesky failed -> numpy.linalg.LinAlgError */
#define PF_E_HIP 4             /* HIP runtime error */
#define PF_E_UNSUPPORTED 5     /* model shape not compiled into this library */
#define PF_E_NAN 6             /* every particle weight zero or NaN (all-dead filter) -> FloatingPointError */
#define PF_E_RETRY 7           /* pf_run_device: the resident grid was not co-resident; nothing computed, state
                                  unchanged, the handle launches cooperatively from now on: run again */

/* g: transition kinds (pf.py:237 per-particle g(x,u)) */
#define PF_TRANS_LINEAR 0 /* x' = A x (+ u)                         params: A[nx*nx]         */
#define PF_TRANS_L96 1    /* one RK4 step of Lorenz-96              params: F, dt            */
/* h: observation kinds (pf.py:257 per-particle h(x)) */
#define PF_OBS_LINEAR 0   /* z = H x + c                            params: H[nz*nx], c[nz]  */
#define PF_OBS_EXP_HALF 1 /* z_k = beta_k exp(x_k / 2)   (nz==nx)   params: beta[nz]         */
#define PF_OBS_ACOUSTIC 2 /* z_s = sum_c psi/(|p_c-s|^2+d0) (nx=4C) params: psi, d0, sx[nz], sy[nz] */
#define PF_OBS_SV_EXACT 3 /* exact SV likelihood y_k ~ N(0, beta_k^2 e^{x_k}) (nz==nx) params: beta[nz];
                             log p = -x/2 - y^2 e^{-x}/(2 beta^2): test_dpf_vs_sv_simulator.py:60-97.
                             R is not used (pass any PD matrix, e.g. I). */
#define PF_OBS_BEARINGS 4 /* angles of a sensor at s: [atan2(x0-s0, x1-s1), atan2(x2-s2, |(x0,x1)-(s0,s1)|)]
                             (nz==2, nx>=3)                          params: s[3]
                             (SPF_results_reproduction_example2.ipynb cell 1 e2_measurement_function) */

#define PF_RESAMPLE_SYSTEMATIC 0 /* pf.py:146-171 */
#define PF_RESAMPLE_MULTINOMIAL 1 /* pf.py:173-186 (any other method string) */

#define PF_PRECISION_FP32 0
#define PF_PRECISION_FP64 1

typedef struct pf_model_desc {
  int32_t nx, nz;
  int32_t trans_kind, obs_kind;
  const double* trans_params; /* see PF_TRANS_* */
  int64_t n_trans_params;
  const double* obs_params;   /* see PF_OBS_* */
  int64_t n_obs_params;
  const double* Q; /* nx*nx process-noise covariance (pf.py:94) */
  const double* R; /* nz*nz measurement-noise covariance (pf.py:95) */
} pf_model_desc;

typedef struct pf_opts {
  int64_t n_particles;     /* Np (pf.py:96) */
  int32_t n_replicates;    /* independent filters batched in one launch (>= 1) */
  int32_t resample_method; /* PF_RESAMPLE_* (pf.py:98, 205-208) */
  double resample_thresh;  /* resample when Neff < thresh * Np (pf.py:97, 204) */
  int32_t regularize;      /* jitter 0.001*chol(Q) n after resampling (pf.py:99, 212-218) */
  int32_t precision;       /* PF_PRECISION_* : particle storage / arithmetic type */
  uint64_t seed;           /* Philox key; replicate r uses counter word r */
  int32_t device;          /* HIP device ordinal */
  int32_t replicate_base;  /* global id of local replicate 0: replicate r draws with counter
                              word replicate_base + r, so sharding replicates over GPUs gives
                              bitwise the same per-replicate results as one GPU */
  int32_t kernel_path;     /* PF_PATH_*: which step kernels serve the model */
} pf_opts;

#define PF_PATH_AUTO 0    /* the compiled shape's kernels when (nx, nz, g, h) is in the compiled list,
                             else the runtime-shape kernels */
#define PF_PATH_RUNTIME 1 /* always the runtime-shape kernels (pf_dyn.h): any nx, nz */

typedef struct pf_handle pf_handle;

/* Per-replicate posterior summary of one update (pf.py:262-268). */
typedef struct pf_update_info {
  double neff;     /* pre-resample 1/sum w^2 (pf.py:203) */
  double log_norm; /* log sum_i w_{t-1,i} exp(-quad_i/2): marginal-likelihood increment */
  int32_t resample; /* 1 if Neff < thresh*Np (the resample is applied by pf_resample) */
  int32_t _pad;
} pf_update_info;

const char* pf_last_error(void);
const char* pf_version(void);
int32_t pf_device_count(void);

/* ParticleFilter.__init__ (pf.py:79-107): validates the model, factorises R
 * (+1e-12 I) and Q (+1e-10 I / +1e-12 I fallbacks), allocates device state. */
pf_status pf_create(const pf_model_desc* model, const pf_opts* opts, pf_handle** out);
void pf_destroy(pf_handle* h);
/* Can the engine run (nx, nz, trans_kind, obs_kind)?  Any positive shape whose kinds fit
 * (EXP_HALF / SV_EXACT: nz == nx; ACOUSTIC: nx % 4 == 0; BEARINGS: nz == 2, nx >= 3). */
int32_t pf_model_supported(int32_t nx, int32_t nz, int32_t trans_kind, int32_t obs_kind);
/* Is the shape in the compiled (register-state) list, i.e. does PF_PATH_AUTO pick those kernels? */
int32_t pf_model_compiled(int32_t nx, int32_t nz, int32_t trans_kind, int32_t obs_kind);
/* PF_PATH_RUNTIME if the handle runs the runtime-shape kernels, else PF_PATH_AUTO. */
int32_t pf_kernel_path(pf_handle* h);
/* 1 if the handle's last fused step launch ran the persistent many-replicate kernel (k_step_stream:
 * fp32 scalar models with per-step replicate heads; PF_STREAM=0 turns it off), else 0.  Diagnostics. */
int32_t pf_last_step_streamed(pf_handle* h);

/* initialize (pf.py:110-132): particles ~ N(mean_r, cov_r), uniform weights.
 * mean [R][nx], cov [R][nx][nx]; replay_normals [R][N][nx] or NULL (device Philox). */
pf_status pf_initialize(pf_handle* h, const double* mean, const double* cov, const double* replay_normals);

/* predict (pf.py:223-237): x <- g(x, u) + chol(Q) n.  u [R][nx] or NULL;
 * replay_normals [R][N][nx] or NULL. */
pf_status pf_predict(pf_handle* h, const double* u, const double* replay_normals);

/* update, weighting half (pf.py:253-264 up to the resample decision).
 * z [R][nz]; info [R] out (nullable); mean [R][nx], cov [R][nx][nx] out (nullable):
 * the weighted posterior (the reported state when no resample happens). */
pf_status pf_update(pf_handle* h, const double* z, pf_update_info* info, double* mean, double* cov);

/* _resample, applying half (pf.py:204-218): replicates whose last update decided to
 * resample get their ancestors gathered (+ jitter); weights become uniform.
 * uniforms: NULL (device Philox) or [R] systematic U / [R][N] multinomial u;
 * jitter_normals [R][N][nx] or NULL.  mean/cov out (nullable): uniform-weight
 * statistics of the resampled set (pf.py:266-267), written for resampled replicates. */
pf_status pf_resample(pf_handle* h, const double* uniforms, const double* jitter_normals, double* mean,
                      double* cov);

/* Force a resample of the current (set_state) particles with their weights, whatever
 * Neff is: the applying half of ParticleFilter._resample(particles, weights) once the
 * caller has made the Neff test itself (pf.py:203-218).  uniforms / jitter as in
 * pf_resample (NULL = device Philox). */
pf_status pf_resample_state(pf_handle* h, const double* uniforms, const double* jitter_normals);

/* The device-resident T loop: for t in [0,T): step(Z[t], U[t]) — or update(Z[0]) first
 * when first_update_only (notebook driver, PF_VS_experiments.ipynb cell 7) — with no
 * host synchronisation inside T.  Z [T][R][nz]; U [T][R][nx] or NULL.
 * Outputs (host, nullable): means [T][R][nx] (post-resample when resampled, as the
 * reference's PFState.mean), covs [T][R][nx][nx] (any nx: the step records carry them for nx <= 4,
 * the device-loop covariance kernels of pf_cov.h for larger states), neff [T][R] (pre-resample),
 * flags [T][R], log_norm [T][R]. */
pf_status pf_run(pf_handle* h, const double* Z, const double* U, int64_t T, int32_t first_update_only,
                 double* means, double* covs, double* neff, uint8_t* flags, double* log_norm);

/* Same, with every array already in device memory (HBM-resident inputs and outputs;
 * Z/U in the engine precision).  No host copies, no synchronisation: returns after
 * enqueueing on the handle's stream.  flags are int32 [T][R]. */
pf_status pf_run_device(pf_handle* h, const void* dZ, const void* dU, int64_t T, int32_t first_update_only,
                        double* d_means, double* d_covs, double* d_neff, int32_t* d_flags,
                        double* d_log_norm);

/* State readout / injection.  particles [R][N][nx] (AoS like PFState.particles);
 * log_weights [R][N] normalised (log w); weights [R][N]. */
pf_status pf_get_particles(pf_handle* h, double* particles);
pf_status pf_get_weights(pf_handle* h, double* weights, double* log_weights);
pf_status pf_set_state(pf_handle* h, const double* particles, const double* weights);
int32_t pf_weights_uniform(pf_handle* h);

/* Philox position of the handle (SURVEY.md §5 checkpoint/resume; the reference's counterpart is
 * the NumPy Generator state behind self.rng, pf.py:100-101).  The next predict draws at `epoch`,
 * the next update reserves epoch + 1 for its resample; `ep_res` is the epoch of the resample the
 * last update decided (pending = 1 while it is not yet applied).  pf_set_rng_state moves the
 * handle to a position (seed = Philox key, replicate_base = counter word of replicate 0);
 * `pending` is ignored on set. */
typedef struct pf_rng_state {
  uint64_t seed;
  uint32_t epoch;
  uint32_t ep_res;
  int32_t replicate_base;
  int32_t pending;
} pf_rng_state;
pf_status pf_get_rng_state(pf_handle* h, pf_rng_state* out);
pf_status pf_set_rng_state(pf_handle* h, const pf_rng_state* in);

/* Bit-exact checkpoint / resume of the whole filter state at a step boundary (a decided
 * resample is applied first): particles and UNNORMALISED log-weights in the engine precision,
 * the tile records, the systematic-CDF prefix, the resident kernel's entry header and the
 * Philox position.  Restoring into a handle created with the same model and options (shape,
 * Np, replicates, precision, resample method) continues bitwise as the original would have.
 * The blob is opaque host memory of pf_checkpoint_bytes(h) bytes. */
int64_t pf_checkpoint_bytes(pf_handle* h);
pf_status pf_checkpoint(pf_handle* h, void* buf, int64_t nbytes);
pf_status pf_restore(pf_handle* h, const void* buf, int64_t nbytes);

/* Weighted mean/cov of the current state, exact two-pass (np.average / np.cov
 * aweights, bias=True; pf.py:266-267), any nx.  mean [R][nx], cov [R][nx][nx]. */
pf_status pf_moments(pf_handle* h, double* mean, double* cov);

/* Standalone resampling of caller weights (pf.py:146-186 _systematic_resample /
 * _multinomial_resample).  w [N] normalised; method PF_RESAMPLE_*; systematic uses U,
 * multinomial uses uniforms [N].  idx [N] int64 out. */
pf_status pf_resample_indices(int32_t device, int32_t method, const double* w, int64_t N, double U,
                              const double* uniforms, int64_t* idx);

/* Measurement hooks for bench.py: the handle's HIP stream (hipStream_t as void*),
 * synchronisation, and per-launch device durations of `steps` step-kernels timed
 * with HIP events on that stream (ms_out [steps]). */
void* pf_stream(pf_handle* h);
pf_status pf_synchronize(pf_handle* h);
pf_status pf_profile_steps(pf_handle* h, const void* dZ, int64_t steps, float* ms_out);
/* 1 if the last pf_run / pf_run_device ran as the register-resident whole-run
 * kernel (one launch for all T steps: scalar fp32 models, systematic resampling,
 * grid co-resident), 0 if as the launch-per-step loop.  PF_RESIDENT=0 in the
 * environment forces the launch-per-step loop. */
int32_t pf_last_run_resident(pf_handle* h);
/* 1 if that resident run took the reducer form: one workgroup more per replicate
 * reduces each step's records once and the others verify from its summary (used
 * when the larger grid still fits co-resident).  PF_RES_REDUCER=0 in the
 * environment forces the form in which every workgroup reduces all records. */
int32_t pf_last_run_reducer(pf_handle* h);
/* Uninitialised-LDS test hooks (tests/test_gpu_lds_poison.py; no reference counterpart):
 * pf_test_lds_poison fills the whole 160 KB of LDS of every CU with 0xFFFFFFFF (NaN in fp32 and
 * fp64) on `stream` (a hipStream_t); with PF_TEST_HOOKS=1 and PF_TEST_LDS_POISON=1 in the
 * environment the engine does the same before every launch of its LDS-staging step, flow, EKF and
 * covariance kernels.  pf_test_lds_probe launches pf_test_lds_probe_blocks() workgroups that count
 * the words of their uninitialised LDS not holding that pattern (out [blocks], waits). */
pf_status pf_test_lds_poison(void* stream);
int32_t pf_test_lds_probe_blocks(void);
int64_t pf_test_lds_poison_count(void);  /* poison launches the engine's hook has made so far */
pf_status pf_test_lds_probe(void* stream, int32_t* out);
/* The wave and row reductions of the DPP network on given lanes (tests/test_gpu_dpp_reduce.py; no
 * reference counterpart): `ncases` cases of 64 lanes each, in_f [ncases][64] fp32 and in_d
 * [ncases][64] fp64 (host pointers), one 64-lane workgroup per case on `stream`; waits.
 * out_f [ncases][133]: the wave's fp32 maximum, its fp32 sum, the three interleaved fp32 sums of
 * the products v * 0.7f, -v * 1.3f and v * 3 (first stage fused: fma(a, b, partner's rounded
 * product)), then every lane's row maximum [64] and row sum [64].
 * out_d [ncases][66]: the wave's fp64 sum and maximum, then every lane's row sum [64]. */
pf_status pf_test_wave_reduce(void* stream, int32_t ncases, const float* in_f, const double* in_d, float* out_f,
                              double* out_d);
/* Live kernel timing for the bench: when on, every pf_run_device records HIP events on
 * the handle's stream right before its first and after its last filter kernel;
 * pf_last_run_ms waits for the last run and returns the device time between them. */
pf_status pf_set_timing(pf_handle* h, int32_t on);
pf_status pf_last_run_ms(pf_handle* h, float* ms);
/* Verification trace of the register-resident kernel (tests; the shipped kernel instance is not
 * touched: a second instance with the trace stores runs while a trace is set).  pf_set_trace
 * allocates room for T_cap steps (0 frees it).  While set, every resident run records, for each
 * of its first T_cap steps, the state its verification accepted - after any rollback and
 * recomputation inside the launch: the predicted particles and pre-resample log-weights (fp32,
 * any uniform frame), and on a resample step the ancestor index of every output slot (-1
 * elsewhere).  pf_get_trace copies step t (of the last run) of replicate r: x, l, anc [N]
 * (nullable), and resets that step's ancestors to -1; PF_E_ARG when the last run did not execute
 * as the resident kernel (a launch-per-step run records no trace). */
pf_status pf_set_trace(pf_handle* h, int64_t T_cap);
pf_status pf_get_trace(pf_handle* h, int64_t t, int32_t r, float* x, float* l, int32_t* anc);
/* Geometry of the step launch: tiles per replicate, tile size, dynamic LDS bytes. */
pf_status pf_geometry(pf_handle* h, int32_t* G, int32_t* tile, int32_t* lds_bytes);

/* ---- Sinkhorn optimal-transport resampling (models/DPF_OT_resampling.py, cited "ot.py:LINE") ----
 * sinkhorn_ot_resample (ot.py:71-234) for `batch` independent problems of n_particles particles in
 * dim dimensions: the cost matrix, the 2 n_iters log-sum-exp passes of the dual iteration with the
 * reference's stopping rule decided on the device, and the barycentric projection.  Arithmetic is
 * fp64 (the reference casts to float32).  No floating-point atomics: two calls on the same input
 * give bitwise equal output, and problem b of a batch equals the same problem solved alone.
 * pf_ot_backward is the backward pass with respect to X and w.  The Python mirror is
 * particle_filters_amd/dpf_ot.py. */
typedef struct pf_ot_opts {
  int64_t n_particles; /* N >= 1 */
  int32_t dim;         /* 1 <= d <= 1024 */
  int32_t batch;       /* B >= 1 (at most 65535) */
  int32_t device;
} pf_ot_opts;

typedef struct pf_ot_handle pf_ot_handle;

/* The handle owns B N Npad doubles for the cost matrices (Npad = N rounded up to 64); a failed
 * allocation is PF_E_HIP with the requested size in the message.  PF_E_ARG for a null pointer,
 * n_particles < 1, dim outside 1..1024 or batch < 1 - checked before any device is touched. */
pf_status pf_ot_create(const pf_ot_opts* opts, pf_ot_handle** out);
void pf_ot_destroy(pf_ot_handle* h);

/* One resampling (ot.py:119-204) as a stream-ordered sequence of launches; the call returns after
 * the results have reached the host.
 *   X [B][N][d] particles, w [B][N] weights (floored at min_val and divided by sum + min_val here),
 *   epsilon > 0, n_iters >= 0 (0 gives the plan at f = g = 0), tol the stopping tolerance
 *   (ot.py:169-181; 0 runs every iteration).
 *   X_out [B][N][d] = (P^T X) / b; the new weights are 1 / N.
 *   iterations (nullable) [B]: iterations run, the reference's actual_iterations;
 *   history (nullable) [B][n_iters][2]: (max|f - f_old|, max|g - g_old|) of iteration it (0-based)
 *     for 1 <= it < iterations[b], zero elsewhere;
 *   f, g (nullable) [B][N]: the dual variables of the stopping iteration;
 *   plan_stats (nullable) [B][2]: sum_ij P_ij C_ij and the number of entries P_ij > 1e-6.
 * The iterations are enqueued in chunks (PF_OT_POLL in the environment, read at every call,
 * default 16) between which the host reads the B done flags; the result does not depend on the
 * chunk length. */
pf_status pf_ot_resample(pf_ot_handle* h, const double* X, const double* w, double epsilon, int32_t n_iters,
                         double min_val, double tol, double* X_out, int32_t* iterations, double* history, double* f,
                         double* g, double* plan_stats);

/* The backward pass of pf_ot_resample with respect to X and w at the same (X, w, epsilon, min_val):
 * the derivative of the unrolled damped loop (ot.py:146-181) run for iterations[b] iterations in
 * problem b - the stopping rule is control flow - through the plan and projection (ot.py:184-201),
 * the cost (ot.py:25-31) and the weight normalisation (ot.py:127-128); every maximum passes its
 * gradient where its first argument is the larger.  Not the implicit derivative at the fixed point.
 *   iterations [B]: what pf_ot_resample returned, each in 0 .. k_cap;
 *   hist [B][4][k_cap + 1][N], hist_argmax [B][k_cap][N] (nullable together; hist_argmax may be
 *   null when k_cap = 0): the dual history pf_ot_replay returned for these arguments - f^k, g^k,
 *   Tau_f^k, Tau_g^k for k = 0 .. iterations[b] (f^0 = g^0 = 0), and per column of the g pass of
 *   iteration k (row k - 1) the index of the maximum where the floor inside Tau bound, -1 elsewhere.
 *   Null: the call replays the iterations itself first;
 *   grad_X_out [B][N][d], the gradient of a scalar with respect to X_out;
 *   grad_X [B][N][d], grad_w [B][N] out.  grad_w is exactly 0 where w <= min_val.
 * The first call (or pf_ot_replay) allocates a second B N Npad doubles, the gradient with respect
 * to the cost matrix, and the history of 4 (k_cap + 1) Npad doubles and k_cap Npad int32 per
 * problem (PF_E_HIP with the size if that fails).  No floating-point atomics: bitwise repeatable, in
 * a batch or alone, with a history or without.  PF_E_ARG for a null pointer, epsilon <= 0, k_cap
 * outside 0 .. 2^24, iterations[b] outside 0 .. k_cap, or one of hist / hist_argmax alone. */
pf_status pf_ot_backward(pf_ot_handle* h, const double* X, const double* w, double epsilon, double min_val,
                         const int32_t* iterations, int32_t k_cap, const double* hist, const int32_t* hist_argmax,
                         const double* grad_X_out, double* grad_X, double* grad_w);

/* The dual history pf_ot_backward needs: exactly iterations[b] iterations of problem b again, with no
 * check, recorded into hist and hist_argmax (layouts above; rows past iterations[b] are 0 and -1).
 * The iterates are those of pf_ot_resample.  hist_argmax may be null when k_cap = 0. */
pf_status pf_ot_replay(pf_ot_handle* h, const double* X, const double* w, double epsilon, double min_val,
                       const int32_t* iterations, int32_t k_cap, double* hist, int32_t* hist_argmax);

/* The handle's hipStream_t (as void*), for event timing; and a wait for it and for the handle's
 * latest entry, on whichever stream that ran. */
void* pf_ot_stream(pf_ot_handle* h);
pf_status pf_ot_synchronize(pf_ot_handle* h);

/* ---- Soft (Gumbel-Softmax) resampling (models/DPF_soft_resampling.py, cited "soft.py:LINE") ----
 * The resampling of DifferentiableParticleFilter.step (soft.py:309-334) for `batch` independent
 * problems: with log_probs_j = log q_j and independent Gumbel draws G_ij,
 *   z_ij = (log_probs_j + G_ij) / T,  a_ij = softmax_j(z_ij),  X'_i = sum_j a_ij X_j,
 * and on request the row entropies H_i = -sum_j a_ij log(a_ij + 1e-10) (soft.py:348-350).  The
 * N x N matrix and its draws are never stored.  Arithmetic is fp64.  pf_soft_backward is the
 * backward pass with respect to X and log_probs.
 *
 * The draws.  The uniform of output row i, source j, problem b is Philox4x32-10 with key
 * (lo32(seed), hi32(seed)) at the counter (j >> 1, i, epoch, 5 + 256 (batch_base + b)); an even j
 * takes the words (x, y), an odd j (z, w), as (hi, lo); m = ((hi >> 6) << 26) | (lo >> 6) and
 * u = (2 m + 1) 2^-53, exact in fp64 and strictly inside (0, 1); G = -log(-log(u)).  A draw does
 * not depend on N, d or the batch size.
 *
 * No floating-point atomics: two calls on the same input give bitwise equal output, problem b of a
 * batch equals the same problem solved alone with batch_base = b, and X_out does not depend on
 * whether row_entropy is requested.  The Python mirror is particle_filters_amd/dpf_soft.py. */
typedef struct pf_soft_opts {
  int64_t n_particles; /* N >= 1 */
  int32_t dim;         /* 1 <= d <= 1024 */
  int32_t batch;       /* B >= 1 (at most 65535) */
  int32_t device;
} pf_soft_opts;

typedef struct pf_soft_handle pf_soft_handle;

/* PF_E_ARG for a null pointer, n_particles < 1, dim outside 1..1024 or batch outside 1..65535 -
 * checked before any device is touched.  The handle owns B S d Npad doubles of partial sums (S <= 64
 * source splits, Npad = N rounded up to 64); a failed allocation is PF_E_HIP with the size in the
 * message. */
pf_status pf_soft_create(const pf_soft_opts* opts, pf_soft_handle** out);
void pf_soft_destroy(pf_soft_handle* h);

/* One resampling; the call returns after the results have reached the host.
 *   X [B][N][d] particles, log_probs [B][N] (need not be normalised), temperature > 0,
 *   X_out [B][N][d]; row_entropy (nullable) [B][N].
 * PF_E_ARG for a null handle, X, log_probs or X_out, a temperature that is not positive and finite,
 * or batch_base + B > 2^24. */
pf_status pf_soft_resample(pf_soft_handle* h, const double* X, const double* log_probs, double temperature,
                           uint64_t seed, uint32_t epoch, uint32_t batch_base, double* X_out,
                           double* row_entropy);

/* The row statistics of the handle's latest forward pass, which a backward pass needs beside X_out:
 * row_max, row_sum [B][N], M_i = max_j z_ij and L_i = sum_j exp(z_ij - M_i).  PF_E_ARG for a null
 * pointer, or if no forward pass has completed on the handle yet (a pf_soft_backward that was called
 * without saved results ran one). */
pf_status pf_soft_row_stats(pf_soft_handle* h, double* row_max, double* row_sum);

/* The backward pass of pf_soft_resample at the same (X, log_probs, temperature, seed, epoch,
 * batch_base): given grad_X_out [B][N][d], the gradient of a scalar with respect to X_out,
 *   grad_X_j = sum_i a_ij grad_X_out_i                                          [B][N][d],
 *   grad_log_probs_j = (X_j . grad_X_j - sum_i a_ij (grad_X_out_i . X_out_i)) / T   [B][N];
 * there is no gradient with respect to the temperature.  The matrix is regenerated from the same
 * Philox counters as in the forward pass, one more all-pairs pass, and never stored.
 *   X_out [B][N][d], row_max, row_sum [B][N]: what pf_soft_resample and pf_soft_row_stats returned
 *   for these arguments - all three, or all three null, in which case the call runs the forward
 *   launches itself first.  Row statistics that an earlier call left in the handle are never read, so
 *   backward calls may come in any order after their forward calls.
 * PF_E_ARG as for pf_soft_resample, for a null grad_X_out, grad_X or grad_log_probs, and for one or
 * two of the three saved results.  The first call allocates B S (d + 1) Npad doubles of partial sums
 * (PF_E_HIP if that fails).  Bitwise repeatable, in a batch or alone, with saved results or without. */
pf_status pf_soft_backward(pf_soft_handle* h, const double* X, const double* log_probs, double temperature,
                           uint64_t seed, uint32_t epoch, uint32_t batch_base, const double* X_out,
                           const double* row_max, const double* row_sum, const double* grad_X_out, double* grad_X,
                           double* grad_log_probs);

/* The draws the kernels of pf_soft_resample use, for inspection and tests: U, G [B][N][N], either
 * nullable (not both).  PF_E_ARG also when B N N > 2^31. */
pf_status pf_soft_draws(pf_soft_handle* h, uint64_t seed, uint32_t epoch, uint32_t batch_base, double* U,
                        double* G);

/* The handle's hipStream_t (as void*), for event timing; and a wait for it and for the handle's
 * latest entry, on whichever stream that ran. */
void* pf_soft_stream(pf_soft_handle* h);
pf_status pf_soft_synchronize(pf_soft_handle* h);

/* ---- RNN resampling (models/DPF_RNN_resampling.py, cited "rnn.py:LINE") ----
 * The resampling of DifferentiableParticleFilterRNN.step (rnn.py:263-349) for `batch` independent
 * problems.  For each new particle i a fresh `layers`-layer LSTM / GRU of `hidden` units runs over
 * the old particles j = 0..N-1 with the input [w_j (use_weight), x_j (use_particle), onehot_N(i)];
 * the top layer's last hidden state h_i gives logits_i = h_i Kd + bd, A_i = softmax(logits_i / T)
 * and X'_i = sum_j A_ij X_j.  Keras cell conventions: LSTMCell with gate order i, f, c, o; GRUCell
 * with reset_after = True, gate order z, r, h and a bias of shape (2, 3 H).  Arithmetic is fp64;
 * pf_rnn_backward is the backward pass.  The recurrence is one launch whatever N is; its weights stay in LDS when they
 * fit (hidden <= 32 with layers <= 2, hidden = 64 with one layer, among others) and are streamed
 * through L2 otherwise.  The forward pass has no buffer of batch x N^2 x hidden elements.
 *
 * No floating-point atomics: two calls on the same input give bitwise equal output, and problem b of
 * a batch equals the same problem solved alone.  The Python mirror is
 * particle_filters_amd/dpf_rnn.py. */
typedef struct pf_rnn_opts {
  int64_t n_particles; /* N >= 1, batch x N^2 <= 2^28 */
  int32_t dim;         /* 1 <= d <= 1024 */
  int32_t batch;       /* 1 <= B <= 65535 */
  int32_t hidden;      /* 1 <= H <= 128 */
  int32_t layers;      /* 1 <= L <= 4 */
  int32_t cell;        /* 0 lstm, 1 gru */
  int32_t use_weight;  /* the weight w_j is an input feature */
  int32_t use_particle; /* the state x_j is an input feature; at least one of the two */
  int32_t device;
} pf_rnn_opts;

typedef struct pf_rnn_handle pf_rnn_handle;

/* PF_E_ARG, with a message naming the field, for a null pointer or a field outside the limits
 * above - checked before any device is touched.  The handle owns batch x N^2 doubles for the
 * assignment matrices; a failed allocation is PF_E_HIP with the size in the message. */
pf_status pf_rnn_create(const pf_rnn_opts* opts, pf_rnn_handle** out);
void pf_rnn_destroy(pf_rnn_handle* h);

/* The network, as the n = 3 L + 2 arrays of Keras' get_weights() (row-major, sizes[k] elements):
 * per layer kernel [in][G H], recurrent_kernel [H][G H], bias ([4 H] for the LSTM, [2][3 H] for the
 * GRU), with G = 4 or 3 and in = F0 + N for layer 0 (F0 = use_weight + use_particle x d), H above;
 * then the output layer's kernel [H][N] and bias [N].  PF_E_ARG for a wrong count or size. */
pf_status pf_rnn_set_weights(pf_rnn_handle* h, const double* const* arrays, const int64_t* sizes, int32_t n);

/* One resampling; the call returns after the results have reached the host.
 *   X [B][N][d] particles, w [B][N] the normalised weights exp(log w) (read only with use_weight),
 *   temperature > 0; X_out [B][N][d]; A_out (nullable) [B][N][N] the assignment matrices;
 *   hid_out (nullable) [B][N][H] the last hidden states of the top layer.
 * PF_E_ARG for a null h, X, w or X_out, a temperature that is not positive and finite, or weights
 * that were never set. */
pf_status pf_rnn_resample(pf_rnn_handle* h, const double* X, const double* w, double temperature, double* X_out,
                          double* A_out, double* hid_out);

/* The baseline resampler (rnn.py:217-261): A_ij = softmax_j(lp_j + 0.1 G_ij), X'_i = sum_j A_ij X_j,
 * with lp [B][N] formed by the caller (log(w_j + 1e-10) / temperature) and G_ij the Gumbel draws of
 * pf_soft_resample at the same (seed, epoch, batch_base): pf_soft_draws reproduces them.  Needs no
 * weights.  A_out is nullable.  PF_E_ARG also when batch_base + B > 2^24. */
pf_status pf_rnn_baseline(pf_rnn_handle* h, const double* X, const double* lp, uint64_t seed, uint32_t epoch,
                          uint32_t batch_base, double* X_out, double* A_out);

/* The backward pass of pf_rnn_resample: the gradients of  sum grad_X_out . X_out + sum grad_A . A  at
 * the same (X, w, temperature) and the handle's current weights.
 *   grad_X_out [B][N][d]; grad_A (nullable: taken as 0) [B][N][N];
 *   grad_X [B][N][d]; grad_w [B][N], the gradient to the weights w (zeros when use_weight = 0);
 *   grad_arrays: n = 3 L + 2 arrays in the layouts of pf_rnn_set_weights with their sizes, each the sum
 *   over the B problems of the per-problem gradient, added in ascending b on the device.
 * The call runs the forward launches itself, recording the hidden and cell states of every
 * (problem, new particle, timestep, layer), and reads nothing an earlier call left in the handle, so
 * backward calls may come in any order.  The first call allocates a workspace of
 * pf_rnn_backward_bytes(h) bytes, which grows as B N^2 L hidden; a failed allocation is PF_E_HIP with
 * the size in the message.  A handle that only runs forward allocates nothing of it.  There is no
 * gradient for the temperature and no backward pass of pf_rnn_baseline.  No floating-point atomics:
 * the bitwise properties of pf_rnn_resample hold.  PF_E_ARG for a null pointer other than grad_A, a
 * temperature that is not positive and finite, weights that were never set, or a wrong n or size. */
pf_status pf_rnn_backward(pf_rnn_handle* h, const double* X, const double* w, double temperature,
                          const double* grad_X_out, const double* grad_A, double* grad_X, double* grad_w,
                          double* const* grad_arrays, const int64_t* sizes, int32_t n);
int64_t pf_rnn_backward_bytes(pf_rnn_handle* h);

/* 1 when the handle's recurrence keeps its weights in LDS, 0 when it streams them (or h is null). */
int32_t pf_rnn_resident(pf_rnn_handle* h);

/* The handle's hipStream_t (as void*), for event timing; and a wait for it and for the handle's
 * latest entry, on whichever stream that ran. */
void* pf_rnn_stream(pf_rnn_handle* h);
pf_status pf_rnn_synchronize(pf_rnn_handle* h);

/* ---- Device-pointer entries of the soft and the RNN resampler ----
 * pf_soft_resample / pf_soft_backward / pf_rnn_set_weights / pf_rnn_resample / pf_rnn_backward for
 * callers whose data is on the GPU already.  Every d* pointer is device memory on the handle's
 * device, in the layout of the host entry's argument of the same name, at least 8-byte aligned (the
 * kernels use scalar loads and stores only).  Inputs are read where they lie, outputs are written
 * where the caller points; results are bitwise those of the host entries on the same bits.
 *
 *   stream: a hipStream_t of the handle's device (as void*).  Non-null: all work is enqueued on it and
 *   the entry returns without synchronising (the first backward of a handle allocates its workspace,
 *   which may wait for the device).  Null: the handle's own stream, and the entry synchronises before
 *   it returns.
 *
 *   Order across entries.  A handle's scratch is shared by its entries, so every entry, host or
 *   device, waits (on its stream, not on the host) for the handle's previous entry before its first
 *   launch: a _dev call on stream S followed by a host entry on the same handle is correct without a
 *   synchronisation by the caller.  pf_x_synchronize and pf_x_destroy wait for the latest entry, so a
 *   handle may be destroyed straight after an asynchronous call.  Two threads must not call into one
 *   handle at the same time.
 *
 *   Aliasing.  No output may overlap an input of the same call (dX_out == dX, say): PF_E_ARG, decided
 *   from the pointers and sizes.
 *
 * Otherwise the checks, messages and statuses are the host entries'.  pf_soft_resample_dev writes the
 * row statistics M_i, L_i (pf_soft_row_stats) to d_row_max, d_row_sum [B][N] when both are given;
 * pf_soft_backward_dev takes them back with dX_out, all three or none.  d_arrays / d_grad_arrays are
 * host arrays of n device pointers. */
pf_status pf_soft_resample_dev(pf_soft_handle* h, void* stream, const double* dX, const double* d_log_probs,
                               double temperature, uint64_t seed, uint32_t epoch, uint32_t batch_base,
                               double* dX_out, double* d_row_entropy, double* d_row_max, double* d_row_sum);
pf_status pf_soft_backward_dev(pf_soft_handle* h, void* stream, const double* dX, const double* d_log_probs,
                               double temperature, uint64_t seed, uint32_t epoch, uint32_t batch_base,
                               const double* dX_out, const double* d_row_max, const double* d_row_sum,
                               const double* d_grad_X_out, double* d_grad_X, double* d_grad_log_probs);
pf_status pf_rnn_set_weights_dev(pf_rnn_handle* h, void* stream, const double* const* d_arrays, const int64_t* sizes,
                                 int32_t n);
pf_status pf_rnn_resample_dev(pf_rnn_handle* h, void* stream, const double* dX, const double* dw, double temperature,
                              double* dX_out, double* dA, double* d_hid);
pf_status pf_rnn_backward_dev(pf_rnn_handle* h, void* stream, const double* dX, const double* dw, double temperature,
                              const double* d_grad_X_out, const double* d_grad_A, double* d_grad_X, double* d_grad_w,
                              double* const* d_grad_arrays, const int64_t* sizes, int32_t n);

/* ---- Device-pointer entries of the OT resampler ----
 * pf_ot_resample / pf_ot_backward under the conventions of the block above: device pointers in the
 * layouts of the host arguments of the same names (d_iterations and d_hist_argmax int32, 4-byte
 * aligned), the stream, the order across entries (the handle's fence, which its host entries,
 * pf_ot_synchronize and pf_ot_destroy honour too), the aliasing rule, and otherwise the host
 * entries' checks and messages.  Results are bitwise those of the host entries on the same bits.
 *
 * pf_ot_resample_dev.  With a caller's stream nothing is read back: all n_iters iterations are
 * enqueued, and a done problem's launches return at entry (with a null stream the entry polls the done
 * flags as pf_ot_resample does).  dX_out is required; d_iterations [B], d_history [B][n_iters][2],
 * d_f, d_g [B][N] and d_plan_stats [B][2] are nullable.  Without d_history the changes go to a buffer
 * of the handle, which grows (and waits for the device) when n_iters does.
 *   d_hist [B][4][n_iters + 1][N] and d_hist_argmax [B][n_iters][N], together or not at all
 *   (d_hist_argmax may be null when n_iters = 0): the forward pass records its own dual history,
 *   pf_ot_replay's layout with k_cap = n_iters and bitwise its values; the entry writes every
 *   element, the rows past a problem's stopping iteration as 0 and -1.
 *   flags: 0, the launch sequence, or PF_OT_RESIDENT, the one-launch solver for N <= 128: one workgroup
 *   per problem runs the whole resampling with the cost matrix in LDS - the weight normalisation, the
 *   cost, the iterations with the stopping rule decided in the kernel, the histories, the plan, its
 *   statistics and the projection - and writes the same outputs in the same layouts.  Its sums run in
 *   a fixed order of their own: two calls are bitwise equal and problem b of a batch is bitwise that
 *   problem alone, but the results agree with the launch sequence's to rounding, not bitwise.
 *   PF_OT_RESIDENT on a handle for which pf_ot_resident_supported is 0 is PF_E_ARG: there is no
 *   fallback.  pf_ot_backward_dev takes a history recorded by either solver.
 *
 * pf_ot_backward_dev.  The iteration counts stay on the device, so the host cannot know the largest:
 * it enqueues the reverse sweep for k = k_sweep .. 1.  k_cap is the layout of the history; k_sweep, in
 * 1 .. k_cap (0 when k_cap = 0), is the caller's promise that no problem took more iterations, and a
 * caller that knows nothing passes k_cap.  A count outside 0 .. k_sweep is used as if clamped to that
 * range: no kernel reads the history outside the iterations 0 .. k_sweep.  d_hist and d_hist_argmax
 * are a history recorded by pf_ot_resample_dev (or pf_ot_replay's, copied to the device); null
 * together: the call replays first, k_sweep iterations enqueued, gated by the counts.  The first
 * backward call of a handle allocates its workspace and may wait for the device.  PF_E_ARG also
 * for a k_sweep outside its range. */
#define PF_OT_RESIDENT 1
/* 1 when PF_OT_RESIDENT is available on the handle (N <= 128: the problem fits one CU's LDS), else 0. */
int32_t pf_ot_resident_supported(pf_ot_handle* h);
pf_status pf_ot_resample_dev(pf_ot_handle* h, void* stream, const double* dX, const double* dw, double epsilon,
                             int32_t n_iters, double min_val, double tol, int32_t flags, double* dX_out,
                             int32_t* d_iterations, double* d_history, double* d_f, double* d_g, double* d_plan_stats,
                             double* d_hist, int32_t* d_hist_argmax);
pf_status pf_ot_backward_dev(pf_ot_handle* h, void* stream, const double* dX, const double* dw, double epsilon,
                             double min_val, const int32_t* d_iterations, int32_t k_cap, int32_t k_sweep,
                             const double* d_hist, const int32_t* d_hist_argmax, const double* d_grad_X_out,
                             double* d_grad_X, double* d_grad_w);

#ifdef __cplusplus
}
#endif
#endif /* PF_ENGINE_H */
