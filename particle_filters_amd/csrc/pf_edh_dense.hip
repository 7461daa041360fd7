// Host side of the dense EDH particle-flow path: the pf_edh_dense_* entries of include/pf_edh.h.
//
// One step is a stream-ordered sequence of launches of pf_edh_dense_kernels.h: the composed map
// applied to eta_0 (G_MAP), the two whitened quadratic forms (G_QX, G_QV), the log-weights, their
// normalisation with the ESS and the resample decision, then (finish) the CDF, the ancestor gather
// and the weighted moments.  The decision stays on the device, so pf_edh_dense_run enqueues all T
// steps without waiting for the host.
//
// The dense LEDH flow (pf_ledh_dense_*) replaces the map by the per-particle flow kernel of
// pf_ledh_dense_kernels.h, launched in chunks of particles (pf_ledh_dense_plan.h), and adds its
// log-determinant term theta to the log-weights; everything after the flow is the same sequence.
//
// pf_edh_dense_flow_* compose the EDH map itself on the device (pf_edh_flowmap_kernels.h) into the
// handle's M / c and then run the sequence of pf_edh_dense_step on it.
//
// pf_ukf_dense_* is the UKF tracker of these flows with its state on the device (pf_ukf_dense_kernels.h);
// pf_edh_dense_flow_run_tracked chains its predict and update into the steps of pf_edh_dense_flow_run on
// the filter handle's stream, so a run has no host work inside T.
//
// PF_NOISE_DEVICE (pf_edh_dense_set_noise) draws a step's process noise on the device
// (pf_noise_dense_kernels.h) into the buffer an uploaded v would fill, ahead of the step on the same stream;
// pf_edh_dense_init_gaussian draws the initial particles with the same kernel.
//
// The four step entries and the four run entries are straight-line callers of the same pieces.  A step:
// its preconditions (flow_check, step_ready), upload_step, its own enqueue_* sequence, download_step, its
// own verdict on the flow's flag, commit_step.  A run: check_T, run_ready, a RunFrame (the run's device
// temporaries with their upload, per-step pointers, download and dead-weight verdict), and in between the
// entry's own loop body and failure message.  What differs between the paths (when has_map is set, what
// a failure restores or names) is written in the entries, not behind options of the shared pieces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pf_edh.h"
#include "pf_edh_dense_kernels.h"
#include "pf_edh_flowmap_kernels.h"
#include "pf_hooks.h"
#include "pf_host.h"
#include "pf_ledh_dense_kernels.h"
#include "pf_ledh_dense_plan.h"
#include "pf_noise_dense_kernels.h"
#include "pf_ukf_dense_kernels.h"
#include "pf_ukf_dense_plan.h"

using namespace pf::edh_dense;
using pf::DevBuf;
using pf::fail;

namespace {
constexpr int MAXDIM = 1024;
constexpr int64_t MAXN = 1048576;  // the flow engines' limit (pf_ledh_create)
}  // namespace

struct pf_edh_dense_handle {
  int N = 0, d = 0, obs = 0, like = 0, device = 0;
  double alpha = 0.0, m1 = 0.0, m2 = 0.0, ratio = 0.0;
  int ctiles = 1;                // column tiles of the product kernel
  int cS = 1, cchunk = 0;        // covariance splits over the particle index
  int mS = 1, mchunk = 0;        // mean splits
  bool initialised = false, pending = false;
  int last_flag = 0;
  pf::Stream stream;  // before the buffers: destroyed after them
  DevBuf<double> X, Xn, w, wn, logw, cdf, qx, qv, M, c, z, u, v, W, rdiag, info, U, mean, cov, mpart, wpart, wsum, cpart;
  // pf_edh_dense_set_run_replay
  DevBuf<double> rpV, rpU;
  int64_t rpT = -1;
  bool rp_has_v = false;
  // the dense LEDH flow: made at its first step
  DevBuf<double> frd, theta, trace, ws;
  DevBuf<int> lfail, lnfail;
  int64_t ws_bytes = 0;
  int trace_L = 0;
  // the device-composed EDH map (pf_edh_dense_flow_*): made at its first step.  Seven d x d buffers
  // (P, the factor of S, S^-1, A, two of the G / Phi chain, the second M) and the d-vectors.
  DevBuf<double> fmP, fmW, fmSi, fmA, fmT1, fmT2, fmM2, fmv, fmeta0;
  DevBuf<int> fmfail;
  bool fm_ready = false, has_map = false;
  // device process noise: chol(Q) beside W, and the draw armed by pf_edh_dense_set_noise
  DevBuf<double> Lq;
  bool noise_armed = false;
  uint64_t nseed = 0;
  uint32_t nepoch = 0;
  ~pf_edh_dense_handle() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

namespace {

// ---- preconditions: no device is touched ----

pf_status check_T(int64_t T) { return T < 1 || T > (1 << 20) ? fail(PF_E_ARG, "T out of range") : PF_OK; }

// path: "EDH" or "LEDH"
pf_status check_noise(int32_t noise, const char* path) {
  if (noise != PF_NOISE_NONE && noise != PF_NOISE_HOST && noise != PF_NOISE_DEVICE)
    return fail(PF_E_ARG, std::string("noise must be PF_NOISE_NONE, PF_NOISE_HOST or PF_NOISE_DEVICE on the dense ") +
                              path + " path");
  return PF_OK;
}

// PF_NOISE_DEVICE draws the T epochs from the one armed by pf_edh_dense_set_noise
pf_status noise_ready(const pf_edh_dense_handle* h, int32_t noise, int64_t T) {
  if (noise != PF_NOISE_DEVICE) return PF_OK;
  if (!h->noise_armed) return fail(PF_E_ARG, "PF_NOISE_DEVICE needs pf_edh_dense_set_noise before the step or run");
  if ((uint64_t)h->nepoch + (uint64_t)T > 0xFFFFFFFFull) return fail(PF_E_ARG, "the noise epoch overflows 32 bits");
  return PF_OK;
}

// the arguments of a flow composed on the device; integrator_ok is true where the flow has no integrator
pf_status flow_check(const pf_edh_dense_handle* h, const double* R_diag, int32_t n_lambda, bool integrator_ok,
                     int32_t noise, const char* path) {
  if (n_lambda < 1 || n_lambda > (1 << 20)) return fail(PF_E_ARG, "n_lambda must be positive");
  if (!integrator_ok) return fail(PF_E_ARG, "bad integrator (PF_EDH_RK4 or PF_EDH_EULER)");
  const pf_status st = check_noise(noise, path);
  if (st != PF_OK) return st;
  for (int j = 0; j < h->d; ++j)
    if (!(R_diag[j] > 0.0) || !std::isfinite(R_diag[j])) return fail(PF_E_ARG, "R_diag must be finite and positive");
  return PF_OK;
}

bool integrator_ok(int32_t integrator) { return integrator == PF_EDH_RK4 || integrator == PF_EDH_EULER; }

// the handle holds a complete state
pf_status check_ready(const pf_edh_dense_handle* h) {
  if (!h->initialised) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  if (h->pending) return fail(PF_E_ARG, "a step is pending: call pf_edh_dense_finish first");
  return PF_OK;
}

pf_status step_ready(const pf_edh_dense_handle* h, int32_t noise, const double* v) {
  if (noise == PF_NOISE_HOST && !v) return fail(PF_E_ARG, "PF_NOISE_HOST needs v");
  const pf_status st = noise_ready(h, noise, 1);
  return st != PF_OK ? st : check_ready(h);
}

// a run needs the draws of pf_edh_dense_set_run_replay whenever it can read them
pf_status run_ready(const pf_edh_dense_handle* h, int64_t T, int32_t noise) {
  const pf_status st = check_ready(h);
  if (st != PF_OK) return st;
  if (h->rpT != T && (h->ratio > 0.0 || noise == PF_NOISE_HOST))
    return fail(PF_E_ARG, "pf_edh_dense_set_run_replay must give the draws of a run of exactly this T");
  if (noise == PF_NOISE_HOST && !h->rp_has_v) return fail(PF_E_ARG, "PF_NOISE_HOST needs the replayed V");
  return noise_ready(h, noise, T);
}

// ---- the pieces of a step ----

struct StepIn {
  const double *z, *u, *v;  // device pointers; u / v are null when absent
};

// out [N][d] = (mean +) zeta F^T on the handle's stream: zeta the Philox normals of (seed, epoch, stream),
// F [d][d] a lower Cholesky factor and mean [d] (nullable), both on the device
pf_status enqueue_noise(pf_edh_dense_handle* h, uint64_t seed, uint32_t epoch, uint32_t stream, const double* F,
                        const double* mean, double* out) {
  NoiseArgs a{h->N, h->d, seed, epoch, stream, F, mean, out};
  pf::lds_poison_hook(h->stream);  // tests only (pf_hooks.h)
  hipLaunchKernelGGL(k_dense_noise, dim3((unsigned)((h->N + TM - 1) / TM), (unsigned)h->ctiles), dim3(GB), 0, h->stream,
                     a);
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

// z, u and v of one step into the handle's buffers, on its stream; PF_NOISE_DEVICE draws v there and
// consumes the armed epoch
pf_status upload_step(pf_edh_dense_handle* h, const double* z, const double* u, int32_t noise, const double* v,
                      StepIn* in) {
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d;
  PF_HIPCHK(hipMemcpyAsync(h->z, z, d * 8, hipMemcpyHostToDevice, s));
  if (u) PF_HIPCHK(hipMemcpyAsync(h->u, u, d * 8, hipMemcpyHostToDevice, s));
  if (noise == PF_NOISE_HOST) PF_HIPCHK(hipMemcpyAsync(h->v, v, (size_t)h->N * d * 8, hipMemcpyHostToDevice, s));
  if (noise == PF_NOISE_DEVICE) {
    h->noise_armed = false;
    const pf_status st = enqueue_noise(h, h->nseed, h->nepoch, pf::STREAM_PROCESS, h->Lq, nullptr, h->v);
    if (st != PF_OK) return st;
  }
  *in = StepIn{h->z, u ? h->u.get() : nullptr, noise != PF_NOISE_NONE ? h->v.get() : nullptr};
  return PF_OK;
}

// what a step leaves for the host: info, the flow's flag (dflag nullable) and the trace [n_lambda][d]
// (nullable); waits for the stream
pf_status download_step(pf_edh_dense_handle* h, double hi[3], const int* dflag, int* flag, double* trace,
                        int n_lambda) {
  hipStream_t s = h->stream;
  PF_HIPCHK(hipMemcpyAsync(hi, h->info, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (dflag) PF_HIPCHK(hipMemcpyAsync(flag, dflag, sizeof(int), hipMemcpyDeviceToHost, s));
  if (trace) PF_HIPCHK(hipMemcpyAsync(trace, h->trace, (size_t)n_lambda * h->d * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
}

// the verdict on the weights; a live step becomes the pending one (X and w are untouched until finish)
pf_status commit_step(pf_edh_dense_handle* h, const double hi[3], pf_ledh_info* info) {
  if (hi[2] != 0.0) return fail(PF_E_NAN, "no particle has a finite positive weight");
  h->pending = true;
  h->last_flag = hi[1] != 0.0 ? 1 : 0;
  if (info) {
    info->ess = hi[0];
    info->resample = h->last_flag;
  }
  return PF_OK;
}

// what both device flows keep besides their own workspace (after hipSetDevice): the flow's R and the
// trace of n_lambda d-vectors; R_diag is uploaded on the stream
pf_status flow_prepare(pf_edh_dense_handle* h, const double* R_diag, int n_lambda, bool want_trace) {
  const size_t d = (size_t)h->d;
  if (!h->frd) PF_HIPCHK(h->frd.alloc(d));
  if (want_trace && h->trace_L < n_lambda) {
    h->trace_L = 0;
    PF_HIPCHK(h->trace.alloc((size_t)n_lambda * d));
    h->trace_L = n_lambda;
  }
  PF_HIPCHK(hipMemcpyAsync(h->frd, R_diag, d * 8, hipMemcpyHostToDevice, h->stream));
  return PF_OK;
}

// the weights of the flowed particles in Xn: the two whitened quadratic forms, the log-weights (plus
// theta for the LEDH flow), their normalisation, the ESS and the resample decision
pf_status enqueue_weights(pf_edh_dense_handle* h, const double* z, const double* u, const double* v,
                          const double* theta, double* info) {
  hipStream_t s = h->stream;
  const int N = h->N, d = h->d;
  const dim3 grid((unsigned)((N + TM - 1) / TM), (unsigned)h->ctiles);
  GemmArgs a{};
  a.N = N; a.d = d; a.alpha = h->alpha;
  a.X = h->X; a.Xn = h->Xn; a.u = u; a.v = v;
  a.B = h->W; a.c = nullptr; a.out = h->qx;
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL((k_dense_gemm<G_QX>), grid, dim3(GB), 0, s, a);
  const bool moved = u || v;  // otherwise eta_0 = g(x) and its transition term is the constant
  if (moved) {
    a.out = h->qv;
    pf::lds_poison_hook(s);
    hipLaunchKernelGGL((k_dense_gemm<G_QV>), grid, dim3(GB), 0, s, a);
  }
  LogwArgs l{};
  l.N = N; l.d = d; l.ctiles = h->ctiles; l.obs = h->obs; l.like = h->like;
  l.m1 = h->m1; l.m2 = h->m2;
  l.Xn = h->Xn; l.z = z; l.rdiag = h->rdiag; l.qx = h->qx; l.qv = moved ? h->qv.get() : nullptr;
  l.w = h->w; l.theta = theta; l.logw = h->logw;
  hipLaunchKernelGGL(k_logw, dim3((unsigned)((N + 3) / 4)), dim3(GB), 0, s, l);
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL(k_normalise, dim3(1), dim3(RB), 0, s, h->logw, h->wn, N, h->ratio, info);
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

pf_status enqueue_step(pf_edh_dense_handle* h, const double* M, const double* c, const double* z, const double* u,
                       const double* v, double* info) {
  hipStream_t s = h->stream;
  const int N = h->N, d = h->d;
  const dim3 grid((unsigned)((N + TM - 1) / TM), (unsigned)h->ctiles);
  GemmArgs a{};
  a.N = N; a.d = d; a.alpha = h->alpha;
  a.X = h->X; a.Xn = h->Xn; a.u = u; a.v = v;
  a.B = M; a.c = c; a.out = h->Xn;
  pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
  hipLaunchKernelGGL((k_dense_gemm<G_MAP>), grid, dim3(GB), 0, s, a);
  return enqueue_weights(h, z, u, v, nullptr, info);
}

// the workspace cap of the LEDH flow: PF_TEST_LEDH_WS_CAP (bytes) under PF_TEST_HOOKS, for the tests
// that force several chunks at a small shape
int64_t ledh_ws_cap() {
  const int v = pf::test_hook_int("PF_TEST_LEDH_WS_CAP");
  return v > 0 ? (int64_t)v : pf::LEDH_DENSE_WS_CAP;
}

// argument checks shared by pf_ledh_dense_step / _run: no device is touched
pf_status ledh_check(pf_edh_dense_handle* h, const double* R_diag, int32_t n_lambda, int32_t noise,
                     pf::LedhDensePlan* plan) {
  if (h->obs != OBS_EXP) return fail(PF_E_ARG, "the dense LEDH flow needs PF_EDH_OBS_EXP (an identity h is one "
                                               "affine map: compose it and use pf_edh_dense_step)");
  const pf_status st = flow_check(h, R_diag, n_lambda, true, noise, "LEDH");
  if (st != PF_OK) return st;
  if (!pf::ledh_dense_plan(h->N, h->d, ledh_ws_cap(), plan))
    return fail(PF_E_ARG, "the workspace cap does not hold one particle's factors (16 d^2 bytes)");
  return PF_OK;
}

// buffers of the LEDH flow (after hipSetDevice); R_diag is uploaded on the stream
pf_status ledh_prepare(pf_edh_dense_handle* h, const pf::LedhDensePlan& plan, const double* R_diag, int n_lambda,
                       bool want_trace) {
  const size_t N = (size_t)h->N;
  if (!h->theta) PF_HIPCHK(h->theta.alloc(N));
  if (!h->lfail) PF_HIPCHK(h->lfail.alloc(N));
  if (!h->lnfail) PF_HIPCHK(h->lnfail.alloc(1));
  if (h->ws_bytes != plan.ws_bytes) {
    h->ws_bytes = 0;
    PF_HIPCHK(h->ws.alloc((size_t)plan.ws_bytes / sizeof(double)));
    h->ws_bytes = plan.ws_bytes;
  }
  const size_t lds = pf::ledh_dense::lds_bytes(h->d);
  if (lds > 48 * 1024)
    PF_HIPCHK(hipFuncSetAttribute((const void*)pf::ledh_dense::k_ledh_flow, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds));
  return flow_prepare(h, R_diag, n_lambda, want_trace);
}

// the per-particle flow of one step into Xn / theta, chunk by chunk; nfail counts the failed particles
pf_status enqueue_flow(pf_edh_dense_handle* h, const pf::LedhDensePlan& plan, const double* P, const double* z,
                       const double* u, const double* v, int n_lambda, int* nfail, double* trace) {
  hipStream_t s = h->stream;
  PF_HIPCHK(hipMemsetAsync(nfail, 0, sizeof(int), s));
  pf::ledh_dense::FlowArgs a{};
  a.d = h->d; a.L = n_lambda;
  a.alpha = h->alpha; a.m1 = h->m1; a.m2 = h->m2;
  a.X = h->X; a.u = u; a.v = v; a.P = P; a.z = z; a.rdiag = h->frd;
  a.ws = h->ws; a.Xn = h->Xn; a.theta = h->theta; a.fail = h->lfail; a.nfail = nfail; a.trace = trace;
  const size_t lds = pf::ledh_dense::lds_bytes(h->d);
  for (int64_t first = 0; first < h->N; first += plan.chunk) {
    a.first = first;
    a.n = (int)std::min<int64_t>(plan.chunk, h->N - first);
    pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
    hipLaunchKernelGGL(pf::ledh_dense::k_ledh_flow, dim3((unsigned)a.n), dim3(pf::ledh_dense::LB), lds, s, a);
  }
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

// the workgroups of k_chol_solve: SOLVE_RHS right-hand sides each
dim3 solve_grid(int d) { return dim3((unsigned)((d + pf::ledh_dense::SOLVE_RHS - 1) / pf::ledh_dense::SOLVE_RHS)); }

// the weighted moments of X / w into mean / cov
pf_status enqueue_moments(pf_edh_dense_handle* h, double* mean, double* cov) {
  hipStream_t s = h->stream;
  const int N = h->N, d = h->d;
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL(k_mean_part, dim3((unsigned)((d + 63) / 64), (unsigned)h->mS), dim3(MB), 0, s, h->X, h->w, N, d,
                     h->mchunk, h->mpart, h->wpart);
  hipLaunchKernelGGL(k_mean_combine, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, h->mpart, h->wpart, h->mS, d,
                     mean, h->wsum);
  GemmArgs a{};
  a.N = N; a.d = d; a.X = h->X; a.w = h->w; a.mean = mean; a.out = h->cpart; a.chunk = h->cchunk;
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL((k_dense_gemm<G_COV>), dim3((unsigned)h->ctiles, (unsigned)h->ctiles, (unsigned)h->cS), dim3(GB),
                     0, s, a);
  const int64_t dd = (int64_t)d * d;
  hipLaunchKernelGGL(k_cov_combine, dim3((unsigned)((dd + 255) / 256)), dim3(256), 0, s, h->cpart, h->cS, d, h->wsum,
                     cov);
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

// resample (decision on the device) into X / w, then the weighted moments into mean / cov
pf_status enqueue_finish(pf_edh_dense_handle* h, const double* U, const double* info, double* mean, double* cov) {
  hipStream_t s = h->stream;
  const int N = h->N, d = h->d;
  pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
  hipLaunchKernelGGL(k_cdf, dim3(1), dim3(RB), 0, s, h->wn, N, info, h->cdf);
  hipLaunchKernelGGL(k_gather, dim3((unsigned)((N + 3) / 4)), dim3(GB), 0, s, h->Xn, h->wn, h->cdf, U, info, N, d,
                     h->X, h->w);
  PF_HIPCHK(hipGetLastError());
  return enqueue_moments(h, mean, cov);
}

// workspace of the device composition (after hipSetDevice); R_diag is uploaded on the stream
pf_status flowmap_prepare(pf_edh_dense_handle* h, const double* R_diag, int n_lambda, bool want_trace) {
  const size_t d = (size_t)h->d, dd = d * d;
  if (!h->fm_ready) {
    DevBuf<double>* mats[] = {&h->fmP, &h->fmW, &h->fmSi, &h->fmA, &h->fmT1, &h->fmT2, &h->fmM2};
    for (auto* m : mats) PF_HIPCHK(m->alloc(dd));
    PF_HIPCHK(h->fmv.alloc((size_t)pf::edh_flowmap::NVEC * d));
    PF_HIPCHK(h->fmeta0.alloc(d));
    PF_HIPCHK(h->fmfail.alloc(1));
    h->fm_ready = true;
  }
  return flow_prepare(h, R_diag, n_lambda, want_trace);
}

// the flow map of one step into h->M / h->c from P, etabar_0 and z (device pointers); *flag is set to 1
// on a failed pivot (the caller zeroes it); trace (nullable) [L][d] keeps etabar before each lambda step
pf_status enqueue_flowmap(pf_edh_dense_handle* h, const double* P, const double* eta0, const double* z, int L,
                          int integrator, int* flag, double* trace) {
  namespace fm = pf::edh_flowmap;
  hipStream_t s = h->stream;
  const int d = h->d;
  const size_t n = (size_t)d;
  const int64_t dd = (int64_t)d * d;
  double* vec = h->fmv;
  double *eta = vec, *etan = vec + n, *D = vec + 2 * n, *tv = vec + 3 * n, *y = vec + 4 * n, *t1 = vec + 5 * n,
         *b = vec + 6 * n, *psi = vec + 7 * n;
  // M and c alternate between two buffers; the last step writes the handle's own
  double* Mc = (L & 1) ? h->fmM2.get() : h->M.get();
  double* Mn = (L & 1) ? h->M.get() : h->fmM2.get();
  double* cc = (L & 1) ? vec + 8 * n : h->c.get();
  double* cn = (L & 1) ? h->c.get() : vec + 8 * n;
  const dim3 ew((unsigned)((dd + 255) / 256)), tiles((unsigned)h->ctiles, (unsigned)h->ctiles);
  const dim3 rows((unsigned)((d + 3) / 4));
  const size_t lds = pf::ledh_dense::solve_lds_bytes(d);
  auto gemm = [&](const double* X, const double* xD, const double* Y, const double* yD, double ys, double yI,
                  double alpha, double beta, double* out) {
    fm::MatArgs a{d, X, xD, Y, yD, ys, yI, alpha, beta, out};
    pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
    hipLaunchKernelGGL(fm::k_fm_gemm, tiles, dim3(GB), 0, s, a);
  };
  auto matvec = [&](const double* A, const double* in0, double s0, const double* in1, double s1, const double* add,
                    double ca, double* out) {
    fm::VecArgs a{d, A, in0, in1, add, ca, s0, s1, out};
    hipLaunchKernelGGL(fm::k_fm_matvec, rows, dim3(GB), 0, s, a);
  };
  hipLaunchKernelGGL(fm::k_fm_init, ew, dim3(256), 0, s, d, eta0, Mc, cc, eta);
  const double dlam = 1.0 / (double)L;
  double lam = 0.0;
  for (int step = 0; step < L; ++step) {
    lam = std::min(1.0, lam + dlam);
    hipLaunchKernelGGL(fm::k_fm_pre, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, d, h->obs, h->m1, h->m2, eta,
                       z, h->frd.get(), D, tv, trace ? trace + (size_t)step * n : nullptr);
    pf::lds_poison_hook(s);
    hipLaunchKernelGGL(fm::k_fm_chol, dim3(1), dim3(fm::LB), 0, s, d, lam, P, D, h->frd.get(), h->fmW.get(), flag);
    pf::lds_poison_hook(s);
    hipLaunchKernelGGL(pf::ledh_dense::k_chol_solve, solve_grid(d), dim3(fm::LB), lds, s, d, h->fmW.get(),
                       (const double*)nullptr, h->fmSi.get());  // S^-1
    gemm(P, D, h->fmSi, D, 1.0, 0.0, -0.5, 0.0, h->fmA);  // A
    const double* A = h->fmA;
    matvec(P, tv, 1.0, nullptr, 0.0, nullptr, 0.0, y);
    matvec(A, y, lam, eta, 1.0, y, 1.0, t1);            // (I + lam A) y + A etabar
    matvec(A, t1, 2.0 * lam, nullptr, 0.0, t1, 1.0, b);  // b
    const double* Phi = h->fmT1;
    if (integrator == PF_EDH_EULER) {
      hipLaunchKernelGGL(fm::k_fm_axpi, ew, dim3(256), 0, s, d, dlam, A, h->fmT1.get());
      matvec(nullptr, nullptr, 0.0, nullptr, 0.0, b, dlam, psi);
    } else {
      gemm(A, nullptr, A, nullptr, dlam / 4.0, 1.0, dlam / 3.0, 1.0, h->fmT1);        // I + E/3 (I + E/4)
      gemm(A, nullptr, h->fmT1, nullptr, 1.0, 0.0, dlam / 2.0, 1.0, h->fmT2);         // G
      gemm(A, nullptr, h->fmT2, nullptr, 1.0, 0.0, dlam, 1.0, h->fmT1);               // Phi = I + E G
      matvec(h->fmT2, b, dlam, nullptr, 0.0, nullptr, 0.0, psi);                      // psi = dlam G b
    }
    matvec(Phi, eta, 1.0, nullptr, 0.0, psi, 1.0, etan);
    matvec(Phi, cc, 1.0, nullptr, 0.0, psi, 1.0, cn);
    gemm(Phi, nullptr, Mc, nullptr, 1.0, 0.0, 1.0, 0.0, Mn);
    std::swap(eta, etan);
    std::swap(Mc, Mn);
    std::swap(cc, cn);
  }
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

// ---- the frame of a run ----

// The device temporaries of one run and their transfers.  A run entry begins the frame, enqueues its own
// sequence per step with the frame's per-step pointers, ends the frame and reads the verdicts.
struct RunFrame {
  pf_edh_dense_handle* h = nullptr;
  int64_t T = 0;
  size_t d = 0, dd = 0;
  bool host_noise = false, dev_noise = false, replay = false;
  uint64_t nseed = 0;   // PF_NOISE_DEVICE: step t draws with epoch nepoch + t
  uint32_t nepoch = 0;
  DevBuf<double> Z, U, A, B, means, covs, info;  // A [T][d][d], B [T][d]: the entry's own per-step inputs
  DevBuf<int> flag;                              // [T] the flow's failure flag of each step, zeroed
  std::vector<double> hi;                        // info and flag on the host (end)
  std::vector<int> hflag;

  // allocates, uploads on the stream (U, A, B nullable) and leaves the handle uninitialised: only a
  // clean verdict makes it initialised again
  pf_status begin(pf_edh_dense_handle* h_, int64_t T_, int32_t noise, const double* hZ, const double* hU,
                  const double* hA, const double* hB, bool want_flag) {
    h = h_; T = T_; d = (size_t)h->d; dd = d * d;
    host_noise = noise == PF_NOISE_HOST;
    dev_noise = noise == PF_NOISE_DEVICE;
    if (dev_noise) {  // the armed draw is consumed
      nseed = h->nseed;
      nepoch = h->nepoch;
      h->noise_armed = false;
    }
    replay = h->rpT == T;
    hipStream_t s = h->stream;
    struct { DevBuf<double>* buf; const double* src; size_t n; } in[] = {{&A, hA, dd}, {&B, hB, d}, {&Z, hZ, d}, {&U, hU, d}};
    for (auto& e : in)
      if (e.src) PF_HIPCHK(e.buf->alloc((size_t)T * e.n));
    PF_HIPCHK(means.alloc((size_t)T * d));
    PF_HIPCHK(covs.alloc((size_t)T * dd));
    PF_HIPCHK(info.alloc((size_t)T * 3));
    if (want_flag) PF_HIPCHK(flag.alloc((size_t)T));
    for (auto& e : in)
      if (e.src) PF_HIPCHK(hipMemcpyAsync(e.buf->get(), e.src, (size_t)T * e.n * 8, hipMemcpyHostToDevice, s));
    if (want_flag) PF_HIPCHK(hipMemsetAsync(flag, 0, (size_t)T * sizeof(int), s));
    h->initialised = false;
    return PF_OK;
  }

  // step t's device pointers
  const double* z(int64_t t) const { return Z + t * d; }
  const double* u(int64_t t) const { return U ? U + t * d : nullptr; }
  const double* v(int64_t t) const {
    return host_noise ? h->rpV + t * ((size_t)h->N * d) : dev_noise ? h->v.get() : nullptr;
  }
  const double* a(int64_t t) const { return A + t * dd; }
  const double* b(int64_t t) const { return B + t * d; }
  double* inf(int64_t t) const { return info + 3 * t; }
  int* fl(int64_t t) const { return flag + t; }

  // step t's process noise into the handle's v, ahead of the step that reads it (PF_NOISE_DEVICE only)
  pf_status draw(int64_t t) {
    if (!dev_noise) return PF_OK;
    return enqueue_noise(h, nseed, nepoch + (uint32_t)t, pf::STREAM_PROCESS, h->Lq, nullptr, h->v);
  }

  // the resample and the moments of step t, with the replayed uniform when there is one
  pf_status finish(int64_t t) {
    return enqueue_finish(h, replay ? h->rpU + t : h->U.get(), inf(t), means + t * d, covs + t * dd);
  }

  // everything back to the host (last_trace [n_lambda][d] nullable); waits, and the draws are consumed
  pf_status end(double* hmeans, double* hcovs, double* last_trace, int n_lambda) {
    hipStream_t s = h->stream;
    hi.resize((size_t)T * 3);
    hflag.resize(flag ? (size_t)T : 0);
    PF_HIPCHK(hipMemcpyAsync(hi.data(), info, hi.size() * 8, hipMemcpyDeviceToHost, s));
    if (flag) PF_HIPCHK(hipMemcpyAsync(hflag.data(), flag, hflag.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    PF_HIPCHK(hipMemcpyAsync(hmeans, means, (size_t)T * d * 8, hipMemcpyDeviceToHost, s));
    PF_HIPCHK(hipMemcpyAsync(hcovs, covs, (size_t)T * dd * 8, hipMemcpyDeviceToHost, s));
    if (last_trace)
      PF_HIPCHK(hipMemcpyAsync(last_trace, h->trace, (size_t)n_lambda * d * 8, hipMemcpyDeviceToHost, s));
    PF_HIPCHK(hipStreamSynchronize(s));
    h->rpT = -1;
    return PF_OK;
  }

  // the verdict on step t's weights, and its outputs (ess, flags nullable)
  pf_status alive(int64_t t) const {
    if (hi[3 * t + 2] != 0.0) return fail(PF_E_NAN, "no particle has a finite positive weight at step " + std::to_string(t));
    return PF_OK;
  }
  void report(int64_t t, double* ess, uint8_t* flags) const {
    if (ess) ess[t] = hi[3 * t];
    if (flags) flags[t] = hi[3 * t + 1] != 0.0 ? 1 : 0;
  }
};

}  // namespace

// The dense UKF tracker (pf_ukf_dense_*): state, constants and workspace on the device.
struct pf_ukf_dense_handle {
  int d = 0, obs = 0, device = 0, ctiles = 1;
  double g_alpha = 0.0, m1 = 0.0, m2 = 0.0;
  pf::UkfPlan plan{};
  pf::Stream stream;  // before the buffers: destroyed after them
  // state; its copy from before a sequence / tracked run; constants: ones, jitter, retry jitter, zeros
  DevBuf<double> m, P, past, bm, bP, bpast, Q, R, consts;
  // workspace: sym(P), factor, E and DX [2d + 1][d], partial sums, zbar, z - zbar, S, Pxz, K, two
  // products, the new state, z and u of the one-step entries
  DevBuf<double> Ps, W, E, DX, part, zbar, resid, S, Pxz, K, T1, T2, mn, Pn, z, u;
  DevBuf<int> flags;  // [2][NFLAG] of the one-step entries
  ~pf_ukf_dense_handle() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

namespace {

namespace uk = pf::ukf_dense;

// the shared first half of predict and update on stream s: sym(P), its factor (with the device-side
// retry), the sigma points' images in E (and DX), zbar, and z - zbar when z is given
void ukf_enqueue_sigma(pf_ukf_dense_handle* t, hipStream_t s, const uk::Fn& f, bool want_dx, const double* z,
                       double* zbar, int* fl) {
  const int d = t->d;
  const size_t n = (size_t)d;
  const int64_t dd = (int64_t)d * d;
  const dim3 ew((unsigned)((dd + 255) / 256));
  const double *ones = t->consts, *jit = t->consts + n, *jit2 = t->consts + 2 * n;
  hipLaunchKernelGGL(uk::k_ukf_sym, ew, dim3(256), 0, s, d, t->P.get(), t->Ps.get());
  pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
  hipLaunchKernelGGL(uk::k_ukf_chol, dim3(1), dim3(uk::LB), 0, s, d, t->Ps.get(), ones, jit, t->W.get(), fl, -1, 0);
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL(uk::k_ukf_chol, dim3(1), dim3(uk::LB), 0, s, d, t->Ps.get(), ones, jit2, t->W.get(), fl, 0, 1);
  uk::SigmaArgs a{};
  a.d = d; a.chunk = t->plan.chunk; a.gamma = t->plan.gamma; a.f = f;
  a.m = t->m; a.W = t->W; a.E = t->E; a.DX = want_dx ? t->DX.get() : nullptr; a.part = t->part;
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL(uk::k_ukf_sigma, dim3((unsigned)((d + 63) / 64), (unsigned)t->plan.splits), dim3(GB), 0, s, a);
  hipLaunchKernelGGL(uk::k_ukf_mean, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, d, t->plan.splits, t->plan.w,
                     f, t->m.get(), t->part.get(), z, zbar, t->E.get(), a.DX, t->resid.get());
}

void ukf_enqueue_prod(pf_ukf_dense_handle* t, hipStream_t s, const double* A, const double* B, const double* base,
                      double w0, double* out) {
  uk::ProdArgs p{t->d, A, B, base, t->plan.w, w0, out};
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL(uk::k_ukf_prod, dim3((unsigned)t->ctiles, (unsigned)t->ctiles), dim3(GB), 0, s, p);
}

// ukf.py:129-152 on stream s; u is a device pointer or null; fl [NFLAG] on the device
pf_status ukf_enqueue_predict(pf_ukf_dense_handle* t, hipStream_t s, const double* u, int* fl) {
  const int d = t->d;
  const dim3 ew((unsigned)(((int64_t)d * d + 255) / 256));
  PF_HIPCHK(hipMemsetAsync(fl, 0, uk::NFLAG * sizeof(int), s));
  const uk::Fn g{uk::F_SCALE, t->g_alpha, 0.0, u};
  ukf_enqueue_sigma(t, s, g, false, nullptr, t->mn, fl);
  ukf_enqueue_prod(t, s, t->E, t->E, t->Q, t->plan.w0, t->T1);
  hipLaunchKernelGGL(uk::k_ukf_sym, ew, dim3(256), 0, s, d, t->T1.get(), t->Pn.get());
  hipLaunchKernelGGL(uk::k_ukf_commit, ew, dim3(256), 0, s, d, fl, 1, -1, t->mn.get(), t->Pn.get(), t->m.get(),
                     t->P.get(), t->past.get());
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

// ukf.py:154-192 on stream s; z is a device pointer
pf_status ukf_enqueue_update(pf_ukf_dense_handle* t, hipStream_t s, const double* z, int* fl) {
  const int d = t->d;
  const size_t n = (size_t)d;
  const dim3 ew((unsigned)(((int64_t)d * d + 255) / 256));
  const double *ones = t->consts, *jit = t->consts + n, *zeros = t->consts + 3 * n;
  PF_HIPCHK(hipMemsetAsync(fl, 0, uk::NFLAG * sizeof(int), s));
  const uk::Fn hf{t->obs == OBS_EXP ? uk::F_EXP : uk::F_IDENTITY, t->m1, t->m2, nullptr};
  ukf_enqueue_sigma(t, s, hf, true, z, t->zbar, fl);
  ukf_enqueue_prod(t, s, t->E, t->E, t->R, t->plan.w0, t->T1);
  hipLaunchKernelGGL(uk::k_ukf_sym, ew, dim3(256), 0, s, d, t->T1.get(), t->S.get());
  ukf_enqueue_prod(t, s, t->DX, t->E, nullptr, 0.0, t->Pxz);
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL(uk::k_ukf_chol, dim3(1), dim3(uk::LB), 0, s, d, t->S.get(), ones, jit, t->W.get(), fl, -1, 2);
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL(pf::ledh_dense::k_chol_solve, solve_grid(d), dim3(uk::LB), pf::ledh_dense::solve_lds_bytes(d), s,
                     d, t->W.get(), (const double*)t->Pxz.get(), t->K.get());  // K = Pxz S^-1
  // K S K^T: T1 = K S (k_fm_gemm), T2 = T1 K^T (k_dense_gemm: both operands K-contiguous)
  pf::edh_flowmap::MatArgs ma{d, t->K, nullptr, t->S, nullptr, 1.0, 0.0, 1.0, 0.0, t->T1};
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL(pf::edh_flowmap::k_fm_gemm, dim3((unsigned)t->ctiles, (unsigned)t->ctiles), dim3(GB), 0, s, ma);
  GemmArgs ga{};
  ga.N = d; ga.d = d; ga.alpha = 1.0; ga.X = t->T1; ga.B = t->K; ga.c = zeros; ga.out = t->T2;
  pf::lds_poison_hook(s);
  hipLaunchKernelGGL((k_dense_gemm<G_MAP>), dim3((unsigned)t->ctiles, (unsigned)t->ctiles), dim3(GB), 0, s, ga);
  hipLaunchKernelGGL(uk::k_ukf_post, ew, dim3(256), 0, s, d, t->P.get(), t->T2.get(), t->Pn.get());
  pf::edh_flowmap::VecArgs va{d, t->K, t->resid, nullptr, t->m, 1.0, 1.0, 0.0, t->mn};
  hipLaunchKernelGGL(pf::edh_flowmap::k_fm_matvec, dim3((unsigned)((d + 3) / 4)), dim3(GB), 0, s, va);
  hipLaunchKernelGGL(uk::k_ukf_commit, ew, dim3(256), 0, s, d, fl, 1, 2, t->mn.get(), t->Pn.get(), t->m.get(),
                     t->P.get(), (double*)nullptr);
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

// the tracker's state to / from its backup, on stream s
pf_status ukf_backup(pf_ukf_dense_handle* t, hipStream_t s, bool restore) {
  const size_t d = (size_t)t->d;
  struct { DevBuf<double>*a, *b; size_t n; } v[] = {{&t->m, &t->bm, d}, {&t->P, &t->bP, d * d}, {&t->past, &t->bpast, d}};
  for (auto& e : v) {
    double *src = restore ? e.b->get() : e.a->get(), *dst = restore ? e.a->get() : e.b->get();
    PF_HIPCHK(hipMemcpyAsync(dst, src, e.n * 8, hipMemcpyDeviceToDevice, s));
  }
  return PF_OK;
}

// the first failing step of a sequence from its flags [T][2][NFLAG]: -1 when none failed
int64_t ukf_first_failure(const std::vector<int>& fl, int64_t T, const char** what) {
  for (int64_t t = 0; t < T; ++t) {
    const int* p = fl.data() + (size_t)t * 2 * uk::NFLAG;
    const int* u = p + uk::NFLAG;
    if (p[1]) { *what = "the covariance before predict"; return t; }
    if (u[1]) { *what = "the predicted covariance"; return t; }
    if (u[2]) { *what = "S"; return t; }
  }
  return -1;
}

// a tracked entry's tracker fits its filter
pf_status tracker_check(const pf_edh_dense_handle* h, const pf_ukf_dense_handle* tr) {
  if (tr->device != h->device) return fail(PF_E_ARG, "the tracker and the filter must be on the same device");
  if (tr->d != h->d) return fail(PF_E_ARG, "the tracker and the filter must share nx");
  return PF_OK;
}

// the end of a tracked entry whose verdict failed with bad (its message is the last error): the tracker's
// state from before the entry is put back
pf_status ukf_restore_after(pf_ukf_dense_handle* tr, hipStream_t s, pf_status bad) {
  const std::string msg = pf_last_error();
  if (ukf_backup(tr, s, true) != PF_OK || hipStreamSynchronize(s) != hipSuccess)
    return fail(PF_E_HIP, "the tracker's state could not be restored after: " + msg);
  return fail(bad, msg);
}

}  // namespace

extern "C" {

pf_status pf_ukf_dense_create(const pf_ukf_dense_model* m, int32_t device, pf_ukf_dense_handle** out) try {
  if (!m || !out) return fail(PF_E_ARG, "null argument");
  *out = nullptr;
  const int d = m->nx;
  if (d < 1 || d > MAXDIM) return fail(PF_E_ARG, "nx out of range (1 .. 1024)");
  if (m->obs_kind != PF_EDH_OBS_IDENTITY && m->obs_kind != PF_EDH_OBS_EXP)
    return fail(PF_E_ARG, "bad obs_kind (PF_EDH_OBS_IDENTITY or PF_EDH_OBS_EXP)");
  if (!std::isfinite(m->g_alpha) || !std::isfinite(m->m1) || !std::isfinite(m->m2))
    return fail(PF_E_ARG, "g_alpha, m1 and m2 must be finite");
  if (!(m->jitter >= 0.0) || !std::isfinite(m->jitter)) return fail(PF_E_ARG, "jitter must be finite and non-negative");
  pf::UkfPlan plan{};
  if (!pf::ukf_plan(d, m->alpha, m->beta, m->kappa, &plan))
    return fail(PF_E_ARG, "alpha, beta, kappa must be finite with alpha^2 (nx + kappa) positive");
  if (device < 0) return fail(PF_E_ARG, "bad device");
  if (!m->Q || !m->R) return fail(PF_E_ARG, "Q and R are required");
  const size_t n = (size_t)d, dd = n * n;
  for (size_t e = 0; e < dd; ++e)
    if (!std::isfinite(m->Q[e]) || !std::isfinite(m->R[e])) return fail(PF_E_ARG, "Q and R must be finite");

  PF_HIPCHK(hipSetDevice(device));
  std::unique_ptr<pf_ukf_dense_handle> t(new pf_ukf_dense_handle());
  t->d = d; t->obs = m->obs_kind; t->device = device; t->ctiles = (d + TN - 1) / TN;
  t->g_alpha = m->g_alpha; t->m1 = m->m1; t->m2 = m->m2; t->plan = plan;
  PF_HIPCHK(hipStreamCreateWithFlags(t->stream.out(), hipStreamNonBlocking));
  const size_t kd = (2 * n + 1) * n;
  struct A { DevBuf<double>* p; size_t n; };
  A allocs[] = {{&t->m, n}, {&t->P, dd}, {&t->past, n}, {&t->bm, n}, {&t->bP, dd}, {&t->bpast, n}, {&t->Q, dd},
                {&t->R, dd}, {&t->consts, 4 * n}, {&t->Ps, dd}, {&t->W, dd}, {&t->E, kd}, {&t->DX, kd},
                {&t->part, (size_t)plan.splits * n}, {&t->zbar, n}, {&t->resid, n}, {&t->S, dd}, {&t->Pxz, dd},
                {&t->K, dd}, {&t->T1, dd}, {&t->T2, dd}, {&t->mn, n}, {&t->Pn, dd}, {&t->z, n}, {&t->u, n}};
  for (auto& a : allocs) PF_HIPCHK(a.p->alloc(a.n));
  PF_HIPCHK(t->flags.alloc(2 * uk::NFLAG));
  std::vector<double> c(4 * n, 0.0);
  for (size_t j = 0; j < n; ++j) {
    c[j] = 1.0;
    c[n + j] = m->jitter;
    c[2 * n + j] = std::max(m->jitter, 1e-12);
  }
  hipStream_t s = t->stream;
  PF_HIPCHK(hipMemcpyAsync(t->consts, c.data(), 4 * n * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(t->Q, m->Q, dd * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(t->R, m->R, dd * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemsetAsync(t->m, 0, n * 8, s));
  PF_HIPCHK(hipMemsetAsync(t->past, 0, n * 8, s));
  PF_HIPCHK(hipMemsetAsync(t->P, 0, dd * 8, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  *out = t.release();
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ukf_dense_create"); }

void pf_ukf_dense_destroy(pf_ukf_dense_handle* t) { delete t; }

pf_status pf_ukf_dense_set_state(pf_ukf_dense_handle* t, const double* mean, const double* cov) try {
  if (!t || !mean || !cov) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(t->device));
  const size_t d = (size_t)t->d;
  hipStream_t s = t->stream;
  PF_HIPCHK(hipMemcpyAsync(t->m, mean, d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(t->past, mean, d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(t->P, cov, d * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ukf_dense_set_state"); }

pf_status pf_ukf_dense_get_state(pf_ukf_dense_handle* t, double* mean, double* cov) try {
  if (!t || !mean || !cov) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(t->device));
  const size_t d = (size_t)t->d;
  PF_HIPCHK(hipMemcpyAsync(mean, t->m, d * 8, hipMemcpyDeviceToHost, t->stream));
  PF_HIPCHK(hipMemcpyAsync(cov, t->P, d * d * 8, hipMemcpyDeviceToHost, t->stream));
  PF_HIPCHK(hipStreamSynchronize(t->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ukf_dense_get_state"); }

pf_status pf_ukf_dense_get_past_mean(pf_ukf_dense_handle* t, double* past_mean) try {
  if (!t || !past_mean) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(t->device));
  PF_HIPCHK(hipMemcpyAsync(past_mean, t->past, (size_t)t->d * 8, hipMemcpyDeviceToHost, t->stream));
  PF_HIPCHK(hipStreamSynchronize(t->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ukf_dense_get_past_mean"); }

pf_status pf_ukf_dense_predict(pf_ukf_dense_handle* t, const double* u) try {
  if (!t) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(t->device));
  hipStream_t s = t->stream;
  if (u) PF_HIPCHK(hipMemcpyAsync(t->u, u, (size_t)t->d * 8, hipMemcpyHostToDevice, s));
  const pf_status st = ukf_enqueue_predict(t, s, u ? t->u.get() : nullptr, t->flags);
  if (st != PF_OK) return st;
  int fl[uk::NFLAG] = {0, 0, 0, 0};
  PF_HIPCHK(hipMemcpyAsync(fl, t->flags, sizeof(fl), hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  if (fl[1]) return fail(PF_E_NOT_PD, "Matrix is not positive definite (the covariance before predict)");
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ukf_dense_predict"); }

pf_status pf_ukf_dense_update(pf_ukf_dense_handle* t, const double* z) try {
  if (!t || !z) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(t->device));
  hipStream_t s = t->stream;
  PF_HIPCHK(hipMemcpyAsync(t->z, z, (size_t)t->d * 8, hipMemcpyHostToDevice, s));
  const pf_status st = ukf_enqueue_update(t, s, t->z, t->flags);
  if (st != PF_OK) return st;
  int fl[uk::NFLAG] = {0, 0, 0, 0};
  PF_HIPCHK(hipMemcpyAsync(fl, t->flags, sizeof(fl), hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  if (fl[1]) return fail(PF_E_NOT_PD, "Matrix is not positive definite (the predicted covariance)");
  if (fl[2]) return fail(PF_E_NOT_PD, "Matrix is not positive definite (S)");
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ukf_dense_update"); }

pf_status pf_ukf_dense_sequence(pf_ukf_dense_handle* t, const double* Z, const double* U, int64_t T, double* Ps,
                                double* xbars, double* means, double* covs) try {
  if (!t || !Z) return fail(PF_E_ARG, "null argument");
  if (check_T(T) != PF_OK) return PF_E_ARG;
  PF_HIPCHK(hipSetDevice(t->device));
  hipStream_t s = t->stream;
  const size_t d = (size_t)t->d, dd = d * d;
  DevBuf<double> dZ, dU, dPs, dxb, dmean, dcov;
  DevBuf<int> dfl;
  PF_HIPCHK(dZ.alloc((size_t)T * d));
  if (U) PF_HIPCHK(dU.alloc((size_t)T * d));
  if (Ps) PF_HIPCHK(dPs.alloc((size_t)T * dd));
  if (xbars) PF_HIPCHK(dxb.alloc((size_t)T * d));
  if (means) PF_HIPCHK(dmean.alloc((size_t)T * d));
  if (covs) PF_HIPCHK(dcov.alloc((size_t)T * dd));
  PF_HIPCHK(dfl.alloc((size_t)T * 2 * uk::NFLAG));
  PF_HIPCHK(hipMemcpyAsync(dZ, Z, (size_t)T * d * 8, hipMemcpyHostToDevice, s));
  if (U) PF_HIPCHK(hipMemcpyAsync(dU, U, (size_t)T * d * 8, hipMemcpyHostToDevice, s));
  pf_status st = ukf_backup(t, s, false);
  for (int64_t k = 0; k < T && st == PF_OK; ++k) {
    int* fl = dfl + (size_t)k * 2 * uk::NFLAG;
    st = ukf_enqueue_predict(t, s, U ? dU + k * d : nullptr, fl);
    if (st != PF_OK) break;
    if (Ps) PF_HIPCHK(hipMemcpyAsync(dPs + k * dd, t->P, dd * 8, hipMemcpyDeviceToDevice, s));
    if (xbars) PF_HIPCHK(hipMemcpyAsync(dxb + k * d, t->past, d * 8, hipMemcpyDeviceToDevice, s));
    st = ukf_enqueue_update(t, s, dZ + k * d, fl + uk::NFLAG);
    if (st != PF_OK) break;
    if (means) PF_HIPCHK(hipMemcpyAsync(dmean + k * d, t->m, d * 8, hipMemcpyDeviceToDevice, s));
    if (covs) PF_HIPCHK(hipMemcpyAsync(dcov + k * dd, t->P, dd * 8, hipMemcpyDeviceToDevice, s));
  }
  if (st != PF_OK) {
    (void)ukf_backup(t, s, true);
    (void)hipStreamSynchronize(s);
    return st;
  }
  std::vector<int> fl((size_t)T * 2 * uk::NFLAG);
  PF_HIPCHK(hipMemcpyAsync(fl.data(), dfl, fl.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  if (Ps) PF_HIPCHK(hipMemcpyAsync(Ps, dPs, (size_t)T * dd * 8, hipMemcpyDeviceToHost, s));
  if (xbars) PF_HIPCHK(hipMemcpyAsync(xbars, dxb, (size_t)T * d * 8, hipMemcpyDeviceToHost, s));
  if (means) PF_HIPCHK(hipMemcpyAsync(means, dmean, (size_t)T * d * 8, hipMemcpyDeviceToHost, s));
  if (covs) PF_HIPCHK(hipMemcpyAsync(covs, dcov, (size_t)T * dd * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  const char* what = "";
  const int64_t bad = ukf_first_failure(fl, T, &what);
  if (bad >= 0) {
    if (ukf_backup(t, s, true) != PF_OK) return PF_E_HIP;
    PF_HIPCHK(hipStreamSynchronize(s));
    return fail(PF_E_NOT_PD, std::string("Matrix is not positive definite (") + what + " at step " +
                                 std::to_string(bad) + ")");
  }
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ukf_dense_sequence"); }

pf_status pf_edh_dense_flow_step_tracked(pf_edh_dense_handle* h, pf_ukf_dense_handle* tr, const double* R_diag,
                                         const double* z, const double* u, int32_t n_lambda, int32_t integrator,
                                         int32_t noise, const double* v, pf_ledh_info* info, double* etabar_trace,
                                         double* P_pred) try {
  if (!h || !tr || !R_diag || !z) return fail(PF_E_ARG, "null argument");
  pf_status st = tracker_check(h, tr);
  if (st == PF_OK) st = flow_check(h, R_diag, n_lambda, integrator_ok(integrator), noise, "EDH");
  if (st == PF_OK) st = step_ready(h, noise, v);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipStreamSynchronize(tr->stream));
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d;
  h->has_map = false;
  StepIn in{};
  st = flowmap_prepare(h, R_diag, n_lambda, etabar_trace != nullptr);
  if (st == PF_OK) st = upload_step(h, z, u, noise, v, &in);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipMemsetAsync(h->fmfail, 0, sizeof(int), s));
  st = ukf_backup(tr, s, false);
  if (st == PF_OK) st = ukf_enqueue_predict(tr, s, nullptr, tr->flags);  // UKFTracker.predict: no control
  if (st != PF_OK) return st;
  PF_HIPCHK(hipMemcpyAsync(h->fmP, tr->P, d * d * 8, hipMemcpyDeviceToDevice, s));  // kept for P_pred
  hipLaunchKernelGGL(uk::k_ukf_eta0, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, (int)d, h->alpha,
                     tr->past.get(), in.u, h->fmeta0.get());
  st = enqueue_flowmap(h, h->fmP, h->fmeta0, in.z, n_lambda, integrator, h->fmfail,
                       etabar_trace ? h->trace.get() : nullptr);
  if (st == PF_OK) st = enqueue_step(h, h->M, h->c, in.z, in.u, in.v, h->info);
  if (st == PF_OK) st = ukf_enqueue_update(tr, s, in.z, tr->flags + uk::NFLAG);
  if (st != PF_OK) {
    (void)ukf_backup(tr, s, true);
    (void)hipStreamSynchronize(s);
    return st;
  }
  double hi[3] = {0.0, 0.0, 0.0};
  int failed = 0;
  std::vector<int> fl(2 * uk::NFLAG);
  PF_HIPCHK(hipMemcpyAsync(fl.data(), tr->flags, fl.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  if (P_pred) PF_HIPCHK(hipMemcpyAsync(P_pred, h->fmP, d * d * 8, hipMemcpyDeviceToHost, s));
  st = download_step(h, hi, h->fmfail, &failed, etabar_trace, n_lambda);
  if (st != PF_OK) return st;
  // on a failure X and w are untouched: the state before the step is kept, and the tracker's is put back
  const char* what = "";
  if (ukf_first_failure(fl, 1, &what) == 0)
    st = fail(PF_E_NOT_PD, std::string("Matrix is not positive definite (the tracker's ") + what + ")");
  else if (failed != 0)
    st = fail(PF_E_NOT_PD, "Matrix is not positive definite (S of the EDH flow)");
  else
    st = commit_step(h, hi, info);
  if (st != PF_OK) return ukf_restore_after(tr, s, st);
  h->has_map = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_flow_step_tracked"); }

pf_status pf_edh_dense_flow_run_tracked(pf_edh_dense_handle* h, pf_ukf_dense_handle* tr, const double* R_diag,
                                        const double* Z, const double* U, int64_t T, int32_t n_lambda,
                                        int32_t integrator, int32_t noise, double* means, double* covs, double* ess,
                                        uint8_t* flags, double* last_trace) try {
  if (!h || !tr || !R_diag || !Z || !means || !covs) return fail(PF_E_ARG, "null argument");
  pf_status st = check_T(T);
  if (st == PF_OK) st = tracker_check(h, tr);
  if (st == PF_OK) st = flow_check(h, R_diag, n_lambda, integrator_ok(integrator), noise, "EDH");
  if (st == PF_OK) st = run_ready(h, T, noise);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipStreamSynchronize(tr->stream));  // the tracker's own entries end synchronised; be sure
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d;
  h->has_map = false;
  RunFrame f;
  DevBuf<int> dfl;  // the tracker's flags [T][2][NFLAG]
  PF_HIPCHK(dfl.alloc((size_t)T * 2 * uk::NFLAG));
  st = flowmap_prepare(h, R_diag, n_lambda, last_trace != nullptr);
  if (st == PF_OK) st = f.begin(h, T, noise, Z, U, nullptr, nullptr, true);
  if (st != PF_OK) return st;
  st = ukf_backup(tr, s, false);
  for (int64_t t = 0; t < T && st == PF_OK; ++t) {
    int* fl = dfl + (size_t)t * 2 * uk::NFLAG;
    st = f.draw(t);
    if (st == PF_OK) st = ukf_enqueue_predict(tr, s, nullptr, fl);  // UKFTracker.predict: no control
    if (st != PF_OK) break;
    hipLaunchKernelGGL(uk::k_ukf_eta0, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, (int)d, h->alpha,
                       tr->past.get(), f.u(t), h->fmeta0.get());
    st = enqueue_flowmap(h, tr->P, h->fmeta0, f.z(t), n_lambda, integrator, f.fl(t),
                         last_trace && t == T - 1 ? h->trace.get() : nullptr);
    if (st == PF_OK) st = enqueue_step(h, h->M, h->c, f.z(t), f.u(t), f.v(t), f.inf(t));
    if (st == PF_OK) st = f.finish(t);
    if (st == PF_OK) st = ukf_enqueue_update(tr, s, f.z(t), fl + uk::NFLAG);
  }
  if (st != PF_OK) {
    (void)ukf_backup(tr, s, true);
    (void)hipStreamSynchronize(s);
    return st;
  }
  std::vector<int> fl((size_t)T * 2 * uk::NFLAG);
  PF_HIPCHK(hipMemcpyAsync(fl.data(), dfl, fl.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  st = f.end(means, covs, last_trace, n_lambda);
  if (st != PF_OK) return st;
  // per step: the tracker's flags, the flow's flag, the weights; the first failing step is reported
  const char* what = "";
  const int64_t tb = ukf_first_failure(fl, T, &what);
  for (int64_t t = 0; t < T && st == PF_OK; ++t) {
    if (tb == t)
      st = fail(PF_E_NOT_PD, std::string("Matrix is not positive definite (the tracker's ") + what + " at step " +
                                 std::to_string(t) + ")");
    else if (f.hflag[(size_t)t] != 0)
      st = fail(PF_E_NOT_PD, "Matrix is not positive definite (S of the EDH flow at step " + std::to_string(t) + ")");
    else
      st = f.alive(t);
  }
  if (st != PF_OK) return ukf_restore_after(tr, s, st);
  for (int64_t t = 0; t < T; ++t) f.report(t, ess, flags);
  h->has_map = true;
  h->initialised = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_flow_run_tracked"); }

pf_status pf_edh_dense_create(const pf_edh_dense_model* m, const pf_edh_dense_opts* o,
                              pf_edh_dense_handle** out) try {
  if (!m || !o || !out) return fail(PF_E_ARG, "null argument");
  *out = nullptr;
  if (o->n_particles < 1) return fail(PF_E_ARG, "n_particles must be positive");
  if (o->n_particles > MAXN) return fail(PF_E_ARG, "n_particles too large (max 1048576)");
  const int d = m->nx;
  if (d < 1 || d > MAXDIM) return fail(PF_E_ARG, "nx out of range (1 .. 1024)");
  if (m->obs_kind != PF_EDH_OBS_IDENTITY && m->obs_kind != PF_EDH_OBS_EXP)
    return fail(PF_E_ARG, "bad obs_kind (PF_EDH_OBS_IDENTITY or PF_EDH_OBS_EXP)");
  if (m->like_kind != PF_EDH_LIKE_GAUSSIAN && m->like_kind != PF_EDH_LIKE_POISSON)
    return fail(PF_E_ARG, "bad like_kind (PF_EDH_LIKE_GAUSSIAN or PF_EDH_LIKE_POISSON)");
  if (!std::isfinite(m->alpha) || !std::isfinite(m->m1) || !std::isfinite(m->m2))
    return fail(PF_E_ARG, "alpha, m1 and m2 must be finite");
  if (!(o->resample_ess_ratio >= 0.0) || !std::isfinite(o->resample_ess_ratio))
    return fail(PF_E_ARG, "resample_ess_ratio must be finite and non-negative");
  if (!m->Q) return fail(PF_E_ARG, "Q is required");
  std::vector<double> rd((size_t)d, 1.0);
  if (m->like_kind == PF_EDH_LIKE_GAUSSIAN) {
    if (!m->R_diag) return fail(PF_E_ARG, "R_diag is required for the Gaussian likelihood");
    for (int j = 0; j < d; ++j) {
      if (!(m->R_diag[j] > 0.0) || !std::isfinite(m->R_diag[j]))
        return fail(PF_E_NOT_PD, "Matrix is not positive definite (R)");
      rd[j] = m->R_diag[j];
    }
  }
  std::vector<double> L, W;
  if (!pf::chol_lower(m->Q, d, 0.0, L)) return fail(PF_E_NOT_PD, "Matrix is not positive definite (Q)");
  pf::lower_inverse(L.data(), d, W);

  PF_HIPCHK(hipSetDevice(o->device));
  std::unique_ptr<pf_edh_dense_handle> h(new pf_edh_dense_handle());
  const int N = (int)o->n_particles;
  h->N = N; h->d = d; h->obs = m->obs_kind; h->like = m->like_kind; h->device = o->device;
  h->alpha = m->alpha; h->m1 = m->m1; h->m2 = m->m2; h->ratio = o->resample_ess_ratio;
  h->ctiles = (d + TN - 1) / TN;
  // the split counts are part of the summation order: functions of (N, d) only
  int S = std::min(32, std::max(1, (N + 511) / 512));
  h->cchunk = ((N + S - 1) / S + KC - 1) / KC * KC;
  h->cS = (N + h->cchunk - 1) / h->cchunk;
  S = std::min(64, std::max(1, (N + 255) / 256));
  h->mchunk = (N + S - 1) / S;
  h->mS = (N + h->mchunk - 1) / h->mchunk;

  PF_HIPCHK(hipStreamCreateWithFlags(h->stream.out(), hipStreamNonBlocking));
  const size_t nd = (size_t)N * d, dd = (size_t)d * d, qn = (size_t)h->ctiles * N;
  struct A { DevBuf<double>* p; size_t n; };
  A allocs[] = {{&h->X, nd}, {&h->Xn, nd}, {&h->v, nd}, {&h->w, (size_t)N}, {&h->wn, (size_t)N},
                {&h->logw, (size_t)N}, {&h->cdf, (size_t)N}, {&h->qx, qn}, {&h->qv, qn}, {&h->M, dd},
                {&h->c, (size_t)d}, {&h->z, (size_t)d}, {&h->u, (size_t)d}, {&h->W, dd}, {&h->Lq, dd},
                {&h->rdiag, (size_t)d}, {&h->info, 3}, {&h->U, 1}, {&h->mean, (size_t)d}, {&h->cov, dd},
                {&h->mpart, (size_t)h->mS * d}, {&h->wpart, (size_t)h->mS}, {&h->wsum, 1},
                {&h->cpart, (size_t)h->cS * dd}};
  for (auto& a : allocs) PF_HIPCHK(a.p->alloc(a.n));
  PF_HIPCHK(hipMemcpyAsync(h->W, W.data(), dd * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipMemcpyAsync(h->Lq, L.data(), dd * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipMemcpyAsync(h->rdiag, rd.data(), (size_t)d * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipMemsetAsync(h->U, 0, 8, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  *out = h.release();
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_create"); }

void pf_edh_dense_destroy(pf_edh_dense_handle* h) { delete h; }

pf_status pf_edh_dense_set_state(pf_edh_dense_handle* h, const double* particles, const double* weights) try {
  if (!h || !particles || !weights) return fail(PF_E_ARG, "null argument");
  for (int i = 0; i < h->N; ++i)
    if (!(weights[i] >= 0.0) || !std::isfinite(weights[i])) return fail(PF_E_ARG, "weights must be finite and non-negative");
  PF_HIPCHK(hipSetDevice(h->device));
  h->initialised = false;
  h->pending = false;
  PF_HIPCHK(hipMemcpyAsync(h->X, particles, (size_t)h->N * h->d * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipMemcpyAsync(h->w, weights, (size_t)h->N * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  h->initialised = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_set_state"); }

pf_status pf_edh_dense_get_particles(pf_edh_dense_handle* h, double* particles) try {
  if (!h || !particles) return fail(PF_E_ARG, "null argument");
  const pf_status st = check_ready(h);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipMemcpyAsync(particles, h->X, (size_t)h->N * h->d * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_get_particles"); }

pf_status pf_edh_dense_get_weights(pf_edh_dense_handle* h, double* weights) try {
  if (!h || !weights) return fail(PF_E_ARG, "null argument");
  const pf_status st = check_ready(h);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipMemcpyAsync(weights, h->w, (size_t)h->N * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_get_weights"); }

pf_status pf_edh_dense_step(pf_edh_dense_handle* h, const double* M, const double* c, const double* z,
                            const double* u, int32_t noise, const double* v, pf_ledh_info* info) try {
  if (!h || !M || !c || !z) return fail(PF_E_ARG, "null argument");
  pf_status st = check_noise(noise, "EDH");
  if (st == PF_OK) st = step_ready(h, noise, v);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d;
  h->has_map = false;  // M / c now hold the caller's map
  PF_HIPCHK(hipMemcpyAsync(h->M, M, d * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->c, c, d * 8, hipMemcpyHostToDevice, s));
  StepIn in{};
  st = upload_step(h, z, u, noise, v, &in);
  if (st == PF_OK) st = enqueue_step(h, h->M, h->c, in.z, in.u, in.v, h->info);
  double hi[3] = {0.0, 0.0, 0.0};
  if (st == PF_OK) st = download_step(h, hi, nullptr, nullptr, nullptr, 0);
  if (st != PF_OK) return st;
  return commit_step(h, hi, info);
} catch (...) { return pf::on_exception("pf_edh_dense_step"); }

pf_status pf_edh_dense_finish(pf_edh_dense_handle* h, const double* U, double* mean, double* cov) try {
  if (!h || !mean || !cov) return fail(PF_E_ARG, "null argument");
  if (!h->initialised) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  if (!h->pending) return fail(PF_E_ARG, "no step is pending");
  if (h->last_flag && !U) return fail(PF_E_ARG, "the step resamples: U is required");
  if (U && !(U[0] >= 0.0 && U[0] < 1.0)) return fail(PF_E_ARG, "U must be in [0, 1)");
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d;
  if (U) PF_HIPCHK(hipMemcpyAsync(h->U, U, 8, hipMemcpyHostToDevice, s));
  h->initialised = false;  // until the new state is complete
  h->pending = false;
  const pf_status st = enqueue_finish(h, h->U, h->info, h->mean, h->cov);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipMemcpyAsync(mean, h->mean, d * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(cov, h->cov, d * d * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  h->initialised = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_finish"); }

pf_status pf_edh_dense_set_run_replay(pf_edh_dense_handle* h, const double* V, const double* U, int64_t T) try {
  if (!h || !U) return fail(PF_E_ARG, "null argument");
  if (check_T(T) != PF_OK) return PF_E_ARG;
  for (int64_t t = 0; t < T; ++t)
    if (!(U[t] >= 0.0 && U[t] < 1.0)) return fail(PF_E_ARG, "U must be in [0, 1)");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  h->rpT = -1;
  const size_t nd = (size_t)h->N * h->d;
  PF_HIPCHK(h->rpU.alloc((size_t)T));
  PF_HIPCHK(hipMemcpy(h->rpU, U, (size_t)T * 8, hipMemcpyHostToDevice));
  h->rp_has_v = V != nullptr;
  if (V) {
    PF_HIPCHK(h->rpV.alloc((size_t)T * nd));
    PF_HIPCHK(hipMemcpy(h->rpV, V, (size_t)T * nd * 8, hipMemcpyHostToDevice));
  } else {
    h->rpV.reset();
  }
  h->rpT = T;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_set_run_replay"); }

pf_status pf_edh_dense_run(pf_edh_dense_handle* h, const double* Ms, const double* cs, const double* Z,
                           const double* U, int64_t T, int32_t noise, double* means, double* covs, double* ess,
                           uint8_t* flags) try {
  if (!h || !Ms || !cs || !Z || !means || !covs) return fail(PF_E_ARG, "null argument");
  pf_status st = check_T(T);
  if (st == PF_OK) st = check_noise(noise, "EDH");
  if (st == PF_OK) st = run_ready(h, T, noise);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  RunFrame f;
  st = f.begin(h, T, noise, Z, U, Ms, cs, false);
  if (st != PF_OK) return st;
  for (int64_t t = 0; t < T; ++t) {
    st = f.draw(t);
    if (st == PF_OK) st = enqueue_step(h, f.a(t), f.b(t), f.z(t), f.u(t), f.v(t), f.inf(t));
    if (st == PF_OK) st = f.finish(t);
    if (st != PF_OK) {
      (void)hipStreamSynchronize(h->stream);
      return st;
    }
  }
  st = f.end(means, covs, nullptr, 0);
  for (int64_t t = 0; t < T && st == PF_OK; ++t)
    if ((st = f.alive(t)) == PF_OK) f.report(t, ess, flags);
  if (st != PF_OK) return st;
  h->initialised = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_run"); }

pf_status pf_ledh_dense_step(pf_edh_dense_handle* h, const double* P, const double* R_diag, const double* z,
                             const double* u, int32_t n_lambda, int32_t noise, const double* v, pf_ledh_info* info,
                             double* eta0_trace) try {
  if (!h || !P || !R_diag || !z) return fail(PF_E_ARG, "null argument");
  pf::LedhDensePlan plan{};
  pf_status st = ledh_check(h, R_diag, n_lambda, noise, &plan);
  if (st == PF_OK) st = step_ready(h, noise, v);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d;
  st = ledh_prepare(h, plan, R_diag, n_lambda, eta0_trace != nullptr);
  if (st != PF_OK) return st;
  h->has_map = false;  // M holds P
  PF_HIPCHK(hipMemcpyAsync(h->M, P, d * d * 8, hipMemcpyHostToDevice, s));
  StepIn in{};
  st = upload_step(h, z, u, noise, v, &in);
  if (st == PF_OK)
    st = enqueue_flow(h, plan, h->M, in.z, in.u, in.v, n_lambda, h->lnfail, eta0_trace ? h->trace.get() : nullptr);
  if (st == PF_OK) st = enqueue_weights(h, in.z, in.u, in.v, h->theta, h->info);
  double hi[3] = {0.0, 0.0, 0.0};
  int nfail = 0;
  if (st == PF_OK) st = download_step(h, hi, h->lnfail, &nfail, eta0_trace, n_lambda);
  if (st != PF_OK) return st;
  if (nfail != 0) {  // X and w are untouched: the state before the step is kept
    std::vector<int> f((size_t)h->N);
    PF_HIPCHK(hipMemcpy(f.data(), h->lfail, f.size() * sizeof(int), hipMemcpyDeviceToHost));
    const int64_t first = std::find(f.begin(), f.end(), 1) - f.begin();
    return fail(PF_E_NOT_PD, "Matrix is not positive definite (S of " + std::to_string(nfail) +
                                 " particles, the first is particle " + std::to_string(first) + ")");
  }
  return commit_step(h, hi, info);
} catch (...) { return pf::on_exception("pf_ledh_dense_step"); }

pf_status pf_ledh_dense_run(pf_edh_dense_handle* h, const double* Ps, const double* R_diag, const double* Z,
                            const double* U, int64_t T, int32_t n_lambda, int32_t noise, double* means, double* covs,
                            double* ess, uint8_t* flags) try {
  if (!h || !Ps || !R_diag || !Z || !means || !covs) return fail(PF_E_ARG, "null argument");
  pf::LedhDensePlan plan{};
  pf_status st = check_T(T);
  if (st == PF_OK) st = ledh_check(h, R_diag, n_lambda, noise, &plan);
  if (st == PF_OK) st = run_ready(h, T, noise);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  RunFrame f;
  st = ledh_prepare(h, plan, R_diag, n_lambda, false);
  if (st == PF_OK) st = f.begin(h, T, noise, Z, U, Ps, nullptr, true);
  if (st != PF_OK) return st;
  for (int64_t t = 0; t < T; ++t) {
    st = f.draw(t);
    if (st == PF_OK) st = enqueue_flow(h, plan, f.a(t), f.z(t), f.u(t), f.v(t), n_lambda, f.fl(t), nullptr);
    if (st == PF_OK) st = enqueue_weights(h, f.z(t), f.u(t), f.v(t), h->theta, f.inf(t));
    if (st == PF_OK) st = f.finish(t);
    if (st != PF_OK) {
      (void)hipStreamSynchronize(h->stream);
      return st;
    }
  }
  st = f.end(means, covs, nullptr, 0);
  for (int64_t t = 0; t < T && st == PF_OK; ++t) {
    const int nf = f.hflag[(size_t)t];  // the number of failed particles
    if (nf != 0)
      st = fail(PF_E_NOT_PD, "Matrix is not positive definite (S of " + std::to_string(nf) + " particles at step " +
                                 std::to_string(t) + ")");
    else if ((st = f.alive(t)) == PF_OK)
      f.report(t, ess, flags);
  }
  if (st != PF_OK) return st;
  h->initialised = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ledh_dense_run"); }

pf_status pf_edh_dense_flow_step(pf_edh_dense_handle* h, const double* P, const double* etabar0,
                                 const double* R_diag, const double* z, const double* u, int32_t n_lambda,
                                 int32_t integrator, int32_t noise, const double* v, pf_ledh_info* info,
                                 double* etabar_trace) try {
  if (!h || !P || !etabar0 || !R_diag || !z) return fail(PF_E_ARG, "null argument");
  pf_status st = flow_check(h, R_diag, n_lambda, integrator_ok(integrator), noise, "EDH");
  if (st == PF_OK) st = step_ready(h, noise, v);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d;
  h->has_map = false;
  st = flowmap_prepare(h, R_diag, n_lambda, etabar_trace != nullptr);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipMemcpyAsync(h->fmP, P, d * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->fmeta0, etabar0, d * 8, hipMemcpyHostToDevice, s));
  StepIn in{};
  st = upload_step(h, z, u, noise, v, &in);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipMemsetAsync(h->fmfail, 0, sizeof(int), s));
  st = enqueue_flowmap(h, h->fmP, h->fmeta0, in.z, n_lambda, integrator, h->fmfail,
                       etabar_trace ? h->trace.get() : nullptr);
  if (st == PF_OK) st = enqueue_step(h, h->M, h->c, in.z, in.u, in.v, h->info);
  double hi[3] = {0.0, 0.0, 0.0};
  int failed = 0;
  if (st == PF_OK) st = download_step(h, hi, h->fmfail, &failed, etabar_trace, n_lambda);
  if (st != PF_OK) return st;
  // X and w are untouched: the state before the step is kept
  if (failed != 0) return fail(PF_E_NOT_PD, "Matrix is not positive definite (S of the EDH flow)");
  h->has_map = true;  // the map is complete whatever the weights say
  return commit_step(h, hi, info);
} catch (...) { return pf::on_exception("pf_edh_dense_flow_step"); }

pf_status pf_edh_dense_flow_run(pf_edh_dense_handle* h, const double* Ps, const double* etabar0s,
                                const double* R_diag, const double* Z, const double* U, int64_t T, int32_t n_lambda,
                                int32_t integrator, int32_t noise, double* means, double* covs, double* ess,
                                uint8_t* flags, double* last_trace) try {
  if (!h || !Ps || !etabar0s || !R_diag || !Z || !means || !covs) return fail(PF_E_ARG, "null argument");
  pf_status st = check_T(T);
  if (st == PF_OK) st = flow_check(h, R_diag, n_lambda, integrator_ok(integrator), noise, "EDH");
  if (st == PF_OK) st = run_ready(h, T, noise);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  h->has_map = false;
  RunFrame f;
  st = flowmap_prepare(h, R_diag, n_lambda, last_trace != nullptr);
  if (st == PF_OK) st = f.begin(h, T, noise, Z, U, Ps, etabar0s, true);
  if (st != PF_OK) return st;
  for (int64_t t = 0; t < T; ++t) {
    st = f.draw(t);
    if (st == PF_OK)
      st = enqueue_flowmap(h, f.a(t), f.b(t), f.z(t), n_lambda, integrator, f.fl(t),
                           last_trace && t == T - 1 ? h->trace.get() : nullptr);
    if (st == PF_OK) st = enqueue_step(h, h->M, h->c, f.z(t), f.u(t), f.v(t), f.inf(t));
    if (st == PF_OK) st = f.finish(t);
    if (st != PF_OK) {
      (void)hipStreamSynchronize(h->stream);
      return st;
    }
  }
  st = f.end(means, covs, last_trace, n_lambda);
  for (int64_t t = 0; t < T && st == PF_OK; ++t) {
    if (f.hflag[(size_t)t] != 0)
      st = fail(PF_E_NOT_PD, "Matrix is not positive definite (S of the EDH flow at step " + std::to_string(t) + ")");
    else if ((st = f.alive(t)) == PF_OK)
      f.report(t, ess, flags);
  }
  if (st != PF_OK) return st;
  h->has_map = true;
  h->initialised = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_flow_run"); }

pf_status pf_edh_dense_set_noise(pf_edh_dense_handle* h, uint64_t seed, uint32_t epoch) try {
  if (!h) return fail(PF_E_ARG, "null handle");
  h->nseed = seed;
  h->nepoch = epoch;
  h->noise_armed = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_set_noise"); }

pf_status pf_edh_dense_noise_draws(pf_edh_dense_handle* h, uint64_t seed, uint32_t epoch, double* V) try {
  if (!h || !V) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(h->device));
  // v is written only ahead of the step that reads it: nothing of the state lives there
  const pf_status st = enqueue_noise(h, seed, epoch, pf::STREAM_PROCESS, h->Lq, nullptr, h->v);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipMemcpyAsync(V, h->v, (size_t)h->N * h->d * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_noise_draws"); }

pf_status pf_edh_dense_init_gaussian(pf_edh_dense_handle* h, const double* mean0, const double* cov0, uint64_t seed,
                                     uint32_t epoch, double* mean, double* cov) try {
  if (!h || !mean0 || !cov0 || !mean || !cov) return fail(PF_E_ARG, "null argument");
  const size_t d = (size_t)h->d;
  for (size_t j = 0; j < d; ++j)
    if (!std::isfinite(mean0[j])) return fail(PF_E_ARG, "mean0 must be finite");
  std::vector<double> F;
  if (!pf::chol_lower(cov0, h->d, 0.0, F)) return fail(PF_E_NOT_PD, "Matrix is not positive definite (cov0)");
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  h->initialised = false;
  h->pending = false;
  h->has_map = false;  // M / c hold the factor and mean0
  PF_HIPCHK(hipMemcpyAsync(h->M, F.data(), d * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->c, mean0, d * 8, hipMemcpyHostToDevice, s));
  pf_status st = enqueue_noise(h, seed, epoch, pf::STREAM_INIT, h->M, h->c, h->X);
  if (st != PF_OK) return st;
  hipLaunchKernelGGL(k_fill, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, s, h->w.get(), h->N,
                     1.0 / (double)h->N);
  PF_HIPCHK(hipGetLastError());
  st = enqueue_moments(h, h->mean, h->cov);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipMemcpyAsync(mean, h->mean, d * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(cov, h->cov, d * d * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));  // also: F outlives the upload
  h->initialised = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_init_gaussian"); }

pf_status pf_edh_dense_get_map(pf_edh_dense_handle* h, double* M, double* c) try {
  if (!h || !M || !c) return fail(PF_E_ARG, "null argument");
  if (!h->has_map) return fail(PF_E_ARG, "no device-composed map: call pf_edh_dense_flow_step or _flow_run first");
  PF_HIPCHK(hipSetDevice(h->device));
  const size_t d = (size_t)h->d;
  PF_HIPCHK(hipMemcpyAsync(M, h->M, d * d * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipMemcpyAsync(c, h->c, d * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_get_map"); }

void* pf_edh_dense_stream(pf_edh_dense_handle* h) { return h ? (void*)h->stream : nullptr; }

pf_status pf_edh_dense_synchronize(pf_edh_dense_handle* h) try {
  if (!h) return fail(PF_E_ARG, "null handle");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_synchronize"); }

}  // extern "C"
