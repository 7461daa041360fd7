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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pf_edh.h"
#include "pf_edh_dense_kernels.h"
#include "pf_hooks.h"
#include "pf_host.h"
#include "pf_ledh_dense_kernels.h"
#include "pf_ledh_dense_plan.h"

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
  ~pf_edh_dense_handle() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

namespace {

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
  if (n_lambda < 1 || n_lambda > (1 << 20)) return fail(PF_E_ARG, "n_lambda must be positive");
  if (noise != PF_NOISE_NONE && noise != PF_NOISE_HOST)
    return fail(PF_E_ARG, "noise must be PF_NOISE_NONE or PF_NOISE_HOST on the dense LEDH path");
  for (int j = 0; j < h->d; ++j)
    if (!(R_diag[j] > 0.0) || !std::isfinite(R_diag[j])) return fail(PF_E_ARG, "R_diag must be finite and positive");
  if (!pf::ledh_dense_plan(h->N, h->d, ledh_ws_cap(), plan))
    return fail(PF_E_ARG, "the workspace cap does not hold one particle's factors (16 d^2 bytes)");
  return PF_OK;
}

// buffers of the LEDH flow (after hipSetDevice); R_diag is uploaded on the stream
pf_status ledh_prepare(pf_edh_dense_handle* h, const pf::LedhDensePlan& plan, const double* R_diag, int n_lambda,
                       bool want_trace) {
  const size_t N = (size_t)h->N, d = (size_t)h->d;
  if (!h->theta) PF_HIPCHK(h->theta.alloc(N));
  if (!h->lfail) PF_HIPCHK(h->lfail.alloc(N));
  if (!h->lnfail) PF_HIPCHK(h->lnfail.alloc(1));
  if (!h->frd) PF_HIPCHK(h->frd.alloc(d));
  if (h->ws_bytes != plan.ws_bytes) {
    h->ws_bytes = 0;
    PF_HIPCHK(h->ws.alloc((size_t)plan.ws_bytes / sizeof(double)));
    h->ws_bytes = plan.ws_bytes;
  }
  if (want_trace && h->trace_L < n_lambda) {
    h->trace_L = 0;
    PF_HIPCHK(h->trace.alloc((size_t)n_lambda * d));
    h->trace_L = n_lambda;
  }
  const size_t lds = pf::ledh_dense::lds_bytes(h->d);
  if (lds > 48 * 1024)
    PF_HIPCHK(hipFuncSetAttribute((const void*)pf::ledh_dense::k_ledh_flow, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds));
  PF_HIPCHK(hipMemcpyAsync(h->frd, R_diag, d * 8, hipMemcpyHostToDevice, h->stream));
  return PF_OK;
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

// resample (decision on the device) into X / w, then the weighted moments into mean / cov
pf_status enqueue_finish(pf_edh_dense_handle* h, const double* U, const double* info, double* mean, double* cov) {
  hipStream_t s = h->stream;
  const int N = h->N, d = h->d;
  pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
  hipLaunchKernelGGL(k_cdf, dim3(1), dim3(RB), 0, s, h->wn, N, info, h->cdf);
  hipLaunchKernelGGL(k_gather, dim3((unsigned)((N + 3) / 4)), dim3(GB), 0, s, h->Xn, h->wn, h->cdf, U, info, N, d,
                     h->X, h->w);
  PF_HIPCHK(hipGetLastError());
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

}  // namespace

extern "C" {

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

  auto bail = [](const char* what) { return fail(PF_E_HIP, std::string("hipMalloc failed: ") + what); };
  if (hipStreamCreateWithFlags(h->stream.out(), hipStreamNonBlocking) != hipSuccess) return bail("stream");
  const size_t nd = (size_t)N * d, dd = (size_t)d * d, qn = (size_t)h->ctiles * N;
  struct A { DevBuf<double>* p; size_t n; };
  A allocs[] = {{&h->X, nd}, {&h->Xn, nd}, {&h->v, nd}, {&h->w, (size_t)N}, {&h->wn, (size_t)N},
                {&h->logw, (size_t)N}, {&h->cdf, (size_t)N}, {&h->qx, qn}, {&h->qv, qn}, {&h->M, dd},
                {&h->c, (size_t)d}, {&h->z, (size_t)d}, {&h->u, (size_t)d}, {&h->W, dd}, {&h->rdiag, (size_t)d},
                {&h->info, 3}, {&h->U, 1}, {&h->mean, (size_t)d}, {&h->cov, dd}, {&h->mpart, (size_t)h->mS * d},
                {&h->wpart, (size_t)h->mS}, {&h->wsum, 1}, {&h->cpart, (size_t)h->cS * dd}};
  for (auto& a : allocs)
    if (a.p->alloc(a.n) != hipSuccess) return bail("state");
  if (hipMemcpyAsync(h->W, W.data(), dd * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(h->rdiag, rd.data(), (size_t)d * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemsetAsync(h->U, 0, 8, h->stream) != hipSuccess)
    return bail("upload");
  if (hipStreamSynchronize(h->stream) != hipSuccess) return bail("upload");
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
  if (!h->initialised) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  if (h->pending) return fail(PF_E_ARG, "a step is pending: call pf_edh_dense_finish first");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipMemcpyAsync(particles, h->X, (size_t)h->N * h->d * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_get_particles"); }

pf_status pf_edh_dense_get_weights(pf_edh_dense_handle* h, double* weights) try {
  if (!h || !weights) return fail(PF_E_ARG, "null argument");
  if (!h->initialised) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  if (h->pending) return fail(PF_E_ARG, "a step is pending: call pf_edh_dense_finish first");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipMemcpyAsync(weights, h->w, (size_t)h->N * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_get_weights"); }

pf_status pf_edh_dense_step(pf_edh_dense_handle* h, const double* M, const double* c, const double* z,
                            const double* u, int32_t noise, const double* v, pf_ledh_info* info) try {
  if (!h || !M || !c || !z) return fail(PF_E_ARG, "null argument");
  if (noise != PF_NOISE_NONE && noise != PF_NOISE_HOST)
    return fail(PF_E_ARG, "noise must be PF_NOISE_NONE or PF_NOISE_HOST on the dense EDH path");
  if (noise == PF_NOISE_HOST && !v) return fail(PF_E_ARG, "PF_NOISE_HOST needs v");
  if (!h->initialised) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  if (h->pending) return fail(PF_E_ARG, "a step is pending: call pf_edh_dense_finish first");
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d;
  PF_HIPCHK(hipMemcpyAsync(h->M, M, d * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->c, c, d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->z, z, d * 8, hipMemcpyHostToDevice, s));
  if (u) PF_HIPCHK(hipMemcpyAsync(h->u, u, d * 8, hipMemcpyHostToDevice, s));
  if (noise == PF_NOISE_HOST) PF_HIPCHK(hipMemcpyAsync(h->v, v, (size_t)h->N * d * 8, hipMemcpyHostToDevice, s));
  const pf_status st = enqueue_step(h, h->M, h->c, h->z, u ? h->u.get() : nullptr,
                                    noise == PF_NOISE_HOST ? h->v.get() : nullptr, h->info);
  if (st != PF_OK) return st;
  double hi[3] = {0.0, 0.0, 0.0};
  PF_HIPCHK(hipMemcpyAsync(hi, h->info, sizeof(hi), hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  if (hi[2] != 0.0) return fail(PF_E_NAN, "no particle has a finite positive weight");
  h->pending = true;
  h->last_flag = hi[1] != 0.0 ? 1 : 0;
  if (info) {
    info->ess = hi[0];
    info->resample = h->last_flag;
  }
  return PF_OK;
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
  if (T < 1 || T > (1 << 20)) return fail(PF_E_ARG, "T out of range");
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
  if (T < 1 || T > (1 << 20)) return fail(PF_E_ARG, "T out of range");
  if (noise != PF_NOISE_NONE && noise != PF_NOISE_HOST)
    return fail(PF_E_ARG, "noise must be PF_NOISE_NONE or PF_NOISE_HOST on the dense EDH path");
  if (!h->initialised) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  if (h->pending) return fail(PF_E_ARG, "a step is pending: call pf_edh_dense_finish first");
  if (h->rpT != T && (h->ratio > 0.0 || noise == PF_NOISE_HOST))
    return fail(PF_E_ARG, "pf_edh_dense_set_run_replay must give the draws of a run of exactly this T");
  if (noise == PF_NOISE_HOST && !h->rp_has_v) return fail(PF_E_ARG, "PF_NOISE_HOST needs the replayed V");
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d, dd = d * d, nd = (size_t)h->N * d;
  DevBuf<double> dM, dc, dZ, dU, dmean, dcov, dinfo;
  PF_HIPCHK(dM.alloc((size_t)T * dd));
  PF_HIPCHK(dc.alloc((size_t)T * d));
  PF_HIPCHK(dZ.alloc((size_t)T * d));
  if (U) PF_HIPCHK(dU.alloc((size_t)T * d));
  PF_HIPCHK(dmean.alloc((size_t)T * d));
  PF_HIPCHK(dcov.alloc((size_t)T * dd));
  PF_HIPCHK(dinfo.alloc((size_t)T * 3));
  PF_HIPCHK(hipMemcpyAsync(dM, Ms, (size_t)T * dd * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(dc, cs, (size_t)T * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(dZ, Z, (size_t)T * d * 8, hipMemcpyHostToDevice, s));
  if (U) PF_HIPCHK(hipMemcpyAsync(dU, U, (size_t)T * d * 8, hipMemcpyHostToDevice, s));
  h->initialised = false;  // a failure inside the run leaves the handle uninitialised
  const bool replay = h->rpT == T;
  for (int64_t t = 0; t < T; ++t) {
    double* info = dinfo + 3 * t;
    pf_status st = enqueue_step(h, dM + t * dd, dc + t * d, dZ + t * d, U ? dU + t * d : nullptr,
                                noise == PF_NOISE_HOST ? h->rpV + t * nd : nullptr, info);
    if (st == PF_OK) st = enqueue_finish(h, replay ? h->rpU + t : h->U.get(), info, dmean + t * d, dcov + t * dd);
    if (st != PF_OK) {
      (void)hipStreamSynchronize(s);
      return st;
    }
  }
  std::vector<double> hi((size_t)T * 3);
  PF_HIPCHK(hipMemcpyAsync(hi.data(), dinfo, (size_t)T * 3 * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(means, dmean, (size_t)T * d * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(covs, dcov, (size_t)T * dd * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  h->rpT = -1;  // the draws are consumed
  for (int64_t t = 0; t < T; ++t) {
    if (hi[3 * t + 2] != 0.0) return fail(PF_E_NAN, "no particle has a finite positive weight at step " + std::to_string(t));
    if (ess) ess[t] = hi[3 * t];
    if (flags) flags[t] = hi[3 * t + 1] != 0.0 ? 1 : 0;
  }
  h->initialised = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_run"); }

pf_status pf_ledh_dense_step(pf_edh_dense_handle* h, const double* P, const double* R_diag, const double* z,
                             const double* u, int32_t n_lambda, int32_t noise, const double* v, pf_ledh_info* info,
                             double* eta0_trace) try {
  if (!h || !P || !R_diag || !z) return fail(PF_E_ARG, "null argument");
  pf::LedhDensePlan plan{};
  pf_status st = ledh_check(h, R_diag, n_lambda, noise, &plan);
  if (st != PF_OK) return st;
  if (noise == PF_NOISE_HOST && !v) return fail(PF_E_ARG, "PF_NOISE_HOST needs v");
  if (!h->initialised) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  if (h->pending) return fail(PF_E_ARG, "a step is pending: call pf_edh_dense_finish first");
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d;
  st = ledh_prepare(h, plan, R_diag, n_lambda, eta0_trace != nullptr);
  if (st != PF_OK) return st;
  PF_HIPCHK(hipMemcpyAsync(h->M, P, d * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->z, z, d * 8, hipMemcpyHostToDevice, s));
  if (u) PF_HIPCHK(hipMemcpyAsync(h->u, u, d * 8, hipMemcpyHostToDevice, s));
  if (noise == PF_NOISE_HOST) PF_HIPCHK(hipMemcpyAsync(h->v, v, (size_t)h->N * d * 8, hipMemcpyHostToDevice, s));
  const double* du = u ? h->u.get() : nullptr;
  const double* dv = noise == PF_NOISE_HOST ? h->v.get() : nullptr;
  st = enqueue_flow(h, plan, h->M, h->z, du, dv, n_lambda, h->lnfail, eta0_trace ? h->trace.get() : nullptr);
  if (st == PF_OK) st = enqueue_weights(h, h->z, du, dv, h->theta, h->info);
  if (st != PF_OK) return st;
  double hi[3] = {0.0, 0.0, 0.0};
  int nfail = 0;
  PF_HIPCHK(hipMemcpyAsync(hi, h->info, sizeof(hi), hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(&nfail, h->lnfail, sizeof(int), hipMemcpyDeviceToHost, s));
  if (eta0_trace)
    PF_HIPCHK(hipMemcpyAsync(eta0_trace, h->trace, (size_t)n_lambda * d * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  if (nfail != 0) {  // X and w are untouched: the state before the step is kept
    std::vector<int> f((size_t)h->N);
    PF_HIPCHK(hipMemcpy(f.data(), h->lfail, f.size() * sizeof(int), hipMemcpyDeviceToHost));
    const int64_t first = std::find(f.begin(), f.end(), 1) - f.begin();
    return fail(PF_E_NOT_PD, "Matrix is not positive definite (S of " + std::to_string(nfail) +
                                 " particles, the first is particle " + std::to_string(first) + ")");
  }
  if (hi[2] != 0.0) return fail(PF_E_NAN, "no particle has a finite positive weight");
  h->pending = true;
  h->last_flag = hi[1] != 0.0 ? 1 : 0;
  if (info) {
    info->ess = hi[0];
    info->resample = h->last_flag;
  }
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ledh_dense_step"); }

pf_status pf_ledh_dense_run(pf_edh_dense_handle* h, const double* Ps, const double* R_diag, const double* Z,
                            const double* U, int64_t T, int32_t n_lambda, int32_t noise, double* means, double* covs,
                            double* ess, uint8_t* flags) try {
  if (!h || !Ps || !R_diag || !Z || !means || !covs) return fail(PF_E_ARG, "null argument");
  if (T < 1 || T > (1 << 20)) return fail(PF_E_ARG, "T out of range");
  pf::LedhDensePlan plan{};
  pf_status st = ledh_check(h, R_diag, n_lambda, noise, &plan);
  if (st != PF_OK) return st;
  if (!h->initialised) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  if (h->pending) return fail(PF_E_ARG, "a step is pending: call pf_edh_dense_finish first");
  if (h->rpT != T && (h->ratio > 0.0 || noise == PF_NOISE_HOST))
    return fail(PF_E_ARG, "pf_edh_dense_set_run_replay must give the draws of a run of exactly this T");
  if (noise == PF_NOISE_HOST && !h->rp_has_v) return fail(PF_E_ARG, "PF_NOISE_HOST needs the replayed V");
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t d = (size_t)h->d, dd = d * d, nd = (size_t)h->N * d;
  st = ledh_prepare(h, plan, R_diag, n_lambda, false);
  if (st != PF_OK) return st;
  DevBuf<double> dP, dZ, dU, dmean, dcov, dinfo;
  DevBuf<int> dnfail;
  PF_HIPCHK(dP.alloc((size_t)T * dd));
  PF_HIPCHK(dZ.alloc((size_t)T * d));
  if (U) PF_HIPCHK(dU.alloc((size_t)T * d));
  PF_HIPCHK(dmean.alloc((size_t)T * d));
  PF_HIPCHK(dcov.alloc((size_t)T * dd));
  PF_HIPCHK(dinfo.alloc((size_t)T * 3));
  PF_HIPCHK(dnfail.alloc((size_t)T));
  PF_HIPCHK(hipMemcpyAsync(dP, Ps, (size_t)T * dd * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(dZ, Z, (size_t)T * d * 8, hipMemcpyHostToDevice, s));
  if (U) PF_HIPCHK(hipMemcpyAsync(dU, U, (size_t)T * d * 8, hipMemcpyHostToDevice, s));
  h->initialised = false;  // a failure inside the run leaves the handle uninitialised
  const bool replay = h->rpT == T;
  for (int64_t t = 0; t < T; ++t) {
    double* info = dinfo + 3 * t;
    const double* du = U ? dU + t * d : nullptr;
    const double* dv = noise == PF_NOISE_HOST ? h->rpV + t * nd : nullptr;
    st = enqueue_flow(h, plan, dP + t * dd, dZ + t * d, du, dv, n_lambda, dnfail + t, nullptr);
    if (st == PF_OK) st = enqueue_weights(h, dZ + t * d, du, dv, h->theta, info);
    if (st == PF_OK) st = enqueue_finish(h, replay ? h->rpU + t : h->U.get(), info, dmean + t * d, dcov + t * dd);
    if (st != PF_OK) {
      (void)hipStreamSynchronize(s);
      return st;
    }
  }
  std::vector<double> hi((size_t)T * 3);
  std::vector<int> nf((size_t)T);
  PF_HIPCHK(hipMemcpyAsync(hi.data(), dinfo, (size_t)T * 3 * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(nf.data(), dnfail, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(means, dmean, (size_t)T * d * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(covs, dcov, (size_t)T * dd * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  h->rpT = -1;  // the draws are consumed
  for (int64_t t = 0; t < T; ++t) {
    if (nf[(size_t)t] != 0)
      return fail(PF_E_NOT_PD, "Matrix is not positive definite (S of " + std::to_string(nf[(size_t)t]) +
                                   " particles at step " + std::to_string(t) + ")");
    if (hi[3 * t + 2] != 0.0) return fail(PF_E_NAN, "no particle has a finite positive weight at step " + std::to_string(t));
    if (ess) ess[t] = hi[3 * t];
    if (flags) flags[t] = hi[3 * t + 1] != 0.0 ? 1 : 0;
  }
  h->initialised = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ledh_dense_run"); }

void* pf_edh_dense_stream(pf_edh_dense_handle* h) { return h ? (void*)h->stream : nullptr; }

pf_status pf_edh_dense_synchronize(pf_edh_dense_handle* h) try {
  if (!h) return fail(PF_E_ARG, "null handle");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_edh_dense_synchronize"); }

}  // extern "C"
