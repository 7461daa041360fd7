// Host side of the MI355X kernel particle flow filter: the C ABI of include/pf_kpf.h.
//
// Turns one KernelParticleFilter.analyze (models/kernel_particle_filter.py:324-447) into a single
// stream-ordered sequence of launches of pf_kpf_kernels.h: upload, then the score, all-pairs and
// update kernels per pseudo-time step over two ping-pong ensembles, then download.  The step sizes
// come in as an array (the schedule depends on the configuration only), so nothing inside the
// sequence waits for the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/pf_kpf.h"
#include "pf_hooks.h"
#include "pf_kpf_kernels.h"

namespace pf {
// the engine's thread-local error message (pf_last_error, pf_engine.hip)
void set_last_error(const std::string& msg);
namespace kpf {
static pf_status kfail(pf_status code, const std::string& msg) {
  set_last_error(msg);
  return code;
}
#define KCHK(expr)                                                                                   \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return kfail(PF_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

constexpr int MAXDIM = 1024;

static bool model_ok(int nx, int nz, int ok) {
  if (nx < 1 || nz < 1 || nx > MAXDIM || nz > MAXDIM) return false;
  if (ok == PF_OBS_LINEAR) return true;
  if (ok == PF_OBS_EXP_HALF) return nz == nx;
  if (ok == PF_OBS_ACOUSTIC) return nx % 4 == 0;
  return false;
}

// inverse of a symmetric positive definite matrix through its Cholesky factor; false if not PD
static bool spd_inv(const double* A, int n, std::vector<double>& out) {
  std::vector<double> L((size_t)n * n, 0.0), Li((size_t)n * n, 0.0);
  for (int r = 0; r < n; ++r)
    for (int c = 0; c <= r; ++c) {
      double s = 0.5 * (A[(size_t)r * n + c] + A[(size_t)c * n + r]);
      for (int k = 0; k < c; ++k) s -= L[(size_t)r * n + k] * L[(size_t)c * n + k];
      if (r == c) {
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        L[(size_t)r * n + r] = std::sqrt(s);
      } else {
        L[(size_t)r * n + c] = s / L[(size_t)c * n + c];
      }
    }
  for (int c = 0; c < n; ++c)  // Li = L^-1, column by column
    for (int r = c; r < n; ++r) {
      double s = (r == c) ? 1.0 : 0.0;
      for (int k = c; k < r; ++k) s -= L[(size_t)r * n + k] * Li[(size_t)k * n + c];
      Li[(size_t)r * n + c] = s / L[(size_t)r * n + r];
    }
  out.assign((size_t)n * n, 0.0);
  for (int r = 0; r < n; ++r)  // A^-1 = Li^T Li
    for (int c = 0; c <= r; ++c) {
      double s = 0.0;
      for (int k = r; k < n; ++k) s += Li[(size_t)k * n + r] * Li[(size_t)k * n + c];
      out[(size_t)r * n + c] = out[(size_t)c * n + r] = s;
    }
  return true;
}

}  // namespace kpf
}  // namespace pf

using namespace pf::kpf;

struct pf_kpf_handle {
  int N = 0, Npad = 0, nx = 0, nz = 0, ok = 0, kernel = 0, device = 0;
  // all-pairs geometry, fixed by (N, nx, kernel): the split count is part of the summation order
  int bs = 64, tiles = 1, S = 1, chunk = 0, TM = 4;
  hipStream_t stream = nullptr;
  double *xa = nullptr, *xb = nullptr, *G = nullptr, *gsum = nullptr, *rw = nullptr, *zw = nullptr, *U = nullptr,
         *V = nullptr, *W = nullptr, *part = nullptr, *aos = nullptr, *op = nullptr, *Rinv = nullptr, *y = nullptr,
         *x0 = nullptr, *B = nullptr, *Binv = nullptr, *ell = nullptr, *ds = nullptr;
  int32_t* nclip = nullptr;
  int64_t steps_cap = 0;
};

extern "C" {

int32_t pf_kpf_model_supported(int32_t nx, int32_t nz, int32_t ok) { return model_ok(nx, nz, ok) ? 1 : 0; }

pf_status pf_kpf_create(const pf_model_desc* m, const pf_kpf_opts* o, pf_kpf_handle** out) {
  if (!m || !o || !out) return kfail(PF_E_ARG, "null argument");
  *out = nullptr;
  if (o->n_particles < 1) return kfail(PF_E_ARG, "n_particles must be positive");
  if (o->n_particles > (int64_t)1 << 24) return kfail(PF_E_ARG, "n_particles too large (max 16777216)");
  if (o->kernel_type != PF_KPF_DIAGONAL && o->kernel_type != PF_KPF_SCALAR)
    return kfail(PF_E_ARG, "bad kernel_type (PF_KPF_DIAGONAL or PF_KPF_SCALAR)");
  const int nx = m->nx, nz = m->nz, ok = m->obs_kind;
  if (!model_ok(nx, nz, ok))
    return kfail(PF_E_UNSUPPORTED, "KPF observation (nx=" + std::to_string(nx) + ", nz=" + std::to_string(nz) +
                                       ", h=" + std::to_string(ok) +
                                       ") is not supported: PF_OBS_LINEAR, PF_OBS_EXP_HALF (nz == nx) or "
                                       "PF_OBS_ACOUSTIC (nx = 4 C), dimensions up to 1024");
  const int64_t need = ok == PF_OBS_LINEAR ? (int64_t)nz * nx + nz : ok == PF_OBS_EXP_HALF ? nz : 2 + 2 * (int64_t)nz;
  if (!m->obs_params || m->n_obs_params < need) return kfail(PF_E_ARG, "observation parameters missing or too short");
  if (!m->R) return kfail(PF_E_ARG, "R is required");
  std::vector<double> Ri;
  if (!spd_inv(m->R, nz, Ri)) return kfail(PF_E_NOT_PD, "Matrix is not positive definite (R)");

  KCHK(hipSetDevice(o->device));
  pf_kpf_handle* h = new pf_kpf_handle();
  h->N = (int)o->n_particles;
  h->Npad = (h->N + 63) / 64 * 64;
  h->nx = nx; h->nz = nz; h->ok = ok;
  h->kernel = o->kernel_type;
  h->device = o->device;
  const int N = h->N;
  // Small ensembles still have to occupy the chip (256 CUs x 4 SIMDs): 64-lane workgroups, and the
  // m range split until about 8 waves per SIMD are in flight.
  int waves;
  if (h->kernel == PF_KPF_DIAGONAL) {
    h->bs = N <= 2048 ? 64 : 256;
    h->tiles = (N + h->bs - 1) / h->bs;
    waves = h->tiles * nx * (h->bs / 64);
  } else {
    h->bs = 64;
    h->tiles = (N + 63) / 64;
    waves = h->tiles;
    h->TM = 64;
    while (h->TM > 4 && (size_t)(nx + 1) * h->TM * 8 > 48 * 1024) h->TM /= 2;
  }
  int S = std::min({(N + MGRAIN - 1) / MGRAIN, std::max(1, 8192 / waves), MAXS});
  h->chunk = ((N + S - 1) / S + MGRAIN - 1) / MGRAIN * MGRAIN;
  h->S = (N + h->chunk - 1) / h->chunk;

  auto bail = [&](const char* what) {
    pf_kpf_destroy(h);
    return kfail(PF_E_HIP, std::string("hipMalloc failed: ") + what);
  };
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return bail("stream");
  const size_t xbytes = (size_t)nx * h->Npad * 8, zbytes = (size_t)nz * h->Npad * 8;
  const size_t pbytes = (size_t)h->S * (h->kernel == PF_KPF_DIAGONAL ? nx : 1) * h->Npad * 8;
  struct A { double** p; size_t b; };
  A allocs[] = {{&h->xa, xbytes}, {&h->xb, xbytes}, {&h->G, xbytes}, {&h->U, xbytes}, {&h->V, xbytes},
                {&h->W, xbytes}, {&h->gsum, (size_t)h->Npad * 8}, {&h->rw, zbytes}, {&h->zw, zbytes}, {&h->part, pbytes},
                {&h->aos, (size_t)N * nx * 8}, {&h->op, (size_t)need * 8}, {&h->Rinv, (size_t)nz * nz * 8},
                {&h->y, (size_t)nz * 8}, {&h->x0, (size_t)nx * 8}, {&h->B, (size_t)nx * nx * 8},
                {&h->Binv, (size_t)nx * nx * 8}, {&h->ell, (size_t)nx * 8}};
  for (auto& a : allocs)
    if (hipMalloc((void**)a.p, a.b) != hipSuccess) return bail("state");
  // the pad lanes [N, Npad) of the ensembles are never written or read; zero them all the same
  if (hipMemset(h->xa, 0, xbytes) != hipSuccess || hipMemset(h->xb, 0, xbytes) != hipSuccess ||
      hipMemcpy(h->op, m->obs_params, (size_t)need * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->Rinv, Ri.data(), Ri.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return bail("upload");
  if (hipDeviceSynchronize() != hipSuccess) return bail("upload");
  *out = h;
  return PF_OK;
}

void pf_kpf_destroy(pf_kpf_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (double* p : {h->xa, h->xb, h->G, h->gsum, h->rw, h->zw, h->U, h->V, h->W, h->part, h->aos, h->op, h->Rinv, h->y,
                    h->x0, h->B, h->Binv, h->ell, h->ds})
    if (p) (void)hipFree(p);
  if (h->nclip) (void)hipFree(h->nclip);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

pf_status pf_kpf_analyze(pf_kpf_handle* h, const double* X, const double* y, const double* x0, const double* B,
                         const double* B_inv, const double* lengthscales, const double* ds, int64_t n_steps,
                         double c_move_max, double* X_out, int32_t* n_clipped) {
  if (!h || !X || !y || !x0 || !B || !B_inv || !lengthscales || !X_out) return kfail(PF_E_ARG, "null argument");
  if (n_steps < 0 || n_steps > (1 << 20)) return kfail(PF_E_ARG, "n_steps out of range");
  if (n_steps > 0 && !ds) return kfail(PF_E_ARG, "null argument (ds)");
  KCHK(hipSetDevice(h->device));
  const int N = h->N, nx = h->nx, nz = h->nz;
  hipStream_t s = h->stream;
  if (n_steps > h->steps_cap) {  // before the launch sequence starts
    KCHK(hipStreamSynchronize(s));
    if (h->ds) (void)hipFree(h->ds);
    if (h->nclip) (void)hipFree(h->nclip);
    h->ds = nullptr; h->nclip = nullptr; h->steps_cap = 0;
    KCHK(hipMalloc((void**)&h->ds, (size_t)n_steps * 8));
    KCHK(hipMalloc((void**)&h->nclip, (size_t)n_steps * sizeof(int32_t)));
    h->steps_cap = n_steps;
  }
  const size_t ebytes = (size_t)N * nx * 8;
  KCHK(hipMemcpyAsync(h->aos, X, ebytes, hipMemcpyHostToDevice, s));
  KCHK(hipMemcpyAsync(h->y, y, (size_t)nz * 8, hipMemcpyHostToDevice, s));
  KCHK(hipMemcpyAsync(h->x0, x0, (size_t)nx * 8, hipMemcpyHostToDevice, s));
  KCHK(hipMemcpyAsync(h->B, B, (size_t)nx * nx * 8, hipMemcpyHostToDevice, s));
  KCHK(hipMemcpyAsync(h->Binv, B_inv, (size_t)nx * nx * 8, hipMemcpyHostToDevice, s));
  KCHK(hipMemcpyAsync(h->ell, lengthscales, (size_t)nx * 8, hipMemcpyHostToDevice, s));
  if (n_steps > 0) {
    KCHK(hipMemcpyAsync(h->ds, ds, (size_t)n_steps * 8, hipMemcpyHostToDevice, s));
    KCHK(hipMemsetAsync(h->nclip, 0, (size_t)n_steps * sizeof(int32_t), s));
  }
  Params p{N, h->Npad, nx, nz, h->ok, h->op, h->Rinv, h->y, h->x0, h->B, h->Binv, h->ell};
  const unsigned eg = (unsigned)(((int64_t)N * nx + PB - 1) / PB), pg = (unsigned)((N + PB - 1) / PB);
  double *cur = h->xa, *nxt = h->xb;
  hipLaunchKernelGGL(k_kpf_load, dim3(eg), dim3(PB), 0, s, h->aos, cur, N, h->Npad, nx);
  KCHK(hipGetLastError());
  const unsigned cg = (unsigned)((N + CB - 1) / CB);
  const int scalar = h->kernel == PF_KPF_SCALAR ? 1 : 0;
  for (int64_t k = 0; k < n_steps; ++k) {
    hipLaunchKernelGGL(k_kpf_resid, dim3(cg, nz), dim3(CB), 0, s, p, cur, h->rw);
    hipLaunchKernelGGL(k_kpf_rinv, dim3(cg, nz), dim3(CB), 0, s, p, h->rw, h->zw);
    hipLaunchKernelGGL(k_kpf_score, dim3(cg, nx), dim3(CB), 0, s, p, cur, h->zw, h->G);
    if (scalar) hipLaunchKernelGGL(k_kpf_gsum, dim3(pg), dim3(PB), 0, s, h->G, h->gsum, N, h->Npad, nx);
    pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
    if (h->kernel == PF_KPF_DIAGONAL)
      hipLaunchKernelGGL(k_kpf_pairs_diag, dim3(h->tiles, nx, h->S), dim3(h->bs), (size_t)h->bs * sizeof(double2), s,
                         cur, h->G, h->ell, h->part, N, h->Npad, nx, h->chunk);
    else
      hipLaunchKernelGGL(k_kpf_pairs_scalar, dim3(h->tiles, h->S), dim3(h->bs), (size_t)(nx + 1) * h->TM * 8, s, cur,
                         h->gsum, h->ell, h->part, N, h->Npad, nx, h->chunk, h->TM);
    hipLaunchKernelGGL(k_kpf_combine, dim3(cg, nx), dim3(CB), 0, s, h->part, h->S, scalar, h->U, N, h->Npad, nx);
    hipLaunchKernelGGL(k_kpf_matvec, dim3(cg, nx), dim3(CB), 0, s, h->B, h->U, h->V, (const double*)nullptr, (int)k, N,
                       h->Npad, nx);
    hipLaunchKernelGGL(k_kpf_matvec, dim3(cg, nx), dim3(CB), 0, s, h->Binv, h->V, h->W, h->ds, (int)k, N, h->Npad, nx);
    hipLaunchKernelGGL(k_kpf_move, dim3(pg), dim3(PB), 0, s, cur, nxt, h->V, h->W, h->ds, (int)k, c_move_max,
                       h->nclip, N, h->Npad, nx);
    KCHK(hipGetLastError());
    std::swap(cur, nxt);
  }
  hipLaunchKernelGGL(k_kpf_store, dim3(eg), dim3(PB), 0, s, cur, h->aos, N, h->Npad, nx);
  KCHK(hipGetLastError());
  KCHK(hipMemcpyAsync(X_out, h->aos, ebytes, hipMemcpyDeviceToHost, s));
  if (n_clipped && n_steps > 0)
    KCHK(hipMemcpyAsync(n_clipped, h->nclip, (size_t)n_steps * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  KCHK(hipStreamSynchronize(s));
  return PF_OK;
}

void* pf_kpf_stream(pf_kpf_handle* h) { return h ? (void*)h->stream : nullptr; }

pf_status pf_kpf_synchronize(pf_kpf_handle* h) {
  if (!h) return kfail(PF_E_ARG, "null handle");
  KCHK(hipSetDevice(h->device));
  KCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
}

}  // extern "C"
