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
#include <memory>
#include <string>
#include <vector>

#include "../../include/pf_kpf.h"
#include "pf_hooks.h"
#include "pf_host.h"
#include "pf_kpf_kernels.h"

namespace pf {
namespace kpf {

constexpr int MAXDIM = 1024;

static bool model_ok(int nx, int nz, int ok) {
  if (nx < 1 || nz < 1 || nx > MAXDIM || nz > MAXDIM) return false;
  if (ok == PF_OBS_LINEAR) return true;
  if (ok == PF_OBS_EXP_HALF) return nz == nx;
  if (ok == PF_OBS_ACOUSTIC) return nx % 4 == 0;
  return false;
}

// inverse of a symmetric positive definite matrix through its Cholesky factor; false if not PD.
// Not pf::spd_inverse: this symmetrises A and forms L^-T L^-1, which rounds differently (KPF's bits).
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
using pf::DevBuf;
using pf::fail;

struct pf_kpf_handle {
  int N = 0, Npad = 0, nx = 0, nz = 0, ok = 0, kernel = 0, device = 0;
  // all-pairs geometry, fixed by (N, nx, kernel): the split count is part of the summation order
  int bs = 64, tiles = 1, S = 1, chunk = 0, TM = 4;
  pf::Stream stream;  // before the buffers: destroyed after them
  DevBuf<double> xa, xb, G, gsum, rw, zw, U, V, W, part, aos, op, Rinv, y, x0, B, Binv, ell, ds;
  DevBuf<int32_t> nclip;
  int64_t steps_cap = 0;
  ~pf_kpf_handle() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

extern "C" {

int32_t pf_kpf_model_supported(int32_t nx, int32_t nz, int32_t ok) { return model_ok(nx, nz, ok) ? 1 : 0; }

pf_status pf_kpf_create(const pf_model_desc* m, const pf_kpf_opts* o, pf_kpf_handle** out) try {
  if (!m || !o || !out) return fail(PF_E_ARG, "null argument");
  *out = nullptr;
  if (o->n_particles < 1) return fail(PF_E_ARG, "n_particles must be positive");
  if (o->n_particles > (int64_t)1 << 24) return fail(PF_E_ARG, "n_particles too large (max 16777216)");
  if (o->kernel_type != PF_KPF_DIAGONAL && o->kernel_type != PF_KPF_SCALAR)
    return fail(PF_E_ARG, "bad kernel_type (PF_KPF_DIAGONAL or PF_KPF_SCALAR)");
  const int nx = m->nx, nz = m->nz, ok = m->obs_kind;
  if (!model_ok(nx, nz, ok))
    return fail(PF_E_UNSUPPORTED, "KPF observation (nx=" + std::to_string(nx) + ", nz=" + std::to_string(nz) +
                                       ", h=" + std::to_string(ok) +
                                       ") is not supported: PF_OBS_LINEAR, PF_OBS_EXP_HALF (nz == nx) or "
                                       "PF_OBS_ACOUSTIC (nx = 4 C), dimensions up to 1024");
  const int64_t need = ok == PF_OBS_LINEAR ? (int64_t)nz * nx + nz : ok == PF_OBS_EXP_HALF ? nz : 2 + 2 * (int64_t)nz;
  if (!m->obs_params || m->n_obs_params < need) return fail(PF_E_ARG, "observation parameters missing or too short");
  if (!m->R) return fail(PF_E_ARG, "R is required");
  std::vector<double> Ri;
  if (!spd_inv(m->R, nz, Ri)) return fail(PF_E_NOT_PD, "Matrix is not positive definite (R)");

  PF_HIPCHK(hipSetDevice(o->device));
  std::unique_ptr<pf_kpf_handle> h(new pf_kpf_handle());
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

  auto bail = [](const char* what) { return fail(PF_E_HIP, std::string("hipMalloc failed: ") + what); };
  if (hipStreamCreateWithFlags(h->stream.out(), hipStreamNonBlocking) != hipSuccess) return bail("stream");
  const size_t xn = (size_t)nx * h->Npad, zn = (size_t)nz * h->Npad;  // doubles
  const size_t xbytes = xn * 8;
  const size_t pn = (size_t)h->S * (h->kernel == PF_KPF_DIAGONAL ? nx : 1) * h->Npad;
  struct A { DevBuf<double>* p; size_t n; };
  A allocs[] = {{&h->xa, xn}, {&h->xb, xn}, {&h->G, xn}, {&h->U, xn}, {&h->V, xn}, {&h->W, xn},
                {&h->gsum, (size_t)h->Npad}, {&h->rw, zn}, {&h->zw, zn}, {&h->part, pn}, {&h->aos, (size_t)N * nx},
                {&h->op, (size_t)need}, {&h->Rinv, (size_t)nz * nz}, {&h->y, (size_t)nz}, {&h->x0, (size_t)nx},
                {&h->B, (size_t)nx * nx}, {&h->Binv, (size_t)nx * nx}, {&h->ell, (size_t)nx}};
  for (auto& a : allocs)
    if (a.p->alloc(a.n) != hipSuccess) return bail("state");
  // the pad lanes [N, Npad) of the ensembles are never written or read; zero them all the same
  if (hipMemset(h->xa, 0, xbytes) != hipSuccess || hipMemset(h->xb, 0, xbytes) != hipSuccess ||
      hipMemcpy(h->op, m->obs_params, (size_t)need * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->Rinv, Ri.data(), Ri.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return bail("upload");
  if (hipDeviceSynchronize() != hipSuccess) return bail("upload");
  *out = h.release();
  return PF_OK;
} catch (...) { return pf::on_exception("pf_kpf_create"); }

void pf_kpf_destroy(pf_kpf_handle* h) { delete h; }

pf_status pf_kpf_analyze(pf_kpf_handle* h, const double* X, const double* y, const double* x0, const double* B,
                         const double* B_inv, const double* lengthscales, const double* ds, int64_t n_steps,
                         double c_move_max, double* X_out, int32_t* n_clipped) try {
  if (!h || !X || !y || !x0 || !B || !B_inv || !lengthscales || !X_out) return fail(PF_E_ARG, "null argument");
  if (n_steps < 0 || n_steps > (1 << 20)) return fail(PF_E_ARG, "n_steps out of range");
  if (n_steps > 0 && !ds) return fail(PF_E_ARG, "null argument (ds)");
  PF_HIPCHK(hipSetDevice(h->device));
  const int N = h->N, nx = h->nx, nz = h->nz;
  hipStream_t s = h->stream;
  if (n_steps > h->steps_cap) {  // before the launch sequence starts
    PF_HIPCHK(hipStreamSynchronize(s));
    h->steps_cap = 0;
    PF_HIPCHK(h->ds.alloc((size_t)n_steps));
    PF_HIPCHK(h->nclip.alloc((size_t)n_steps));
    h->steps_cap = n_steps;
  }
  const size_t ebytes = (size_t)N * nx * 8;
  PF_HIPCHK(hipMemcpyAsync(h->aos, X, ebytes, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->y, y, (size_t)nz * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->x0, x0, (size_t)nx * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->B, B, (size_t)nx * nx * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->Binv, B_inv, (size_t)nx * nx * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->ell, lengthscales, (size_t)nx * 8, hipMemcpyHostToDevice, s));
  if (n_steps > 0) {
    PF_HIPCHK(hipMemcpyAsync(h->ds, ds, (size_t)n_steps * 8, hipMemcpyHostToDevice, s));
    PF_HIPCHK(hipMemsetAsync(h->nclip, 0, (size_t)n_steps * sizeof(int32_t), s));
  }
  Params p{N, h->Npad, nx, nz, h->ok, h->op, h->Rinv, h->y, h->x0, h->B, h->Binv, h->ell};
  const unsigned eg = (unsigned)(((int64_t)N * nx + PB - 1) / PB), pg = (unsigned)((N + PB - 1) / PB);
  double *cur = h->xa, *nxt = h->xb;
  hipLaunchKernelGGL(k_kpf_load, dim3(eg), dim3(PB), 0, s, h->aos, cur, N, h->Npad, nx);
  PF_HIPCHK(hipGetLastError());
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
    PF_HIPCHK(hipGetLastError());
    std::swap(cur, nxt);
  }
  hipLaunchKernelGGL(k_kpf_store, dim3(eg), dim3(PB), 0, s, cur, h->aos, N, h->Npad, nx);
  PF_HIPCHK(hipGetLastError());
  PF_HIPCHK(hipMemcpyAsync(X_out, h->aos, ebytes, hipMemcpyDeviceToHost, s));
  if (n_clipped && n_steps > 0)
    PF_HIPCHK(hipMemcpyAsync(n_clipped, h->nclip, (size_t)n_steps * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_kpf_analyze"); }

void* pf_kpf_stream(pf_kpf_handle* h) { return h ? (void*)h->stream : nullptr; }

pf_status pf_kpf_synchronize(pf_kpf_handle* h) try {
  if (!h) return fail(PF_E_ARG, "null handle");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_kpf_synchronize"); }

}  // extern "C"
