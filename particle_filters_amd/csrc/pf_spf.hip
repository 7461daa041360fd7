// Host side of the MI355X stochastic particle flow filter: the C ABI of include/pf_spf.h.
//
// The handle owns the particles [N][n] on its device.  pf_spf_advance repacks the caller's
// per-step (A, c, G) into the kernel's layout (pf_spf_kernels.h SpfLayout), uploads it (and the
// host normals, when given) and runs every step in one launch of k_spf_advance<NP>.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pf_spf.h"
#include "pf_hooks.h"
#include "pf_host.h"
#include "pf_spf_kernels.h"

namespace pf {
namespace spf {

constexpr int MAXN = 64;
constexpr size_t LDS_BYTES = 160 * 1024;
constexpr int64_t MAX_STEPS = 1 << 20;

static bool dim_ok(int n) { return n >= 1 && n <= MAXN; }

// Workgroup size: the largest of 256 / 128 / 64 lanes whose state tile fits the LDS beside the two
// parameter buffers (256 up to n = 48, 128 up to n = 61, 64 above), halved further while that
// leaves fewer than 512 workgroups (two per CU).  The geometry cannot change a result.
static int block_size(int64_t N, int n) {
  const SpfLayout L(n);
  int bs = 256;
  while (bs > 64 && (2 * (size_t)L.size() + (size_t)L.NP * bs) * 8 > LDS_BYTES) bs /= 2;
  while (bs > 64 && (N + bs - 1) / bs < 512) bs /= 2;
  return bs;
}

template <int NP>
static hipError_t launch_np(bool* attr_set, int NPwant, dim3 grid, dim3 block, size_t lds, hipStream_t s, double* X,
                            const double* P, const double* Z, int64_t N, int n, int n_steps, uint32_t epoch0, uint64_t seed) {
  if constexpr (NP > MAXN) {
    return hipErrorInvalidValue;
  } else {
    if (NP != NPwant)
      return launch_np<NP + 4>(attr_set, NPwant, grid, block, lds, s, X, P, Z, N, n, n_steps, epoch0, seed);
    if (!*attr_set) {  // once per handle: the handle has one n, hence one NP
      hipError_t e = hipFuncSetAttribute((const void*)k_spf_advance<NP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)LDS_BYTES);
      if (e != hipSuccess) return e;
      *attr_set = true;
    }
    pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
    hipLaunchKernelGGL(k_spf_advance<NP>, grid, block, lds, s, X, P, Z, N, n, n_steps, epoch0, seed);
    return hipGetLastError();
  }
}

}  // namespace spf
}  // namespace pf

using namespace pf::spf;
using pf::DevBuf;
using pf::fail;

struct pf_spf_handle {
  int64_t N = 0;
  int n = 0, device = 0;
  pf::Stream stream;  // before the buffers: destroyed after them
  DevBuf<double> X, P, Z, m0, L0;
  size_t p_cap = 0, z_cap = 0;  // doubles
  bool attr_set = false;        // the step kernel's dynamic-LDS limit has been raised
  std::vector<double> pack;
  ~pf_spf_handle() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

extern "C" {

int32_t pf_spf_supported(int32_t n) { return dim_ok(n) ? 1 : 0; }

pf_status pf_spf_create(const pf_spf_opts* o, pf_spf_handle** out) try {
  if (!o || !out) return fail(PF_E_ARG, "null argument");
  *out = nullptr;
  if (o->n_particles < 1) return fail(PF_E_ARG, "n_particles must be positive");
  if (!dim_ok(o->n))
    return fail(PF_E_UNSUPPORTED, "stochastic particle flow: n=" + std::to_string(o->n) + " is not supported (1 <= n <= 64)");
  const SpfLayout L(o->n);
  if (o->n_particles > (((int64_t)1 << 32) - 1) / L.NB)
    return fail(PF_E_ARG, "n_particles too large: N * ceil(n / 4) must stay below 2^32 (Philox group index)");
  PF_HIPCHK(hipSetDevice(o->device));
  std::unique_ptr<pf_spf_handle> h(new pf_spf_handle());
  h->N = o->n_particles;
  h->n = o->n;
  h->device = o->device;
  auto bail = [](const char* what) { return fail(PF_E_HIP, std::string("pf_spf_create failed: ") + what); };
  const size_t xcount = (size_t)h->N * h->n;
  if (hipStreamCreateWithFlags(h->stream.out(), hipStreamNonBlocking) != hipSuccess) return bail("stream");
  if (h->X.alloc(xcount) != hipSuccess) return bail("hipMalloc particles");
  if (h->m0.alloc((size_t)h->n) != hipSuccess) return bail("hipMalloc m0");
  if (h->L0.alloc((size_t)h->n * h->n) != hipSuccess) return bail("hipMalloc L0");
  if (hipMemset(h->X, 0, xcount * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return bail("hipMemset");
  *out = h.release();
  return PF_OK;
} catch (...) { return pf::on_exception("pf_spf_create"); }

void pf_spf_destroy(pf_spf_handle* h) { delete h; }

pf_status pf_spf_set_particles(pf_spf_handle* h, const double* X) try {
  if (!h || !X) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipMemcpyAsync(h->X, X, (size_t)h->N * h->n * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_spf_set_particles"); }

pf_status pf_spf_get_particles(pf_spf_handle* h, double* X_out) try {
  if (!h || !X_out) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipMemcpyAsync(X_out, h->X, (size_t)h->N * h->n * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_spf_get_particles"); }

pf_status pf_spf_draw_prior(pf_spf_handle* h, const double* m0, const double* L0, uint64_t seed) try {
  if (!h || !m0 || !L0) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  PF_HIPCHK(hipMemcpyAsync(h->m0, m0, (size_t)h->n * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->L0, L0, (size_t)h->n * h->n * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_spf_prior, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, s, h->X, h->m0, h->L0, h->N, h->n,
                     seed);
  PF_HIPCHK(hipGetLastError());
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_spf_draw_prior"); }

pf_status pf_spf_advance(pf_spf_handle* h, const double* params, int64_t k0, int64_t n_steps, uint64_t seed,
                         const double* Z) try {
  if (!h) return fail(PF_E_ARG, "null handle");
  if (n_steps < 0 || n_steps > MAX_STEPS) return fail(PF_E_ARG, "n_steps out of range");
  if (k0 < 0 || k0 + n_steps >= ((int64_t)1 << 32)) return fail(PF_E_ARG, "k0 out of range (the epoch is 32 bits)");
  if (n_steps == 0) return PF_OK;
  if (!params) return fail(PF_E_ARG, "null argument (params)");
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int n = h->n;
  const int64_t N = h->N;
  const SpfLayout L(n);
  const size_t PB = (size_t)L.size(), pneed = PB * (size_t)n_steps;
  const size_t zneed = Z ? (size_t)n_steps * (size_t)N * n : 0;
  if (pneed > h->p_cap || zneed > h->z_cap) PF_HIPCHK(hipStreamSynchronize(s));  // before a buffer is replaced
  if (pneed > h->p_cap) {
    h->p_cap = 0;
    PF_HIPCHK(h->P.alloc(pneed));
    h->p_cap = pneed;
  }
  if (zneed > h->z_cap) {
    h->z_cap = 0;
    PF_HIPCHK(h->Z.alloc(zneed));
    h->z_cap = zneed;
  }
  // host layout [A n x n | c n | G n x n] -> SpfLayout
  h->pack.assign(pneed, 0.0);
  const size_t hstride = (size_t)2 * n * n + n;
  for (int64_t k = 0; k < n_steps; ++k) {
    const double *A = params + (size_t)k * hstride, *c = A + (size_t)n * n, *G = c + n;
    double* d = h->pack.data() + (size_t)k * PB;
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) d[L.at(j, i)] = A[(size_t)i * n + j];
    for (int i = 0; i < n; ++i) d[L.c0() + i] = c[i];
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= i; ++j) d[L.gblock(i / 4, j / 4) + 4 * (j % 4) + i % 4] = G[(size_t)i * n + j];
  }
  PF_HIPCHK(hipMemcpyAsync(h->P, h->pack.data(), pneed * 8, hipMemcpyHostToDevice, s));
  if (Z) PF_HIPCHK(hipMemcpyAsync(h->Z, Z, zneed * 8, hipMemcpyHostToDevice, s));
  const int bs = block_size(N, n);
  const size_t lds = (2 * PB + (size_t)L.NP * bs) * 8;
  if (lds > LDS_BYTES) return fail(PF_E_UNSUPPORTED, "parameter buffers do not fit the LDS");
  const hipError_t e = launch_np<4>(&h->attr_set, L.NP, dim3((unsigned)((N + bs - 1) / bs)), dim3(bs), lds, s, h->X, h->P,
                                    Z ? h->Z : nullptr, N, n, (int)n_steps, (uint32_t)(k0 + 1), seed);
  if (e != hipSuccess) return fail(PF_E_HIP, std::string("k_spf_advance: ") + hipGetErrorString(e));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_spf_advance"); }

int32_t pf_spf_workgroup(pf_spf_handle* h) { return h ? block_size(h->N, h->n) : 0; }

void* pf_spf_stream(pf_spf_handle* h) { return h ? (void*)h->stream : nullptr; }

pf_status pf_spf_synchronize(pf_spf_handle* h) try {
  if (!h) return fail(PF_E_ARG, "null handle");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_spf_synchronize"); }

}  // extern "C"
