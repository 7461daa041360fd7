// Host side of the MI355X soft (Gumbel-Softmax) resampler: the pf_soft_* entries of
// include/pf_engine.h.
//
// Turns one soft-resampling step (models/DPF_soft_resampling.py:309-334, 348-350) for B problems
// into a stream-ordered sequence of launches of pf_soft_kernels.h: upload, the all-pairs pass over
// every component chunk and source split, the merge, on request the entropy pass and its merge,
// download.  The split of the source range is fixed by N when the handle is made: it is part of
// the summation order.  pf_soft_backward is the backward pass of such a step: upload, r, the
// transposed all-pairs pass over every component chunk and row split (the same split), the merge,
// glp, download.  The launches of each pass are one enqueue_* function on device pointers and a
// stream: the host entries call it on the handle's staging buffers and stream, between their copies,
// the *_dev entries on the caller's pointers and stream, with no copies.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pf_engine.h"
#include "pf_dpf_host.h"
#include "pf_soft_kernels.h"

using namespace pf::soft;
namespace dpf = pf::dpf;
using pf::DevBuf;
using pf::fail;

constexpr int64_t MAXDRAWS = (int64_t)1 << 31;  // B N N of pf_soft_draws

struct pf_soft_handle {
  int N = 0, Npad = 0, d = 0, B = 0, device = 0;
  dpf::Split split{1, 1, 0};  // of the source range, fixed by N
  pf::Stream stream;          // before the buffers: destroyed after them
  dpf::Fence fence;           // orders the entries, which may run on different streams
  DevBuf<double> Xin, lpin, pm, ps, part, rowM, rowL, hp, Xout, Hout;
  bool has_stats = false;  // rowM, rowL hold the row statistics of a completed forward pass
  // the backward pass (allocated by the first pf_soft_backward): the upstream gradient, the saved
  // forward results as the caller passed them, r, the partials [B][S][d + 1][Npad], the summed r
  // column and the results
  DevBuf<double> gin, sXo, sM, sL, br, bpart, bar, gX, glp;
  ~pf_soft_handle() { dpf::quiesce(device, stream, fence); }
};

// the all-pairs pass over every component chunk and source split, and the merge, on stream s:
// X, lp -> X_out, and rowM, rowL in the handle
static void enqueue_forward(pf_soft_handle* h, hipStream_t s, const Prob& p, double inv_T, const dpf::Poison& poison,
                            const double* X, const double* lp, double* X_out) {
  const int N = h->N, d = h->d, B = h->B, S = h->split.S;
  const dim3 pg(h->split.tiles, (d + PC - 1) / PC * S, B);
  poison();
  dpf::dispatch_nc(std::min(d, PC), [&](auto nc) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_soft_pass<decltype(nc)::value>), pg, dim3(CB), 0, s, p, X, lp, inv_T,
                       h->split.chunk, S, (double*)h->pm, (double*)h->ps, (double*)h->part);
  });
  const unsigned ng = (unsigned)((N + PB - 1) / PB);
  hipLaunchKernelGGL(k_soft_finish, dim3(ng, d, B), dim3(PB), 0, s, p, S, (const double*)h->pm, (const double*)h->ps,
                     (const double*)h->part, (double*)h->rowM, (double*)h->rowL, X_out);
}

// one resampling on stream s, every pointer device memory: X, lp -> X_out, on request the row entropies
static pf_status enqueue_resample(pf_soft_handle* h, hipStream_t s, const Prob& p, double inv_T, const double* X,
                                  const double* lp, double* X_out, double* H_out) {
  const int N = h->N, B = h->B, S = h->split.S;
  const dpf::Poison poison(s);  // tests only: in front of every launch that stages through LDS
  h->has_stats = false;  // until this call's results are complete
  enqueue_forward(h, s, p, inv_T, poison, X, lp, X_out);
  if (H_out) {
    const unsigned ng = (unsigned)((N + PB - 1) / PB);
    poison();
    hipLaunchKernelGGL(k_soft_entropy, dim3(h->split.tiles, S, B), dim3(CB), 0, s, p, lp, inv_T, h->split.chunk, S,
                       (const double*)h->rowM, (const double*)h->rowL, (double*)h->hp);
    hipLaunchKernelGGL(k_soft_entropy_finish, dim3(ng, B), dim3(PB), 0, s, p, S, (const double*)h->hp, H_out);
  }
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

// the scratch of the backward pass, on the first call
static pf_status ensure_bwd(pf_soft_handle* h) {
  if (h->bpart) return PF_OK;
  const size_t nX = (size_t)h->B * h->N * h->d, nR = (size_t)h->B * h->N;
  // bpart last: it marks the set complete
  return dpf::alloc_all({{&h->gin, nX}, {&h->sXo, nX}, {&h->sM, nR}, {&h->sL, nR}, {&h->br, nR}, {&h->bar, nR},
                         {&h->gX, nX}, {&h->glp, nR},
                         {&h->bpart, (size_t)h->B * h->split.S * (h->d + 1) * (size_t)h->Npad}},
                        "backward pass");
}

// one backward pass on stream s, every pointer device memory.  Xo, M, L [B][ldm] are the saved forward
// results, or null: the call runs the forward launches itself - never what an earlier call left in
// rowM, rowL
static pf_status enqueue_backward(pf_soft_handle* h, hipStream_t s, const Prob& p, double inv_T, const double* X,
                                  const double* lp, const double* Xo, const double* M, const double* L,
                                  const double* gin, double* gX, double* glp) {
  const int N = h->N, d = h->d, B = h->B, S = h->split.S;
  const dpf::Poison poison(s);  // tests only, as in enqueue_resample
  int ldm = N;
  if (!Xo) {
    h->has_stats = false;
    enqueue_forward(h, s, p, inv_T, poison, X, lp, h->Xout);
    Xo = h->Xout, M = h->rowM, L = h->rowL, ldm = h->Npad;
  }
  const unsigned ng = (unsigned)((N + PB - 1) / PB);
  hipLaunchKernelGGL(k_soft_bwd_rows, dim3(ng, B), dim3(PB), 0, s, p, gin, Xo, (double*)h->br);
  const dim3 pg(((N + 1) / 2 + CB - 1) / CB, (d + PC - 1) / PC * S, B);
  poison();
  dpf::dispatch_nc(std::min(d, PC), [&](auto nc) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_soft_bwd_pass<decltype(nc)::value>), pg, dim3(CB), 0, s, p, gin,
                       (const double*)h->br, lp, M, L, ldm, inv_T, h->split.chunk, S, (double*)h->bpart);
  });
  hipLaunchKernelGGL(k_soft_bwd_finish, dim3(ng, d + 1, B), dim3(PB), 0, s, p, S, (const double*)h->bpart, gX,
                     (double*)h->bar);
  hipLaunchKernelGGL(k_soft_bwd_glp, dim3(ng, B), dim3(PB), 0, s, p, inv_T, X, (const double*)gX,
                     (const double*)h->bar, glp);
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

extern "C" {

pf_status pf_soft_create(const pf_soft_opts* o, pf_soft_handle** out) try {
  if (!o || !out) return fail(PF_E_ARG, "null argument");
  *out = nullptr;
  if (pf_status st = dpf::check_shape(o->n_particles, true, o->dim)) return st;
  if (pf_status st = dpf::check_batch(o->batch)) return st;

  PF_HIPCHK(hipSetDevice(o->device));
  std::unique_ptr<pf_soft_handle> h(new pf_soft_handle());
  const int N = h->N = (int)o->n_particles;
  const int d = h->d = o->dim, B = h->B = o->batch;
  h->Npad = dpf::npad(N);
  h->device = o->device;
  // one 64-lane workgroup per 64 rows and a chunk of the sources (the pass is a chain of fp64 log
  // and exp calls per lane)
  h->split = dpf::make_split(N, pf::test_hook_int("PF_TEST_SOFT_SPLITS"));  // tests: 1 forces the unsplit order

  if (pf_status st = dpf::make_stream(h->stream)) return st;
  const size_t P = (size_t)h->Npad, BS = (size_t)B * h->split.S;
  const double pbytes = (double)BS * (double)d * (double)P * 8.0;
  if (pbytes > 9.0e18 || h->part.alloc(BS * d * P) != hipSuccess)
    return fail(PF_E_HIP, "hipMalloc failed: partial sums, " + std::to_string((unsigned long long)(pbytes / 1048576.0)) +
                              " MiB (" + std::to_string(B) + " x " + std::to_string(h->split.S) + " x " + std::to_string(d) +
                              " x " + std::to_string(P) + " doubles)");
  if (pf_status st = dpf::alloc_all({{&h->Xin, (size_t)B * N * d}, {&h->lpin, (size_t)B * N}, {&h->pm, BS * P},
                                     {&h->ps, BS * P}, {&h->rowM, (size_t)B * P}, {&h->rowL, (size_t)B * P},
                                     {&h->hp, BS * P}, {&h->Xout, (size_t)B * N * d}, {&h->Hout, (size_t)B * N}},
                                    "state"))
    return st;
  *out = h.release();
  return PF_OK;
} catch (...) { return pf::on_exception("pf_soft_create"); }

void pf_soft_destroy(pf_soft_handle* h) { delete h; }

pf_status pf_soft_resample(pf_soft_handle* h, const double* X, const double* log_probs, double temperature,
                           uint64_t seed, uint32_t epoch, uint32_t batch_base, double* X_out,
                           double* row_entropy) try {
  if (!h || !X || !log_probs || !X_out) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("temperature", temperature)) return st;
  if (pf_status st = dpf::check_base(batch_base, h->B)) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  const int N = h->N, d = h->d, B = h->B;
  hipStream_t s = h->stream;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  PF_HIPCHK(hipMemcpyAsync(h->Xin, X, (size_t)B * N * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->lpin, log_probs, (size_t)B * N * 8, hipMemcpyHostToDevice, s));
  const Prob p = make_prob(h->N, h->d, h->B, seed, epoch, batch_base);
  if (pf_status st = enqueue_resample(h, s, p, 1.0 / temperature, h->Xin, h->lpin, h->Xout,
                                      row_entropy ? (double*)h->Hout : nullptr))
    return st;
  PF_HIPCHK(hipMemcpyAsync(X_out, h->Xout, (size_t)B * N * d * 8, hipMemcpyDeviceToHost, s));
  if (row_entropy) PF_HIPCHK(hipMemcpyAsync(row_entropy, h->Hout, (size_t)B * N * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  h->has_stats = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_soft_resample"); }

pf_status pf_soft_resample_dev(pf_soft_handle* h, void* stream, const double* dX, const double* d_log_probs,
                               double temperature, uint64_t seed, uint32_t epoch, uint32_t batch_base,
                               double* dX_out, double* d_row_entropy, double* d_row_max, double* d_row_sum) try {
  if (!h || !dX || !d_log_probs || !dX_out) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("temperature", temperature)) return st;
  if (pf_status st = dpf::check_base(batch_base, h->B)) return st;
  if (!d_row_max != !d_row_sum) return fail(PF_E_ARG, "d_row_max and d_row_sum must be given together or both be null");
  const size_t N = (size_t)h->N, B = (size_t)h->B, P = (size_t)h->Npad, nX = B * N * h->d, nR = B * N;
  if (pf_status st = dpf::check_no_alias({{dX_out, nX}, {d_row_entropy, nR}, {d_row_max, nR}, {d_row_sum, nR}},
                                         {{dX, nX}, {d_log_probs, nR}}))
    return st;
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)h->stream;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  const Prob p = make_prob(h->N, h->d, h->B, seed, epoch, batch_base);
  if (pf_status st = enqueue_resample(h, s, p, 1.0 / temperature, dX, d_log_probs, dX_out, d_row_entropy)) return st;
  if (d_row_max) {  // the handle's rows are Npad apart (the kernels' layout), the caller's N
    PF_HIPCHK(hipMemcpy2DAsync(d_row_max, N * 8, h->rowM, P * 8, N * 8, B, hipMemcpyDeviceToDevice, s));
    PF_HIPCHK(hipMemcpy2DAsync(d_row_sum, N * 8, h->rowL, P * 8, N * 8, B, hipMemcpyDeviceToDevice, s));
  }
  // the statistics are complete for whoever is ordered behind this entry, as every entry is (the fence)
  h->has_stats = true;
  if (!stream) PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_soft_resample_dev"); }

pf_status pf_soft_row_stats(pf_soft_handle* h, double* row_max, double* row_sum) try {
  if (!h || !row_max || !row_sum) return fail(PF_E_ARG, "null argument");
  if (!h->has_stats) return fail(PF_E_ARG, "no pf_soft_resample has run on this handle");
  PF_HIPCHK(hipSetDevice(h->device));
  const size_t N = (size_t)h->N, P = (size_t)h->Npad, B = (size_t)h->B;
  std::vector<double> m(B * P), l(B * P);  // the device rows are Npad apart
  PF_HIPCHK(h->fence.enter(h->stream));
  const dpf::Fenced fenced{h->fence, h->stream};
  PF_HIPCHK(hipMemcpyAsync(m.data(), h->rowM, B * P * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipMemcpyAsync(l.data(), h->rowL, B * P * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  for (size_t b = 0; b < B; ++b) {
    std::copy_n(m.data() + b * P, N, row_max + b * N);
    std::copy_n(l.data() + b * P, N, row_sum + b * N);
  }
  return PF_OK;
} catch (...) { return pf::on_exception("pf_soft_row_stats"); }

pf_status pf_soft_backward(pf_soft_handle* h, const double* X, const double* log_probs, double temperature,
                           uint64_t seed, uint32_t epoch, uint32_t batch_base, const double* X_out,
                           const double* row_max, const double* row_sum, const double* grad_X_out, double* grad_X,
                           double* grad_log_probs) try {
  if (!h || !X || !log_probs || !grad_X_out || !grad_X || !grad_log_probs) return fail(PF_E_ARG, "null argument");
  const bool saved = X_out && row_max && row_sum;
  if (!saved && (X_out || row_max || row_sum))
    return fail(PF_E_ARG, "X_out, row_max and row_sum must be given together or all be null");
  if (pf_status st = dpf::check_positive("temperature", temperature)) return st;
  if (pf_status st = dpf::check_base(batch_base, h->B)) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  const size_t nX = (size_t)h->B * h->N * h->d, nR = (size_t)h->B * h->N;
  hipStream_t s = h->stream;
  if (pf_status st = ensure_bwd(h)) return st;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  PF_HIPCHK(hipMemcpyAsync(h->Xin, X, nX * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->lpin, log_probs, nR * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->gin, grad_X_out, nX * 8, hipMemcpyHostToDevice, s));
  const Prob p = make_prob(h->N, h->d, h->B, seed, epoch, batch_base);
  if (saved) {
    PF_HIPCHK(hipMemcpyAsync(h->sXo, X_out, nX * 8, hipMemcpyHostToDevice, s));
    PF_HIPCHK(hipMemcpyAsync(h->sM, row_max, nR * 8, hipMemcpyHostToDevice, s));
    PF_HIPCHK(hipMemcpyAsync(h->sL, row_sum, nR * 8, hipMemcpyHostToDevice, s));
  }
  if (pf_status st = enqueue_backward(h, s, p, 1.0 / temperature, h->Xin, h->lpin, saved ? (const double*)h->sXo : nullptr,
                                      h->sM, h->sL, h->gin, h->gX, h->glp))
    return st;
  PF_HIPCHK(hipMemcpyAsync(grad_X, h->gX, nX * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(grad_log_probs, h->glp, nR * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  if (!saved) h->has_stats = true;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_soft_backward"); }

pf_status pf_soft_backward_dev(pf_soft_handle* h, void* stream, const double* dX, const double* d_log_probs,
                               double temperature, uint64_t seed, uint32_t epoch, uint32_t batch_base,
                               const double* dX_out, const double* d_row_max, const double* d_row_sum,
                               const double* d_grad_X_out, double* d_grad_X, double* d_grad_log_probs) try {
  if (!h || !dX || !d_log_probs || !d_grad_X_out || !d_grad_X || !d_grad_log_probs)
    return fail(PF_E_ARG, "null argument");
  const bool saved = dX_out && d_row_max && d_row_sum;
  if (!saved && (dX_out || d_row_max || d_row_sum))
    return fail(PF_E_ARG, "X_out, row_max and row_sum must be given together or all be null");
  if (pf_status st = dpf::check_positive("temperature", temperature)) return st;
  if (pf_status st = dpf::check_base(batch_base, h->B)) return st;
  const size_t nX = (size_t)h->B * h->N * h->d, nR = (size_t)h->B * h->N;
  if (pf_status st = dpf::check_no_alias({{d_grad_X, nX}, {d_grad_log_probs, nR}},
                                         {{dX, nX}, {d_log_probs, nR}, {dX_out, nX}, {d_row_max, nR}, {d_row_sum, nR},
                                          {d_grad_X_out, nX}}))
    return st;
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)h->stream;
  if (pf_status st = ensure_bwd(h)) return st;  // the first call allocates, which may wait for the device
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  const Prob p = make_prob(h->N, h->d, h->B, seed, epoch, batch_base);
  if (pf_status st = enqueue_backward(h, s, p, 1.0 / temperature, dX, d_log_probs, saved ? dX_out : nullptr, d_row_max,
                                      d_row_sum, d_grad_X_out, d_grad_X, d_grad_log_probs))
    return st;
  if (!saved) h->has_stats = true;
  if (!stream) PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_soft_backward_dev"); }

pf_status pf_soft_draws(pf_soft_handle* h, uint64_t seed, uint32_t epoch, uint32_t batch_base, double* U,
                        double* G) try {
  if (!h) return fail(PF_E_ARG, "null handle");
  if (!U && !G) return fail(PF_E_ARG, "U and G are both null");
  if (pf_status st = dpf::check_base(batch_base, h->B)) return st;
  const int64_t NN = (int64_t)h->N * h->N;
  if (NN * h->B > MAXDRAWS) return fail(PF_E_ARG, "batch x N x N draws exceed 2^31: pf_soft_draws is for small problems");
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t n = (size_t)NN * h->B;
  DevBuf<double> dU, dG;  // freed on every path out; hipFree waits for the device
  if (U && dU.alloc(n) != hipSuccess) return fail(PF_E_HIP, "hipMalloc failed: draws, " + std::to_string(n * 8) + " bytes");
  if (G && dG.alloc(n) != hipSuccess) return fail(PF_E_HIP, "hipMalloc failed: draws, " + std::to_string(n * 8) + " bytes");
  const Prob p = make_prob(h->N, h->d, h->B, seed, epoch, batch_base);
  hipLaunchKernelGGL(k_soft_draws, dim3((unsigned)((NN + PB - 1) / PB), h->B), dim3(PB), 0, s, p, (double*)dU,
                     (double*)dG);
  PF_HIPCHK(hipGetLastError());
  if (U) PF_HIPCHK(hipMemcpyAsync(U, dU, n * 8, hipMemcpyDeviceToHost, s));
  if (G) PF_HIPCHK(hipMemcpyAsync(G, dG, n * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_soft_draws"); }

void* pf_soft_stream(pf_soft_handle* h) { return dpf::stream_of(h); }

pf_status pf_soft_synchronize(pf_soft_handle* h) try {
  return dpf::synchronize(h);
} catch (...) { return pf::on_exception("pf_soft_synchronize"); }

}  // extern "C"
