// Host side of the MI355X Sinkhorn optimal-transport resampler: the pf_ot_* entries of
// include/pf_engine.h.
//
// Turns one sinkhorn_ot_resample (models/DPF_OT_resampling.py:119-204) for B problems into a
// stream-ordered sequence of launches of pf_ot_kernels.h: upload, prepare, cost, then per iteration
// the two tau passes (with the merge of the split one) and the check, then the projection and download.  The stopping decision is
// made on the device; the host enqueues the iterations in chunks and reads the B done flags between
// chunks, so that a call that stops early does not pay for the empty launches of the rest.  A done
// problem's launches return at entry, so the result does not depend on the chunk length.
//
// pf_ot_backward is the reverse sweep over the same loop (pf_ot_kernels.h): the cost matrix again,
// the replay of exactly K_b iterations per problem with the dual history recorded (or the history
// the caller saved, uploaded), the projection's backward, then per iteration k = max K_b .. 1 the g
// pass, the f pass and its merge, the cost's backward and the weight chain.  A problem's launches
// for k > K_b return at entry.  The sweep's buffers, the second B N Npad matrix among them, are
// allocated by the handle's first backward or replay call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pf_engine.h"
#include "pf_dpf_host.h"
#include "pf_ot_kernels.h"

namespace pf {
namespace ot {

constexpr int POLL_DEFAULT = 16; // iterations enqueued between two reads of the done flags

// iterations per chunk: PF_OT_POLL in the environment, read at every call (1 .. 1 << 20)
static int poll_chunk() {
  const char* e = std::getenv("PF_OT_POLL");
  const long v = e ? std::atol(e) : 0;
  return v >= 1 && v <= (1 << 20) ? (int)v : POLL_DEFAULT;
}

}  // namespace ot
}  // namespace pf

using namespace pf::ot;
namespace dpf = pf::dpf;
using pf::DevBuf;
using pf::fail;

struct pf_ot_handle {
  int N = 0, Npad = 0, d = 0, B = 0, device = 0;
  // split of the source range of k_ot_tau_cols and k_ot_project, fixed by N: the split count
  // is part of the summation order
  dpf::Split split{1, 1, 0};
  pf::Stream stream;  // before the buffers: destroyed after them
  dpf::Fence fence;   // never armed: every entry of this unit runs on the handle's stream
  DevBuf<double> C, a, x, x2, f, g, fold, gold, pm, ps, part, spart, Xin, win, Xout, stats, hist;
  DevBuf<int32_t> done, iters;
  int64_t hist_cap = 0;
  // the backward pass: allocated by the first pf_ot_backward / pf_ot_replay
  DevBuf<double> Cbar, gx, xbar, fbar, gbar, abar, bpart, Gin, gX, gw, hv;
  DevBuf<int32_t> ham, pam, K;
  bool bwd_ready = false;
  int64_t hv_cap = -1;  // k_cap the history buffers were sized for
  std::vector<int32_t> flags;
  ~pf_ot_handle() { dpf::quiesce(device, stream); }
};

// the buffers of the backward pass, sized for histories of k_cap iterations
static pf_status ensure_backward(pf_ot_handle* h, int k_cap) {
  const int N = h->N, d = h->d, B = h->B;
  const size_t P = (size_t)h->Npad, BP = (size_t)B * P, BS = (size_t)B * h->split.S;
  if (!h->bwd_ready) {
    const double cbytes = (double)B * (double)N * (double)P * 8.0;
    if (h->Cbar.alloc((size_t)B * N * P) != hipSuccess)
      return fail(PF_E_HIP, "hipMalloc failed: cost-gradient matrices, " +
                                std::to_string((unsigned long long)(cbytes / 1048576.0)) + " MiB (" + std::to_string(B) +
                                " x " + std::to_string(N) + " x " + std::to_string(P) + " doubles)");
    if (pf_status st = dpf::alloc_all({{&h->gx, BP * d}, {&h->xbar, BP * d}, {&h->fbar, BP}, {&h->gbar, BP},
                                       {&h->abar, BP}, {&h->bpart, BS * P}, {&h->Gin, (size_t)B * N * d},
                                       {&h->gX, (size_t)B * N * d}, {&h->gw, (size_t)B * N}},
                                      "backward state"))
      return st;
    if (h->pam.alloc(BS * P) != hipSuccess || h->K.alloc((size_t)B) != hipSuccess)
      return fail(PF_E_HIP, "hipMalloc failed: backward flags");
    h->bwd_ready = true;
  }
  if (k_cap > h->hv_cap) {
    PF_HIPCHK(hipStreamSynchronize(h->stream));
    h->hv_cap = -1;
    const size_t nv = BP * 4 * ((size_t)k_cap + 1), na = BP * (size_t)std::max(k_cap, 1);
    if (h->hv.alloc(nv) != hipSuccess || h->ham.alloc(na) != hipSuccess)
      return fail(PF_E_HIP, "hipMalloc failed: dual history, " + std::to_string(nv * 8 + na * 4) + " bytes");
    h->hv_cap = k_cap;
  }
  return PF_OK;
}

// pf_ot_replay (hist_out) and pf_ot_backward (grad_*): see include/pf_engine.h
static pf_status sweep(pf_ot_handle* h, const double* X, const double* w, double epsilon, double min_val,
                       const int32_t* iterations, int32_t k_cap, const double* hist_in, const int32_t* am_in,
                       double* hist_out, int32_t* am_out, const double* grad_out, double* grad_X, double* grad_w) {
  if (!h || !X || !w || !iterations) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("epsilon", epsilon)) return st;
  if (k_cap < 0 || k_cap > (1 << 24)) return fail(PF_E_ARG, "k_cap out of range");
  const int N = h->N, d = h->d, B = h->B, S = h->split.S, tiles = h->split.tiles, chunk = h->split.chunk;
  int kmax = 0;
  for (int b = 0; b < B; ++b) {
    if (iterations[b] < 0 || iterations[b] > k_cap) return fail(PF_E_ARG, "iterations must be in 0 .. k_cap");
    kmax = std::max(kmax, (int)iterations[b]);
  }
  PF_HIPCHK(hipSetDevice(h->device));
  if (pf_status st = ensure_backward(h, k_cap)) return st;
  const size_t P = (size_t)h->Npad;
  hipStream_t s = h->stream;
  const size_t hrows = (size_t)B * 4 * ((size_t)k_cap + 1), arows = (size_t)B * (size_t)k_cap;

  PF_HIPCHK(hipMemcpyAsync(h->Xin, X, (size_t)B * N * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->win, w, (size_t)B * N * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->K, iterations, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (grad_out) PF_HIPCHK(hipMemcpyAsync(h->Gin, grad_out, (size_t)B * N * d * 8, hipMemcpyHostToDevice, s));
  if (hist_in) {
    PF_HIPCHK(hipMemcpy2DAsync(h->hv, P * 8, hist_in, (size_t)N * 8, (size_t)N * 8, hrows, hipMemcpyHostToDevice, s));
    if (arows > 0)
      PF_HIPCHK(hipMemcpy2DAsync(h->ham, P * 4, am_in, (size_t)N * 4, (size_t)N * 4, arows, hipMemcpyHostToDevice, s));
  } else {  // f^0 = g^0 = 0; rows past K_b stay 0 and -1
    PF_HIPCHK(hipMemsetAsync(h->hv, 0, hrows * P * 8, s));
    if (arows > 0) PF_HIPCHK(hipMemsetAsync(h->ham, 0xFF, arows * P * 4, s));
  }
  Prob p{N, h->Npad, d, B, h->a, h->x, h->x2, h->f, h->g, h->fold, h->gold, h->C, h->done, h->iters};
  const Hist hs{h->hv, h->ham, h->K, (int)k_cap};
  const Bwd bw{h->Cbar, h->gx, h->xbar, h->fbar, h->gbar, h->abar, h->bpart};
  const unsigned ng = (unsigned)((N + PB - 1) / PB), nr = (unsigned)((N + RW - 1) / RW);
  const double inv_eps = 1.0 / epsilon;
  const dpf::Poison poison(s);
  poison();
  hipLaunchKernelGGL(k_ot_prepare, dim3(ng, B), dim3(PB), 0, s, p, (const double*)h->Xin, (const double*)h->win,
                     min_val);
  poison();
  hipLaunchKernelGGL(k_ot_cost, dim3(ng, (N + CT - 1) / CT, B), dim3(PB), 0, s, p);
  PF_HIPCHK(hipGetLastError());

  if (!hist_in) {  // the replay: K_b iterations per problem, no check
    for (int k = 1; k <= kmax; ++k) {
      hipLaunchKernelGGL(k_ot_tau_rows<true>, dim3(nr, B), dim3(PB), 0, s, p, inv_eps, epsilon, min_val, hs, k);
      poison();
      hipLaunchKernelGGL(k_ot_tau_cols<true>, dim3(tiles, S, B), dim3(CB), 0, s, p, inv_eps, epsilon, min_val, chunk,
                         S, (double*)h->pm, (double*)h->ps, hs, k, (int32_t*)h->pam);
      if (S > 1)
        hipLaunchKernelGGL(k_ot_merge<true>, dim3(ng, B), dim3(PB), 0, s, p, epsilon, min_val, S,
                           (const double*)h->pm, (const double*)h->ps, hs, k, (const int32_t*)h->pam);
    }
    PF_HIPCHK(hipGetLastError());
  }
  if (hist_out) {
    PF_HIPCHK(hipMemcpy2DAsync(hist_out, (size_t)N * 8, h->hv, P * 8, (size_t)N * 8, hrows, hipMemcpyDeviceToHost, s));
    if (arows > 0)
      PF_HIPCHK(hipMemcpy2DAsync(am_out, (size_t)N * 4, h->ham, P * 4, (size_t)N * 4, arows, hipMemcpyDeviceToHost, s));
  }
  if (!grad_out) {
    PF_HIPCHK(hipStreamSynchronize(s));
    return PF_OK;
  }

  const int nch = (d + PC - 1) / PC;
  hipLaunchKernelGGL(k_ot_bwd_load, dim3(ng, B), dim3(PB), 0, s, p, bw, (const double*)h->Gin);
  poison();
  hipLaunchKernelGGL(k_ot_bwd_q, dim3(ng, (N + CT - 1) / CT, B), dim3(PB), 0, s, p, bw);
  dpf::dispatch_nc(std::min(d, PC), [&](auto nc) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ot_bwd_rowacc<decltype(nc)::value, false>), dim3(nr, nch, B), dim3(PB), 0, s,
                       p, bw, hs, inv_eps, epsilon, min_val);
  });
  hipLaunchKernelGGL(k_ot_bwd_cols<false>, dim3(tiles, S, B), dim3(CB), 0, s, p, bw, hs, 0, inv_eps, chunk, S);
  hipLaunchKernelGGL(k_ot_bwd_merge, dim3(ng, B), dim3(PB), 0, s, p, bw, hs, 0, 0, S);
  PF_HIPCHK(hipGetLastError());
  for (int k = kmax; k >= 1; --k) {
    hipLaunchKernelGGL(k_ot_bwd_rows, dim3(nr, B), dim3(PB), 0, s, p, bw, hs, k, inv_eps, epsilon);
    poison();
    hipLaunchKernelGGL(k_ot_bwd_cols<true>, dim3(tiles, S, B), dim3(CB), 0, s, p, bw, hs, k, inv_eps, chunk, S);
    hipLaunchKernelGGL(k_ot_bwd_merge, dim3(ng, B), dim3(PB), 0, s, p, bw, hs, k, 1, S);
  }
  PF_HIPCHK(hipGetLastError());
  poison();
  dpf::dispatch_nc(std::min(d, PC), [&](auto nc) {
    constexpr int NC = decltype(nc)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ot_bwd_rowacc<NC, true>), dim3(nr, nch, B), dim3(PB), 0, s, p, bw, hs, inv_eps,
                       epsilon, min_val);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ot_bwd_cost_cols<NC>), dim3(tiles, nch * S, B), dim3(CB), 0, s, p, bw, chunk,
                       S, (double*)h->part);
  });
  hipLaunchKernelGGL(k_ot_bwd_finish, dim3((unsigned)(((int64_t)N * d + PB - 1) / PB), B), dim3(PB), 0, s, p, bw, S,
                     (const double*)h->part, (double*)h->gX);
  poison();
  hipLaunchKernelGGL(k_ot_bwd_weights, dim3(ng, B), dim3(PB), 0, s, p, bw, (const double*)h->win, min_val,
                     (double*)h->gw);
  PF_HIPCHK(hipGetLastError());
  PF_HIPCHK(hipMemcpyAsync(grad_X, h->gX, (size_t)B * N * d * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(grad_w, h->gw, (size_t)B * N * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
}

extern "C" {

pf_status pf_ot_create(const pf_ot_opts* o, pf_ot_handle** out) try {
  if (!o || !out) return fail(PF_E_ARG, "null argument");
  *out = nullptr;
  if (pf_status st = dpf::check_shape(o->n_particles, true, o->dim)) return st;
  if (pf_status st = dpf::check_batch(o->batch)) return st;

  PF_HIPCHK(hipSetDevice(o->device));
  std::unique_ptr<pf_ot_handle> h(new pf_ot_handle());
  const int N = h->N = (int)o->n_particles;
  const int d = h->d = o->dim, B = h->B = o->batch;
  h->Npad = dpf::npad(N);
  h->device = o->device;
  // a 64-lane workgroup per 64 columns and a chunk of the sources (each wave's loads of C are a
  // dependent chain of HBM round trips)
  h->split = dpf::make_split(N, pf::test_hook_int("PF_TEST_OT_SPLITS"));  // tests: 1 forces the unsplit order

  if (pf_status st = dpf::make_stream(h->stream)) return st;
  const size_t P = (size_t)h->Npad, BP = (size_t)B * P, BS = (size_t)B * h->split.S;
  const double cbytes = (double)B * (double)N * (double)P * 8.0;
  if (cbytes > 9.0e18 || h->C.alloc((size_t)B * N * P) != hipSuccess)
    return fail(PF_E_HIP, "hipMalloc failed: cost matrices, " + std::to_string((unsigned long long)(cbytes / 1048576.0)) +
                              " MiB (" + std::to_string(B) + " x " + std::to_string(N) + " x " + std::to_string(P) +
                              " doubles)");
  if (pf_status st = dpf::alloc_all(
          {{&h->a, BP}, {&h->x, BP * d}, {&h->x2, BP}, {&h->f, BP}, {&h->g, BP}, {&h->fold, BP}, {&h->gold, BP},
           {&h->pm, BS * P}, {&h->ps, BS * P}, {&h->part, BS * d * P}, {&h->spart, BS * 2 * P},
           {&h->Xin, (size_t)B * N * d}, {&h->win, (size_t)B * N}, {&h->Xout, (size_t)B * N * d},
           {&h->stats, (size_t)B * 2}},
          "state"))
    return st;
  if (h->done.alloc((size_t)B) != hipSuccess || h->iters.alloc((size_t)B) != hipSuccess)
    return fail(PF_E_HIP, "hipMalloc failed: flags");
  h->flags.assign((size_t)B, 0);
  *out = h.release();
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ot_create"); }

void pf_ot_destroy(pf_ot_handle* h) { delete h; }

pf_status pf_ot_resample(pf_ot_handle* h, const double* X, const double* w, double epsilon, int32_t n_iters,
                         double min_val, double tol, double* X_out, int32_t* iterations, double* history, double* f,
                         double* g, double* plan_stats) try {
  if (!h || !X || !w || !X_out) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("epsilon", epsilon)) return st;
  if (n_iters < 0 || n_iters > (1 << 24)) return fail(PF_E_ARG, "n_iters out of range");
  PF_HIPCHK(hipSetDevice(h->device));
  const int N = h->N, d = h->d, B = h->B, S = h->split.S, tiles = h->split.tiles, chunk = h->split.chunk;
  const size_t P = (size_t)h->Npad;
  hipStream_t s = h->stream;
  const int64_t hist_n = (int64_t)B * n_iters * 2;
  if (hist_n > h->hist_cap) {  // before the launch sequence starts
    PF_HIPCHK(hipStreamSynchronize(s));
    h->hist_cap = 0;
    PF_HIPCHK(h->hist.alloc((size_t)hist_n));
    h->hist_cap = hist_n;
  }
  PF_HIPCHK(hipMemcpyAsync(h->Xin, X, (size_t)B * N * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->win, w, (size_t)B * N * 8, hipMemcpyHostToDevice, s));
  if (hist_n > 0) PF_HIPCHK(hipMemsetAsync(h->hist, 0, (size_t)hist_n * 8, s));
  Prob p{N, h->Npad, d, B, h->a, h->x, h->x2, h->f, h->g, h->fold, h->gold, h->C, h->done, h->iters};
  const unsigned ng = (unsigned)((N + PB - 1) / PB);
  const dpf::Poison poison(s);  // tests only: in front of every launch that stages through LDS
  poison();
  hipLaunchKernelGGL(k_ot_prepare, dim3(ng, B), dim3(PB), 0, s, p, (const double*)h->Xin, (const double*)h->win,
                     min_val);
  poison();
  hipLaunchKernelGGL(k_ot_cost, dim3(ng, (N + CT - 1) / CT, B), dim3(PB), 0, s, p);
  PF_HIPCHK(hipGetLastError());

  const double inv_eps = 1.0 / epsilon;
  const int poll = poll_chunk();
  for (int it = 0; it < n_iters;) {
    const int m = std::min(poll, n_iters - it);
    for (int k = 0; k < m; ++k) {
      hipLaunchKernelGGL(k_ot_tau_rows<false>, dim3((N + RW - 1) / RW, B), dim3(PB), 0, s, p, inv_eps, epsilon,
                         min_val, Hist{}, 0);
      poison();
      hipLaunchKernelGGL(k_ot_tau_cols<false>, dim3(tiles, S, B), dim3(CB), 0, s, p, inv_eps, epsilon, min_val, chunk,
                         S, (double*)h->pm, (double*)h->ps, Hist{}, 0, (int32_t*)nullptr);
      if (S > 1)
        hipLaunchKernelGGL(k_ot_merge<false>, dim3(ng, B), dim3(PB), 0, s, p, epsilon, min_val, S,
                           (const double*)h->pm, (const double*)h->ps, Hist{}, 0, (const int32_t*)nullptr);
      poison();
      hipLaunchKernelGGL(k_ot_check, dim3(B), dim3(PB), 0, s, p, tol, (int)n_iters, (double*)h->hist);
    }
    PF_HIPCHK(hipGetLastError());
    it += m;
    if (it < n_iters) {  // every problem done: the remaining launches would all return at entry
      PF_HIPCHK(hipMemcpyAsync(h->flags.data(), h->done, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      PF_HIPCHK(hipStreamSynchronize(s));
      if (std::all_of(h->flags.begin(), h->flags.end(), [](int32_t v) { return v != 0; })) break;
    }
  }

  double* spart = plan_stats ? (double*)h->spart : nullptr;
  const dim3 pg(tiles, (d + PC - 1) / PC * S, B);
  poison();
  dpf::dispatch_nc(std::min(d, PC), [&](auto nc) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ot_project<decltype(nc)::value>), pg, dim3(CB), 0, s, p, inv_eps, min_val,
                       chunk, S, (double*)h->part, spart);
  });
  hipLaunchKernelGGL(k_ot_finish, dim3((unsigned)(((int64_t)N * d + PB - 1) / PB), B), dim3(PB), 0, s, p, S,
                     (const double*)h->part, (double*)h->Xout);
  if (plan_stats) {
    poison();
    hipLaunchKernelGGL(k_ot_stats, dim3(B), dim3(PB), 0, s, p, S, (const double*)h->spart, (double*)h->stats);
  }
  PF_HIPCHK(hipGetLastError());

  PF_HIPCHK(hipMemcpyAsync(X_out, h->Xout, (size_t)B * N * d * 8, hipMemcpyDeviceToHost, s));
  if (iterations) PF_HIPCHK(hipMemcpyAsync(iterations, h->iters, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (history && hist_n > 0) PF_HIPCHK(hipMemcpyAsync(history, h->hist, (size_t)hist_n * 8, hipMemcpyDeviceToHost, s));
  if (f) PF_HIPCHK(hipMemcpy2DAsync(f, (size_t)N * 8, h->f, P * 8, (size_t)N * 8, B, hipMemcpyDeviceToHost, s));
  if (g) PF_HIPCHK(hipMemcpy2DAsync(g, (size_t)N * 8, h->g, P * 8, (size_t)N * 8, B, hipMemcpyDeviceToHost, s));
  if (plan_stats) PF_HIPCHK(hipMemcpyAsync(plan_stats, h->stats, (size_t)B * 16, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ot_resample"); }

pf_status pf_ot_replay(pf_ot_handle* h, const double* X, const double* w, double epsilon, double min_val,
                       const int32_t* iterations, int32_t k_cap, double* hist, int32_t* hist_argmax) try {
  if (!hist || (k_cap > 0 && !hist_argmax)) return fail(PF_E_ARG, "null argument");
  return sweep(h, X, w, epsilon, min_val, iterations, k_cap, nullptr, nullptr, hist, hist_argmax, nullptr, nullptr,
               nullptr);
} catch (...) { return pf::on_exception("pf_ot_replay"); }

pf_status pf_ot_backward(pf_ot_handle* h, const double* X, const double* w, double epsilon, double min_val,
                         const int32_t* iterations, int32_t k_cap, const double* hist, const int32_t* hist_argmax,
                         const double* grad_X_out, double* grad_X, double* grad_w) try {
  if (!grad_X_out || !grad_X || !grad_w) return fail(PF_E_ARG, "null argument");
  if (k_cap > 0 && (hist != nullptr) != (hist_argmax != nullptr))
    return fail(PF_E_ARG, "hist and hist_argmax come together or not at all");
  return sweep(h, X, w, epsilon, min_val, iterations, k_cap, hist, hist_argmax, nullptr, nullptr, grad_X_out, grad_X,
               grad_w);
} catch (...) { return pf::on_exception("pf_ot_backward"); }

void* pf_ot_stream(pf_ot_handle* h) { return dpf::stream_of(h); }

pf_status pf_ot_synchronize(pf_ot_handle* h) try {
  return dpf::synchronize(h);
} catch (...) { return pf::on_exception("pf_ot_synchronize"); }

}  // extern "C"
