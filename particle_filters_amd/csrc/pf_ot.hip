// Host side of the MI355X Sinkhorn optimal-transport resampler: the pf_ot_* entries of
// include/pf_engine.h.
//
// Turns one sinkhorn_ot_resample (models/DPF_OT_resampling.py:119-204) for B problems into a
// stream-ordered sequence of launches of pf_ot_kernels.h: prepare, cost, then per iteration the two
// tau passes (with the merge of the split one) and the check, then the projection.  The stopping
// decision is made on the device.  A done problem's launches return at entry, so the result does not
// depend on how many iterations are enqueued behind the stop: the host entry, and a device entry on
// the handle's own stream, enqueue them in chunks and read the B done flags between chunks, so that a
// call that stops early does not pay for the empty launches of the rest; a device entry on a
// caller's stream enqueues all of them and reads nothing back.  On request the forward pass records
// its own dual history (the third mode of the tau kernels), which is bitwise the replay's.  With
// PF_OT_RESIDENT a device entry runs all of this as one launch instead, one workgroup per problem with
// the cost matrix in LDS (pf_ot_resident.h; N <= 128, PF_E_ARG above, never chosen by itself).
//
// pf_ot_backward is the reverse sweep over the same loop (pf_ot_kernels.h): the cost matrix again,
// the replay of exactly K_b iterations per problem with the dual history recorded (or the history
// the caller saved), the projection's backward, then per iteration k = k_sweep .. 1 the g pass, the
// f pass and its merge, the cost's backward and the weight chain.  A problem's launches for k > K_b
// return at entry.  The sweep's buffers, the second B N Npad matrix among them, are allocated by the
// handle's first backward or replay call.
//
// The launches of each pass are one enqueue_* function on device pointers and a stream: the host
// entries call it on the handle's staging buffers and stream, between their copies, the *_dev
// entries on the caller's pointers and stream, with no copies of the inputs.  The entries of a
// handle are ordered across streams by its fence (pf_dpf_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pf_engine.h"
#include "pf_dpf_host.h"
#include "pf_ot_kernels.h"
#include "pf_ot_resident.h"

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

constexpr int MAXITERS = 1 << 24;  // n_iters and k_cap

struct pf_ot_handle {
  int N = 0, Npad = 0, d = 0, B = 0, device = 0;
  // split of the source range of k_ot_tau_cols and k_ot_project, fixed by N: the split count
  // is part of the summation order
  dpf::Split split{1, 1, 0};
  pf::Stream stream;  // before the buffers: destroyed after them
  dpf::Fence fence;   // orders the entries, which may run on different streams
  DevBuf<double> C, a, x, x2, f, g, fold, gold, pm, ps, part, spart, Xin, win, Xout, stats, hist;
  DevBuf<int32_t> done, iters;
  int64_t hist_cap = 0;
  DevBuf<int32_t> pam;  // the argmax partials of a recording tau pass: the first call that records
  // the backward pass: allocated by the first pf_ot_backward / pf_ot_replay
  DevBuf<double> Cbar, gx, xbar, fbar, gbar, abar, bpart, Gin, gX, gw, hv;
  DevBuf<int32_t> ham, K, Kin;
  bool bwd_ready = false;
  int64_t hv_cap = -1;  // k_cap the history buffers were sized for
  std::vector<int32_t> flags;
  bool resident_ready = false;  // k_ot_resident may use this handle's dynamic LDS (resident_plan(N).total)
  ~pf_ot_handle() { dpf::quiesce(device, stream, fence); }
};

// waits for the handle's latest entry, on whichever stream it ran: before a buffer is replaced
static pf_status drain(pf_ot_handle* h) {
  PF_HIPCHK(h->fence.wait());
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
}

static Prob prob_of(pf_ot_handle* h) {
  return Prob{h->N, h->Npad, h->d, h->B, h->a, h->x, h->x2, h->f, h->g, h->fold, h->gold, h->C, h->done, h->iters};
}

static pf_status ensure_pam(pf_ot_handle* h) {
  if (!h->pam && h->pam.alloc((size_t)h->B * h->split.S * (size_t)h->Npad) != hipSuccess)
    return fail(PF_E_HIP, "hipMalloc failed: argmax partials");
  return PF_OK;
}

// the change history [B][n_iters][2] of the handle, grown before a launch sequence starts
static pf_status ensure_changes(pf_ot_handle* h, int64_t hist_n) {
  if (hist_n <= h->hist_cap) return PF_OK;
  if (pf_status st = drain(h)) return st;
  h->hist_cap = 0;
  PF_HIPCHK(h->hist.alloc((size_t)hist_n));
  h->hist_cap = hist_n;
  return PF_OK;
}

// One resampling on stream s, every pointer device memory: X [B][N][d], w [B][N] -> X_out [B][N][d],
// changes [B][n_iters][2], on request stats [B][2] and the dual history rec (rows rec.ld apart, kcap =
// n_iters, cleared here); the iteration counts and f, g [B][Npad] stay in the handle.  poll: read the
// done flags between chunks of iterations (s is then synchronised here).  resident: all of it in one
// launch of k_ot_resident (pf_ot_resident.h), for a handle that ensure_resident has accepted.
static pf_status enqueue_resample(pf_ot_handle* h, hipStream_t s, bool poll, bool resident, const double* X,
                                  const double* w, double epsilon, int n_iters, double min_val, double tol,
                                  double* X_out, double* changes, double* stats, const Hist* rec) {
  const int N = h->N, d = h->d, B = h->B, S = h->split.S, tiles = h->split.tiles, chunk = h->split.chunk;
  const int64_t hist_n = (int64_t)B * n_iters * 2;
  if (hist_n > 0) PF_HIPCHK(hipMemsetAsync(changes, 0, (size_t)hist_n * 8, s));
  if (rec) {  // f^0 = g^0 = 0; rows past a problem's stop stay 0 and -1
    const size_t hrows = (size_t)B * 4 * ((size_t)n_iters + 1), arows = (size_t)B * (size_t)n_iters;
    PF_HIPCHK(hipMemsetAsync(rec->v, 0, hrows * (size_t)rec->ld * 8, s));
    if (arows > 0) PF_HIPCHK(hipMemsetAsync(rec->am, 0xFF, arows * (size_t)rec->ld * 4, s));
  }
  Prob p = prob_of(h);
  const unsigned ng = (unsigned)((N + PB - 1) / PB), nr = (unsigned)((N + RW - 1) / RW);
  const dpf::Poison poison(s);  // tests only: in front of every launch that stages through LDS
  if (resident) {
    const Resident q{X, w, X_out, h->f, h->g, h->iters, changes, stats, rec ? *rec : Hist{}, N, d, n_iters,
                     epsilon, 1.0 / epsilon, min_val, tol};
    poison();
    hipLaunchKernelGGL(k_ot_resident, dim3(B), dim3(RES_THREADS), resident_plan(N).total, s, q);
    PF_HIPCHK(hipGetLastError());
    return PF_OK;
  }
  poison();
  hipLaunchKernelGGL(k_ot_prepare, dim3(ng, B), dim3(PB), 0, s, p, X, w, min_val);
  poison();
  hipLaunchKernelGGL(k_ot_cost, dim3(ng, (N + CT - 1) / CT, B), dim3(PB), 0, s, p);
  PF_HIPCHK(hipGetLastError());

  const double inv_eps = 1.0 / epsilon;
  const int step = poll ? poll_chunk() : std::max(n_iters, 1);
  for (int it = 0; it < n_iters;) {
    const int m = std::min(step, n_iters - it);
    for (int k = 0; k < m; ++k) {
      if (rec) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ot_tau_rows<true, true>), dim3(nr, B), dim3(PB), 0, s, p, inv_eps,
                           epsilon, min_val, *rec, 0);
        poison();
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ot_tau_cols<true, true>), dim3(tiles, S, B), dim3(CB), 0, s, p, inv_eps,
                           epsilon, min_val, chunk, S, (double*)h->pm, (double*)h->ps, *rec, 0, (int32_t*)h->pam);
        if (S > 1)
          hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ot_merge<true, true>), dim3(ng, B), dim3(PB), 0, s, p, epsilon, min_val,
                             S, (const double*)h->pm, (const double*)h->ps, *rec, 0, (const int32_t*)h->pam);
      } else {
        hipLaunchKernelGGL(k_ot_tau_rows<false>, dim3(nr, B), dim3(PB), 0, s, p, inv_eps, epsilon, min_val, Hist{}, 0);
        poison();
        hipLaunchKernelGGL(k_ot_tau_cols<false>, dim3(tiles, S, B), dim3(CB), 0, s, p, inv_eps, epsilon, min_val,
                           chunk, S, (double*)h->pm, (double*)h->ps, Hist{}, 0, (int32_t*)nullptr);
        if (S > 1)
          hipLaunchKernelGGL(k_ot_merge<false>, dim3(ng, B), dim3(PB), 0, s, p, epsilon, min_val, S,
                             (const double*)h->pm, (const double*)h->ps, Hist{}, 0, (const int32_t*)nullptr);
      }
      poison();
      hipLaunchKernelGGL(k_ot_check, dim3(B), dim3(PB), 0, s, p, tol, (int)n_iters, changes);
    }
    PF_HIPCHK(hipGetLastError());
    it += m;
    if (it < n_iters) {  // every problem done: the remaining launches would all return at entry
      PF_HIPCHK(hipMemcpyAsync(h->flags.data(), h->done, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      PF_HIPCHK(hipStreamSynchronize(s));
      if (std::all_of(h->flags.begin(), h->flags.end(), [](int32_t v) { return v != 0; })) break;
    }
  }

  double* spart = stats ? (double*)h->spart : nullptr;
  const dim3 pg(tiles, (d + PC - 1) / PC * S, B);
  poison();
  dpf::dispatch_nc(std::min(d, PC), [&](auto nc) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ot_project<decltype(nc)::value>), pg, dim3(CB), 0, s, p, inv_eps, min_val,
                       chunk, S, (double*)h->part, spart);
  });
  hipLaunchKernelGGL(k_ot_finish, dim3((unsigned)(((int64_t)N * d + PB - 1) / PB), B), dim3(PB), 0, s, p, S,
                     (const double*)h->part, X_out);
  if (stats) {
    poison();
    hipLaunchKernelGGL(k_ot_stats, dim3(B), dim3(PB), 0, s, p, S, (const double*)h->spart, stats);
  }
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

// PF_OT_RESIDENT on this handle: PF_E_ARG when its N does not fit the plan; the kernel's dynamic LDS
// limit raised once, with the status checked (a discarded failure would surface as a failed launch)
static pf_status ensure_resident(pf_ot_handle* h) {
  const ResidentPlan pl = resident_plan(h->N);
  if (!pl.fits) return fail(PF_E_ARG, "PF_OT_RESIDENT needs n_particles <= " + std::to_string(RES_MAXN));
  if (!h->resident_ready) {
    PF_HIPCHK(hipFuncSetAttribute((const void*)k_ot_resident, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)RES_LDS_MAX));
    h->resident_ready = true;
  }
  return PF_OK;
}

// the buffers of the backward pass; own_hist: the handle's history, sized for k_cap iterations
static pf_status ensure_backward(pf_ot_handle* h, int k_cap, bool own_hist) {
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
    if (pf_status st = ensure_pam(h)) return st;
    if (h->K.alloc((size_t)B) != hipSuccess || h->Kin.alloc((size_t)B) != hipSuccess)
      return fail(PF_E_HIP, "hipMalloc failed: backward flags");
    h->bwd_ready = true;
  }
  if (own_hist && k_cap > h->hv_cap) {
    if (pf_status st = drain(h)) return st;
    h->hv_cap = -1;
    const size_t nv = BP * 4 * ((size_t)k_cap + 1), na = BP * (size_t)std::max(k_cap, 1);
    if (h->hv.alloc(nv) != hipSuccess || h->ham.alloc(na) != hipSuccess)
      return fail(PF_E_HIP, "hipMalloc failed: dual history, " + std::to_string(nv * 8 + na * 4) + " bytes");
    h->hv_cap = k_cap;
  }
  return PF_OK;
}

// The replay and the reverse sweep on stream s, every pointer device memory.  its [B] are the
// caller's counts; the kernels read them clamped to 0 .. k_sweep (hs.K, the handle's).  replay: the
// history hs is cleared and k_sweep iterations are enqueued, gated by K_b, recording into it;
// otherwise hs holds the history already.  gin null: the replay only.
static pf_status enqueue_sweep(pf_ot_handle* h, hipStream_t s, const double* X, const double* w, double epsilon,
                               double min_val, const int32_t* its, int k_sweep, const Hist& hs, bool replay,
                               const double* gin, double* gX, double* gw) {
  const int N = h->N, d = h->d, B = h->B, S = h->split.S, tiles = h->split.tiles, chunk = h->split.chunk;
  const size_t hrows = (size_t)B * 4 * ((size_t)hs.kcap + 1), arows = (size_t)B * (size_t)hs.kcap;
  hipLaunchKernelGGL(k_ot_bwd_counts, dim3((unsigned)((B + PB - 1) / PB)), dim3(PB), 0, s, its, (int32_t*)h->K, B,
                     k_sweep);
  if (replay) {  // f^0 = g^0 = 0; rows past K_b stay 0 and -1
    PF_HIPCHK(hipMemsetAsync(hs.v, 0, hrows * (size_t)hs.ld * 8, s));
    if (arows > 0) PF_HIPCHK(hipMemsetAsync(hs.am, 0xFF, arows * (size_t)hs.ld * 4, s));
  }
  Prob p = prob_of(h);
  const Bwd bw{h->Cbar, h->gx, h->xbar, h->fbar, h->gbar, h->abar, h->bpart};
  const unsigned ng = (unsigned)((N + PB - 1) / PB), nr = (unsigned)((N + RW - 1) / RW);
  const double inv_eps = 1.0 / epsilon;
  const dpf::Poison poison(s);
  poison();
  hipLaunchKernelGGL(k_ot_prepare, dim3(ng, B), dim3(PB), 0, s, p, X, w, min_val);
  poison();
  hipLaunchKernelGGL(k_ot_cost, dim3(ng, (N + CT - 1) / CT, B), dim3(PB), 0, s, p);
  PF_HIPCHK(hipGetLastError());

  if (replay) {  // K_b iterations per problem, no check
    for (int k = 1; k <= k_sweep; ++k) {
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
  if (!gin) return PF_OK;

  const int nch = (d + PC - 1) / PC;
  hipLaunchKernelGGL(k_ot_bwd_load, dim3(ng, B), dim3(PB), 0, s, p, bw, gin);
  poison();
  hipLaunchKernelGGL(k_ot_bwd_q, dim3(ng, (N + CT - 1) / CT, B), dim3(PB), 0, s, p, bw);
  dpf::dispatch_nc(std::min(d, PC), [&](auto nc) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ot_bwd_rowacc<decltype(nc)::value, false>), dim3(nr, nch, B), dim3(PB), 0, s,
                       p, bw, hs, inv_eps, epsilon, min_val);
  });
  hipLaunchKernelGGL(k_ot_bwd_cols<false>, dim3(tiles, S, B), dim3(CB), 0, s, p, bw, hs, 0, inv_eps, chunk, S);
  hipLaunchKernelGGL(k_ot_bwd_merge, dim3(ng, B), dim3(PB), 0, s, p, bw, hs, 0, 0, S);
  PF_HIPCHK(hipGetLastError());
  for (int k = k_sweep; k >= 1; --k) {
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
                     (const double*)h->part, gX);
  poison();
  hipLaunchKernelGGL(k_ot_bwd_weights, dim3(ng, B), dim3(PB), 0, s, p, bw, w, min_val, gw);
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

// pf_ot_replay (hist_out) and pf_ot_backward (grad_*): see include/pf_engine.h
static pf_status sweep(pf_ot_handle* h, const double* X, const double* w, double epsilon, double min_val,
                       const int32_t* iterations, int32_t k_cap, const double* hist_in, const int32_t* am_in,
                       double* hist_out, int32_t* am_out, const double* grad_out, double* grad_X, double* grad_w) {
  if (!h || !X || !w || !iterations) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("epsilon", epsilon)) return st;
  if (k_cap < 0 || k_cap > MAXITERS) return fail(PF_E_ARG, "k_cap out of range");
  const int N = h->N, d = h->d, B = h->B;
  int kmax = 0;
  for (int b = 0; b < B; ++b) {
    if (iterations[b] < 0 || iterations[b] > k_cap) return fail(PF_E_ARG, "iterations must be in 0 .. k_cap");
    kmax = std::max(kmax, (int)iterations[b]);
  }
  PF_HIPCHK(hipSetDevice(h->device));
  if (pf_status st = ensure_backward(h, k_cap, true)) return st;
  const size_t P = (size_t)h->Npad;
  hipStream_t s = h->stream;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  const size_t hrows = (size_t)B * 4 * ((size_t)k_cap + 1), arows = (size_t)B * (size_t)k_cap;

  PF_HIPCHK(hipMemcpyAsync(h->Xin, X, (size_t)B * N * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->win, w, (size_t)B * N * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->Kin, iterations, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (grad_out) PF_HIPCHK(hipMemcpyAsync(h->Gin, grad_out, (size_t)B * N * d * 8, hipMemcpyHostToDevice, s));
  if (hist_in) {  // the handle's rows are Npad apart, the caller's N
    PF_HIPCHK(hipMemcpy2DAsync(h->hv, P * 8, hist_in, (size_t)N * 8, (size_t)N * 8, hrows, hipMemcpyHostToDevice, s));
    if (arows > 0)
      PF_HIPCHK(hipMemcpy2DAsync(h->ham, P * 4, am_in, (size_t)N * 4, (size_t)N * 4, arows, hipMemcpyHostToDevice, s));
  }
  const Hist hs{h->hv, h->ham, h->K, (int)k_cap, h->Npad};
  if (pf_status st = enqueue_sweep(h, s, h->Xin, h->win, epsilon, min_val, h->Kin, kmax, hs, !hist_in,
                                   grad_out ? (const double*)h->Gin : nullptr, h->gX, h->gw))
    return st;
  if (hist_out) {
    PF_HIPCHK(hipMemcpy2DAsync(hist_out, (size_t)N * 8, h->hv, P * 8, (size_t)N * 8, hrows, hipMemcpyDeviceToHost, s));
    if (arows > 0)
      PF_HIPCHK(hipMemcpy2DAsync(am_out, (size_t)N * 4, h->ham, P * 4, (size_t)N * 4, arows, hipMemcpyDeviceToHost, s));
  }
  if (grad_out) {
    PF_HIPCHK(hipMemcpyAsync(grad_X, h->gX, (size_t)B * N * d * 8, hipMemcpyDeviceToHost, s));
    PF_HIPCHK(hipMemcpyAsync(grad_w, h->gw, (size_t)B * N * 8, hipMemcpyDeviceToHost, s));
  }
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
}

// an int32 array as a span of the aliasing check (whole doubles, rounded up)
static dpf::Span span32(const int32_t* p, size_t n) { return dpf::Span{(const double*)p, (n + 1) / 2}; }

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
  if (n_iters < 0 || n_iters > MAXITERS) return fail(PF_E_ARG, "n_iters out of range");
  PF_HIPCHK(hipSetDevice(h->device));
  const int N = h->N, d = h->d, B = h->B;
  const size_t P = (size_t)h->Npad;
  hipStream_t s = h->stream;
  const int64_t hist_n = (int64_t)B * n_iters * 2;
  if (pf_status st = ensure_changes(h, hist_n)) return st;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  PF_HIPCHK(hipMemcpyAsync(h->Xin, X, (size_t)B * N * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->win, w, (size_t)B * N * 8, hipMemcpyHostToDevice, s));
  if (pf_status st = enqueue_resample(h, s, true, false, h->Xin, h->win, epsilon, n_iters, min_val, tol, h->Xout, h->hist,
                                      plan_stats ? (double*)h->stats : nullptr, nullptr))
    return st;

  PF_HIPCHK(hipMemcpyAsync(X_out, h->Xout, (size_t)B * N * d * 8, hipMemcpyDeviceToHost, s));
  if (iterations) PF_HIPCHK(hipMemcpyAsync(iterations, h->iters, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (history && hist_n > 0) PF_HIPCHK(hipMemcpyAsync(history, h->hist, (size_t)hist_n * 8, hipMemcpyDeviceToHost, s));
  if (f) PF_HIPCHK(hipMemcpy2DAsync(f, (size_t)N * 8, h->f, P * 8, (size_t)N * 8, B, hipMemcpyDeviceToHost, s));
  if (g) PF_HIPCHK(hipMemcpy2DAsync(g, (size_t)N * 8, h->g, P * 8, (size_t)N * 8, B, hipMemcpyDeviceToHost, s));
  if (plan_stats) PF_HIPCHK(hipMemcpyAsync(plan_stats, h->stats, (size_t)B * 16, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ot_resample"); }

pf_status pf_ot_resample_dev(pf_ot_handle* h, void* stream, const double* dX, const double* dw, double epsilon,
                             int32_t n_iters, double min_val, double tol, int32_t flags, double* dX_out,
                             int32_t* d_iterations, double* d_history, double* d_f, double* d_g, double* d_plan_stats,
                             double* d_hist, int32_t* d_hist_argmax) try {
  if (!h || !dX || !dw || !dX_out) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("epsilon", epsilon)) return st;
  if (n_iters < 0 || n_iters > MAXITERS) return fail(PF_E_ARG, "n_iters out of range");
  if (flags & ~PF_OT_RESIDENT) return fail(PF_E_ARG, "flags must be 0 or PF_OT_RESIDENT");
  const bool resident = (flags & PF_OT_RESIDENT) != 0;
  if (n_iters > 0 ? (d_hist != nullptr) != (d_hist_argmax != nullptr) : (d_hist_argmax && !d_hist))
    return fail(PF_E_ARG, "hist and hist_argmax come together or not at all");
  const size_t N = (size_t)h->N, B = (size_t)h->B, P = (size_t)h->Npad, nX = B * N * h->d, nR = B * N;
  const size_t nH = nR * 4 * ((size_t)n_iters + 1), nA = nR * (size_t)n_iters;
  const int64_t hist_n = (int64_t)B * n_iters * 2;
  if (pf_status st = dpf::check_no_alias({{dX_out, nX}, span32(d_iterations, B), {d_history, (size_t)hist_n}, {d_f, nR},
                                          {d_g, nR}, {d_plan_stats, B * 2}, {d_hist, nH}, span32(d_hist_argmax, nA)},
                                         {{dX, nX}, {dw, nR}}))
    return st;
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)h->stream;
  if (!d_history)  // the changes go to the handle's buffer, which may have to grow (and then waits)
    if (pf_status st = ensure_changes(h, hist_n)) return st;
  if (resident) {
    if (pf_status st = ensure_resident(h)) return st;
  } else if (d_hist) {
    if (pf_status st = ensure_pam(h)) return st;
  }
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  const Hist rec{d_hist, d_hist_argmax, nullptr, (int)n_iters, h->N};
  if (pf_status st = enqueue_resample(h, s, !stream, resident, dX, dw, epsilon, n_iters, min_val, tol, dX_out,
                                      d_history ? d_history : (double*)h->hist, d_plan_stats, d_hist ? &rec : nullptr))
    return st;
  if (d_iterations)
    PF_HIPCHK(hipMemcpyAsync(d_iterations, h->iters, B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  // the handle's rows are Npad apart (the kernels' layout), the caller's N
  if (d_f) PF_HIPCHK(hipMemcpy2DAsync(d_f, N * 8, h->f, P * 8, N * 8, B, hipMemcpyDeviceToDevice, s));
  if (d_g) PF_HIPCHK(hipMemcpy2DAsync(d_g, N * 8, h->g, P * 8, N * 8, B, hipMemcpyDeviceToDevice, s));
  if (!stream) PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ot_resample_dev"); }

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

pf_status pf_ot_backward_dev(pf_ot_handle* h, void* stream, const double* dX, const double* dw, double epsilon,
                             double min_val, const int32_t* d_iterations, int32_t k_cap, int32_t k_sweep,
                             const double* d_hist, const int32_t* d_hist_argmax, const double* d_grad_X_out,
                             double* d_grad_X, double* d_grad_w) try {
  if (!d_grad_X_out || !d_grad_X || !d_grad_w) return fail(PF_E_ARG, "null argument");
  if (k_cap > 0 && (d_hist != nullptr) != (d_hist_argmax != nullptr))
    return fail(PF_E_ARG, "hist and hist_argmax come together or not at all");
  if (!h || !dX || !dw || !d_iterations) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("epsilon", epsilon)) return st;
  if (k_cap < 0 || k_cap > MAXITERS) return fail(PF_E_ARG, "k_cap out of range");
  if (k_sweep > k_cap || k_sweep < (k_cap > 0 ? 1 : 0))
    return fail(PF_E_ARG, "k_sweep must be in 1 .. k_cap (0 when k_cap is 0)");
  const size_t N = (size_t)h->N, B = (size_t)h->B, nX = B * N * h->d, nR = B * N;
  if (pf_status st = dpf::check_no_alias(
          {{d_grad_X, nX}, {d_grad_w, nR}},
          {{dX, nX}, {dw, nR}, span32(d_iterations, B), {d_hist, nR * 4 * ((size_t)k_cap + 1)},
           span32(d_hist_argmax, nR * (size_t)k_cap), {d_grad_X_out, nX}}))
    return st;
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)h->stream;
  // the first call allocates, which may wait for the device
  if (pf_status st = ensure_backward(h, k_cap, !d_hist)) return st;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  const Hist hs = d_hist ? Hist{const_cast<double*>(d_hist), const_cast<int32_t*>(d_hist_argmax), h->K, (int)k_cap, h->N}
                         : Hist{h->hv, h->ham, h->K, (int)k_cap, h->Npad};
  if (pf_status st = enqueue_sweep(h, s, dX, dw, epsilon, min_val, d_iterations, k_sweep, hs, !d_hist, d_grad_X_out,
                                   d_grad_X, d_grad_w))
    return st;
  if (!stream) PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ot_backward_dev"); }

int32_t pf_ot_resident_supported(pf_ot_handle* h) { return h && resident_plan(h->N).fits ? 1 : 0; }

void* pf_ot_stream(pf_ot_handle* h) { return dpf::stream_of(h); }

pf_status pf_ot_synchronize(pf_ot_handle* h) try {
  return dpf::synchronize(h);
} catch (...) { return pf::on_exception("pf_ot_synchronize"); }

}  // extern "C"
