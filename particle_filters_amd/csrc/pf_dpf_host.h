// Host-side support shared by the three resampler units of the DPF family (pf_ot / pf_soft /
// pf_rnn .hip): their common limits and argument checks, the stream a handle owns, the fence that
// orders a handle's entries across streams, the aliasing check of the device-pointer entries, the
// allocation loop, the LDS-poison test hook and the dispatch on the component-chunk width.  Host code only,
// on top of pf_host.h and pf_hooks.h; the kernels stay in each unit's own header.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "../../include/pf_engine.h"
#include "pf_hooks.h"
#include "pf_host.h"

namespace pf {
namespace dpf {

constexpr int MAXDIM = 1024;
constexpr int MAXBATCH = 65535;                // blockIdx.z
constexpr int64_t MAXN = (int64_t)1 << 24;     // of the all-pairs units (pf_ot, pf_soft)
constexpr int64_t MAXBASE = (int64_t)1 << 24;  // batch_base + B: 256 (batch_base + b) + stream in 32 bits

// The argument checks: PF_OK, or PF_E_ARG with the message set.  Used as
//   if (pf_status st = check_x(...)) return st;
inline pf_status check_shape(int64_t n_particles, bool capped, int dim) {
  if (n_particles < 1) return fail(PF_E_ARG, "n_particles must be positive");
  if (capped && n_particles > MAXN) return fail(PF_E_ARG, "n_particles too large (max 16777216)");
  if (dim < 1 || dim > MAXDIM) return fail(PF_E_ARG, "dim must be in 1 .. 1024");
  return PF_OK;
}
inline pf_status check_batch(int batch) {
  if (batch < 1 || batch > MAXBATCH) return fail(PF_E_ARG, "batch must be in 1 .. 65535");
  return PF_OK;
}
// a temperature, or OT's epsilon: positive and finite
inline pf_status check_positive(const char* name, double v) {
  if (!(v > 0.0) || !std::isfinite(v)) return fail(PF_E_ARG, std::string(name) + " must be positive");
  return PF_OK;
}
inline pf_status check_base(uint32_t batch_base, int batch) {
  if ((int64_t)batch_base + batch > MAXBASE) return fail(PF_E_ARG, "batch_base + batch must be at most 16777216");
  return PF_OK;
}

// The stream of a handle.  A handle declares it before its buffers, so that it is destroyed after
// them, and its destructor calls quiesce(): the stream is drained before any buffer is freed.
inline pf_status make_stream(Stream& s) {
  if (hipStreamCreateWithFlags(s.out(), hipStreamNonBlocking) != hipSuccess)
    return fail(PF_E_HIP, "hipStreamCreate failed");
  return PF_OK;
}
// The fence of a handle whose scratch is touched from more than one stream (the *_dev entries run on
// the caller's stream, the host entries on the handle's): one event, recorded when an entry has
// enqueued its last work; the next entry, on whichever stream, waits on it before its first.  An
// entry reads
//   PF_HIPCHK(h->fence.enter(s));
//   const dpf::Fenced fenced{h->fence, s};  // records on every path out
// quiesce() and synchronize() wait for it too, so a handle may be destroyed, or its host entries
// called, straight after an entry that did not synchronise.
class Fence {
 public:
  hipError_t enter(hipStream_t s) {
    if (!ev_) {
      const hipError_t e = hipEventCreateWithFlags(ev_.out(), hipEventDisableTiming);
      if (e != hipSuccess) return e;
    }
    return armed_ ? hipStreamWaitEvent(s, ev_, 0) : hipSuccess;
  }
  void leave(hipStream_t s) {
    if (ev_ && hipEventRecord(ev_, s) == hipSuccess) armed_ = true;
  }
  hipError_t wait() const { return armed_ ? hipEventSynchronize(ev_) : hipSuccess; }

 private:
  Event ev_;
  bool armed_ = false;
};
struct Fenced {
  Fence& fence;
  hipStream_t s;
  ~Fenced() { fence.leave(s); }
};

inline void quiesce(int device, hipStream_t s) {
  (void)hipSetDevice(device);
  if (s) (void)hipStreamSynchronize(s);
}
inline void quiesce(int device, hipStream_t s, const Fence& fence) {
  (void)hipSetDevice(device);
  (void)fence.wait();
  if (s) (void)hipStreamSynchronize(s);
}
// the bodies of pf_x_stream and pf_x_synchronize; H has the members device, stream and fence
template <class H>
void* stream_of(const H* h) {
  return h ? (void*)h->stream : nullptr;
}
template <class H>
pf_status synchronize(const H* h) {
  if (!h) return fail(PF_E_ARG, "null handle");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(h->fence.wait());
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
}

// PF_E_ARG if the output [out, out + n_out) overlaps the input [in, in + n_in) (doubles; a null
// pointer overlaps nothing): the *_dev entries read their inputs where they lie
inline bool overlaps(const double* out, size_t n_out, const double* in, size_t n_in) {
  if (!out || !in) return false;
  const uintptr_t a = (uintptr_t)out, b = (uintptr_t)in;
  return a < b + n_in * 8 && b < a + n_out * 8;
}
struct Span {
  const double* p;
  size_t n;
};
inline pf_status check_no_alias(std::initializer_list<Span> outs, std::initializer_list<Span> ins) {
  for (const Span& o : outs)
    for (const Span& i : ins)
      if (overlaps(o.p, o.n, i.p, i.n)) return fail(PF_E_ARG, "an output aliases an input of the same call");
  return PF_OK;
}

// every buffer of the list, or the failure "hipMalloc failed: <what>, <bytes> bytes" of the first
// that could not be had
struct Alloc {
  DevBuf<double>* buf;
  size_t n;
};
inline pf_status alloc_all(std::initializer_list<Alloc> list, const char* what) {
  for (const Alloc& a : list)
    if (a.buf->alloc(a.n) != hipSuccess)
      return fail(PF_E_HIP, std::string("hipMalloc failed: ") + what + ", " + std::to_string(a.n * 8) + " bytes");
  return PF_OK;
}

// Tests only (pf_hooks.h): PF_TEST_LDS_POISON is read once, when an entry makes its Poison, and
// when it is on every launch of a kernel that stages through LDS is preceded by the poison: the
// entry calls poison() in front of each such launch (tests/test_gpu_lds_poison.py,
// tests/test_gpu_dpf_*_poison.py).
class Poison {
 public:
  explicit Poison(hipStream_t s) : s_(s), on_(test_hook("PF_TEST_LDS_POISON")) {}
  void operator()() const {
    if (on_) {
      lds_poison(s_);
      lds_poison_count_add();
    }
  }

 private:
  hipStream_t s_;
  bool on_;
};

// f(std::integral_constant<int, NC>) with the narrowest instantiated NC >= nc: the kernels that
// keep NC state components per lane in registers (nc = min(d, PC) <= 16)
template <class F>
void dispatch_nc(int nc, F&& f) {
  if (nc <= 1) f(std::integral_constant<int, 1>{});
  else if (nc <= 2) f(std::integral_constant<int, 2>{});
  else if (nc <= 4) f(std::integral_constant<int, 4>{});
  else if (nc <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

}  // namespace dpf
}  // namespace pf
