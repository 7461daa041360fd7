// Host-side support shared by the nine units behind the C ABI (pf_engine / pf_ledh / pf_diag /
// pf_kpf / pf_spf / pf_edh_dense .hip and, through pf_dpf_host.h, pf_ot / pf_soft / pf_rnn .hip):
// the error helpers, the exception boundary of the extern "C" entries, the owners of
// device memory, streams and events, and the small dense linear algebra of the create functions.
// Host code only; nothing here is visible to a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/pf_engine.h"

namespace pf {

// the thread-local message behind pf_last_error (defined in pf_engine.hip)
void set_last_error(const std::string& msg);

inline pf_status fail(pf_status code, const std::string& msg) {
  set_last_error(msg);
  return code;
}

#define PF_HIPCHK(expr)                                                                                   \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) return ::pf::fail(PF_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// No exception crosses the C ABI.  Every extern "C" entry that can allocate on the host (a handle,
// a std::vector, an error string) is a function-try-block whose handler returns this:
//   pf_status pf_x(...) try { ... } catch (...) { return pf::on_exception("pf_x"); }
inline pf_status on_exception(const char* entry) noexcept {
  try {
    set_last_error(std::string("out of host memory (or another C++ exception) in ") + entry);
  } catch (...) {
  }
  return PF_E_HIP;
}

// Owning device pointer: the one place that calls hipMalloc / hipFree.  Converts to T*, so kernel
// argument lists, parameter-struct initialisers, pointer arithmetic and std::swap read as with a
// raw pointer.  hipFree waits for the device, so a buffer may go out of scope on an error path
// while work that uses it is still queued.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  // count elements of T (bytes for DevBuf<void>); frees what it held first, null on failure
  hipError_t alloc(size_t count) {
    reset();
    const hipError_t e = hipMalloc((void**)&p_, count * sizeof(std::conditional_t<std::is_void_v<T>, char, T>));
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  void reset() {
    if (p_) (void)hipFree((void*)p_);
    p_ = nullptr;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
};

// Owning hipStream_t / hipEvent_t: hipStreamCreateWithFlags(s.out(), flags), hipEventCreate(e.out()).
template <class H, hipError_t (*Destroy)(H)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  ~Owned() { reset(); }
  H* out() {
    reset();
    return &h_;
  }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }
  operator H() const { return h_; }

 private:
  H h_ = nullptr;
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// Lower Cholesky factor of an n x n row-major SPD matrix (+ jitter * I); false if not PD.
inline bool chol_lower(const double* A, int n, double jitter, std::vector<double>& L) {
  L.assign((size_t)n * n, 0.0);
  for (int j = 0; j < n; ++j) {
    double d = A[j * n + j] + jitter;
    for (int k = 0; k < j; ++k) d -= L[j * n + k] * L[j * n + k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    const double ljj = std::sqrt(d);
    L[j * n + j] = ljj;
    for (int i = j + 1; i < n; ++i) {
      double s = A[i * n + j];
      for (int k = 0; k < j; ++k) s -= L[i * n + k] * L[j * n + k];
      L[i * n + j] = s / ljj;
    }
  }
  return true;
}

// W = L^-1 of a lower-triangular n x n row-major L (forward substitution, column by column)
inline void lower_inverse(const double* L, int n, std::vector<double>& W) {
  W.assign((size_t)n * n, 0.0);
  for (int c = 0; c < n; ++c)
    for (int r = c; r < n; ++r) {
      double s = (r == c) ? 1.0 : 0.0;
      for (int k = c; k < r; ++k) s -= L[(size_t)r * n + k] * W[(size_t)k * n + c];
      W[(size_t)r * n + c] = s / L[(size_t)r * n + r];
    }
}

// inverse of an SPD matrix via its Cholesky factor
inline bool spd_inverse(const double* A, int n, std::vector<double>& Ainv) {
  std::vector<double> L;
  if (!chol_lower(A, n, 0.0, L)) return false;
  Ainv.assign((size_t)n * n, 0.0);
  std::vector<double> col(n), y(n);
  for (int c = 0; c < n; ++c) {
    for (int i = 0; i < n; ++i) {
      double s = (i == c) ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k) s -= L[i * n + k] * y[k];
      y[i] = s / L[i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
      double s = y[i];
      for (int k = i + 1; k < n; ++k) s -= L[k * n + i] * col[k];
      col[i] = s / L[i * n + i];
    }
    for (int i = 0; i < n; ++i) Ainv[i * n + c] = col[i];
  }
  return true;
}

inline bool is_diag(const double* A, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      if (i != j && A[i * n + j] != 0.0) return false;
  return true;
}

}  // namespace pf
