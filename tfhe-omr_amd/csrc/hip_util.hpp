// Host-side HIP helpers shared by the translation units of libomr_gpu: the error-return macro, the
// environment switch test and the one owner type of device memory.
#pragma once

#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "common.hpp"

// Returns from the enclosing function with the library's status for a failed HIP call.
#define HIP_TRY(expr)                                                    \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess) return omr::hip_error(#expr, _e);              \
  } while (0)
// The same for a call of the library's own that returns omr_status (its error text is already set).
#define OMR_TRY(expr)                \
  do {                               \
    omr_status _s = (expr);          \
    if (_s != OMR_OK) return _s;     \
  } while (0)

namespace omr {

inline omr_status hip_error(const char *what, hipError_t e) {
  return set_error(e == hipErrorOutOfMemory ? OMR_ERR_OUT_OF_MEMORY : OMR_ERR_DEVICE,
                   std::string(what) + ": " + hipGetErrorString(e));
}

// An environment switch that is on unless set to a value starting with '0'.
inline bool env_off(const char *name) {
  const char *v = getenv(name);
  return v && v[0] == '0';
}

// Move-only owner of one device allocation of T (freed on every path; a failing hipFree leaves
// nothing to recover). Converts to T* so that kernel launches and copies read as with raw pointers.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { reset(); }

  void reset() {
    if (p_) (void)hipFree((void *)p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // A fresh allocation of n elements (the previous one is freed first).
  hipError_t alloc(size_t n) {
    reset();
    const hipError_t e = hipMalloc(&p_, n * sizeof(T));
    if (e == hipSuccess) cap_ = n;
    else p_ = nullptr;
    return e;
  }
  // Growable scratch: frees and reallocates only when n exceeds the capacity. The caller makes sure
  // that no stream still uses the old allocation when !fits(n).
  bool fits(size_t n) const { return n <= cap_; }
  hipError_t reserve(size_t n) { return fits(n) ? hipSuccess : alloc(n); }
  // Allocate (at least one element) and copy n host elements: enqueued on st, or blocking.
  hipError_t upload(const T *src, size_t n, hipStream_t st) {
    const hipError_t e = alloc(n ? n : 1);
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpyAsync(p_, src, n * sizeof(T), hipMemcpyHostToDevice, st);
  }
  hipError_t upload(const std::vector<T> &v, hipStream_t st) { return upload(v.data(), v.size(), st); }
  hipError_t upload_sync(const T *src, size_t n) {
    const hipError_t e = alloc(n ? n : 1);
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
  }
  hipError_t upload_sync(const std::vector<T> &v) { return upload_sync(v.data(), v.size()); }

  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t capacity() const { return cap_; }

 private:
  T *p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace omr
