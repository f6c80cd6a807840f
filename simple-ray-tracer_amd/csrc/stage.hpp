// stage.hpp -- the scaffold the stage objects share (query.hip, refit.hip, denoise.hip, temporal.hip, surface.hip;
// included by nothing else): the HIP error macro, the device and stream an object runs on, and the ownership of its device
// allocations.  The host-only helpers are stage_host.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <utility>

#include "srt_internal.hpp"
#include "stage_host.hpp"

#define STAGE_HIP_OK(expr)                                                    \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) {                                                   \
      srt::SetError(std::string(#expr) + ": " + hipGetErrorString(e_));       \
      return SRT_ERR_HIP;                                                     \
    }                                                                         \
  } while (0)

namespace srt {
namespace stage {

// A device allocation that frees itself.  Move-only; reads as the plain pointer.
template <class T>
class DevPtr {
 public:
  DevPtr() = default;
  DevPtr(DevPtr&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DevPtr& operator=(DevPtr&& o) noexcept {
    if (this != &o) {
      Free();
      p_ = std::exchange(o.p_, nullptr);
    }
    return *this;
  }
  ~DevPtr() { Free(); }
  hipError_t Alloc(size_t bytes) {
    Free();
    return hipMalloc(&p_, bytes);
  }
  void Free() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
};

// A ping-pong pair of `bytes` each, or neither: on failure `pair` is as it was.
template <class T>
hipError_t AllocPair(DevPtr<T> (&pair)[2], size_t bytes) {
  DevPtr<T> a, b;
  hipError_t e = a.Alloc(bytes);
  if (e == hipSuccess) e = b.Alloc(bytes);
  if (e != hipSuccess) return e;
  pair[0] = std::move(a);
  pair[1] = std::move(b);
  return hipSuccess;
}

// The base of the four srt_* objects: the device, and the caller's stream or one of the object's own.
struct Stage {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;

  int Acquire(int dev, void* caller_stream) {
    device = dev;
    stream = static_cast<hipStream_t>(caller_stream);
    STAGE_HIP_OK(hipSetDevice(device));
    if (!stream) {
      STAGE_HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      own_stream = true;
    }
    return SRT_OK;
  }
  // Waits for the work on the stream; only then may the object's allocations go.
  void Release() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
  }
};

inline void* StreamOf(const Stage* s) { return s ? s->stream : nullptr; }

// Owns an object from `new` until srt_*_create hands it out, and ends one in srt_*_destroy: Release, then the
// members' destructors free the allocations.
struct Destroy {
  template <class T>
  void operator()(T* obj) const {
    obj->Release();
    delete obj;
  }
};
template <class T>
using Owned = std::unique_ptr<T, Destroy>;

}  // namespace stage
}  // namespace srt
