// pm_devbuf.hpp -- the one owner of device memory a handle holds.  Host only: a DevBuf never travels to a kernel (the
// structs that do -- PlaneSet, BlurBatch, BgrSource ... -- keep plain pointers, filled through the conversion below).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <utility>

namespace pm {

// what all DevBufs of the process hold right now (include/pm/testing.h: pm_debug_live_device_*)
inline std::atomic<long long> g_devbuf_allocations{0}, g_devbuf_bytes{0};

// Move-only owner of one hipMalloc allocation of capacity() bytes; converts to T* wherever a pointer is read.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {  // what this held goes with `o`
    std::swap(p_, o.p_);
    std::swap(bytes_, o.bytes_);
    return *this;
  }
  ~DevBuf() { (void)release(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t capacity() const { return bytes_; }

  hipError_t alloc(size_t bytes) {  // the buffer must be empty
    if (p_) return hipErrorInvalidValue;
    const hipError_t e = hipMalloc((void**)&p_, bytes);
    if (e != hipSuccess) {
      p_ = nullptr;
      return e;
    }
    bytes_ = bytes;
    g_devbuf_allocations += 1;
    g_devbuf_bytes += (long long)bytes;
    return hipSuccess;
  }
  // allocation and clear of the SAME bytes (the clear is enqueued on `stream`)
  hipError_t alloc_zeroed(size_t bytes, hipStream_t stream) {
    const hipError_t e = alloc(bytes);
    return e != hipSuccess ? e : hipMemsetAsync(p_, 0, bytes, stream);
  }
  // Grow only: nothing happens while `bytes` fit.  Otherwise `stream` is synchronised first (the old buffer may still be
  // in use), the contents are lost, and a failed allocation leaves the buffer empty.  *reallocated: whether that happened.
  hipError_t reserve(size_t bytes, hipStream_t stream, bool* reallocated = nullptr) {
    if (reallocated) *reallocated = false;
    if (bytes <= bytes_) return hipSuccess;
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    if (reallocated) *reallocated = true;
    e = release();
    return e != hipSuccess ? e : alloc(bytes);
  }
  hipError_t release() {
    if (!p_) return hipSuccess;
    g_devbuf_allocations -= 1;
    g_devbuf_bytes -= (long long)bytes_;
    bytes_ = 0;
    return hipFree(std::exchange(p_, nullptr));
  }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

}  // namespace pm
