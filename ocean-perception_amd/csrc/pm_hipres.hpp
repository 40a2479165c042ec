// pm_hipres.hpp -- the owners of everything else a handle takes from the runtime: events, streams, page-locked host
// memory, the instantiated graph.  Host only, shaped like DevBuf (pm_devbuf.hpp): empty by default, move-only, a create
// that needs the empty state, a conversion to the raw handle, release() with the runtime's answer, and a destructor that
// releases.  Each kind counts what the process holds right now (include/pm/testing.h: pm_debug_live_*).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <utility>

namespace pm {

inline std::atomic<long long> g_live_events{0}, g_live_streams{0}, g_live_host_buffers{0}, g_live_host_bytes{0},
    g_live_graph_execs{0};

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event& operator=(Event&& o) noexcept {  // what this held goes with `o`
    std::swap(e_, o.e_);
    return *this;
  }
  ~Event() { (void)release(); }

  operator hipEvent_t() const { return e_; }
  hipEvent_t get() const { return e_; }

  hipError_t create(unsigned flags) {  // hipEventDefault: a timed event
    if (e_) return hipErrorInvalidValue;
    const hipError_t e = hipEventCreateWithFlags(&e_, flags);
    if (e != hipSuccess) {
      e_ = nullptr;
      return e;
    }
    g_live_events += 1;
    return hipSuccess;
  }
  hipError_t release() {
    if (!e_) return hipSuccess;
    g_live_events -= 1;
    return hipEventDestroy(std::exchange(e_, nullptr));
  }

 private:
  hipEvent_t e_ = nullptr;
};

// A stream made by pm::eng::create_stream (pm_handle.hpp), which alone knows the priority classes.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
  Stream& operator=(Stream&& o) noexcept {
    std::swap(s_, o.s_);
    return *this;
  }
  ~Stream() { (void)release(); }

  operator hipStream_t() const { return s_; }
  hipStream_t get() const { return s_; }

  hipError_t adopt(hipStream_t s) {
    if (s_ || !s) return hipErrorInvalidValue;
    s_ = s;
    g_live_streams += 1;
    return hipSuccess;
  }
  hipError_t release() {
    if (!s_) return hipSuccess;
    g_live_streams -= 1;
    return hipStreamDestroy(std::exchange(s_, nullptr));
  }

 private:
  hipStream_t s_ = nullptr;
};

// Page-locked host memory: allocated here (alloc) or the caller's own, locked in place (lock) and only unlocked again by
// release().  dev(): the device's address of base(), null where the runtime maps none.
class HostBuf {
 public:
  HostBuf() = default;
  HostBuf(HostBuf&& o) noexcept
      : p_(std::exchange(o.p_, nullptr)), dev_(std::exchange(o.dev_, nullptr)), bytes_(std::exchange(o.bytes_, 0)),
        owned_(o.owned_) {}
  HostBuf& operator=(HostBuf&& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(dev_, o.dev_);
    std::swap(bytes_, o.bytes_);
    std::swap(owned_, o.owned_);
    return *this;
  }
  ~HostBuf() { (void)release(); }

  operator char*() const { return p_; }
  char* base() const { return p_; }
  char* dev() const { return dev_; }
  size_t bytes() const { return bytes_; }
  bool owned() const { return owned_; }

  hipError_t alloc(size_t bytes) {
    if (p_) return hipErrorInvalidValue;
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) hold(p, bytes, true);
    return e;
  }
  hipError_t lock(void* p, size_t bytes) {
    if (p_) return hipErrorInvalidValue;
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterMapped);
    if (e == hipSuccess) hold(p, bytes, false);
    return e;
  }
  hipError_t release() {
    if (!p_) return hipSuccess;
    g_live_host_buffers -= 1;
    g_live_host_bytes -= (long long)bytes_;
    bytes_ = 0;
    dev_ = nullptr;
    void* p = std::exchange(p_, nullptr);
    return owned_ ? hipHostFree(p) : hipHostUnregister(p);
  }

 private:
  void hold(void* p, size_t bytes, bool owned) {
    p_ = (char*)p;
    bytes_ = bytes;
    owned_ = owned;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, p, 0) == hipSuccess) dev_ = (char*)dp;
    (void)hipGetLastError();
    g_live_host_buffers += 1;
    g_live_host_bytes += (long long)bytes;
  }
  char *p_ = nullptr, *dev_ = nullptr;
  size_t bytes_ = 0;
  bool owned_ = true;
};

class GraphExec {
 public:
  GraphExec() = default;
  GraphExec(GraphExec&& o) noexcept : g_(std::exchange(o.g_, nullptr)) {}
  GraphExec& operator=(GraphExec&& o) noexcept {
    std::swap(g_, o.g_);
    return *this;
  }
  ~GraphExec() { (void)release(); }

  operator hipGraphExec_t() const { return g_; }

  hipError_t create(hipGraph_t graph) {
    if (g_) return hipErrorInvalidValue;
    const hipError_t e = hipGraphInstantiate(&g_, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
      g_ = nullptr;
      return e;
    }
    g_live_graph_execs += 1;
    return hipSuccess;
  }
  hipError_t release() {
    if (!g_) return hipSuccess;
    g_live_graph_execs -= 1;
    return hipGraphExecDestroy(std::exchange(g_, nullptr));
  }

 private:
  hipGraphExec_t g_ = nullptr;
};

}  // namespace pm
