// Device-memory owners of the host engines: DeviceStore for what lives as long as an engine
// (weights, tables), Workspace for the named grow-only per-call buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace zasr {

class DeviceStore {
 public:
  DeviceStore() = default;
  DeviceStore(const DeviceStore&) = delete;
  DeviceStore& operator=(const DeviceStore&) = delete;
  ~DeviceStore() {  // best effort: errors here cannot be reported to the caller
    for (void* p : allocs_) (void)hipFree(p);
  }
  // a buffer a kernel fills (split / converted / packed weights, the decoder table)
  void* alloc(size_t bytes) {
    void* p = nullptr;
    ZASR_HIP_CHECK(hipMalloc(&p, bytes));
    allocs_.push_back(p);
    return p;
  }
  // a device copy of host[0, n) (at least one element is allocated)
  template <class T>
  T* upload(const T* host, size_t n) {
    T* p = static_cast<T*>(alloc(std::max<size_t>(n, 1) * sizeof(T)));
    ZASR_HIP_CHECK(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    return p;
  }
  template <class T>
  T* upload(const std::vector<T>& v) {
    return upload(v.data(), v.size());
  }

 private:
  std::vector<void*> allocs_;
};

class Workspace {
 public:
  Workspace() = default;
  Workspace(const Workspace&) = delete;
  Workspace& operator=(const Workspace&) = delete;
  ~Workspace() {
    for (auto& kv : bufs_)
      if (kv.second.p) (void)hipFree(kv.second.p);
  }
  // `count` elements under `name`, at least 256 bytes, grown with 1/8 slack.  A buffer that
  // grows is freed only after the work that may still read it: on `sync` when the engine
  // runs on that one stream, on the whole device when sync is null (buffers in use on several
  // streams).  Growth is rare.
  template <class T>
  T* get(const std::string& name, size_t count, const hipStream_t* sync) {
    const size_t bytes = std::max<size_t>(count * sizeof(T), 256);
    Buf& b = bufs_[name];
    if (b.bytes < bytes) {
      if (b.p) {
        ZASR_HIP_CHECK(sync ? hipStreamSynchronize(*sync) : hipDeviceSynchronize());
        ZASR_HIP_CHECK(hipFree(b.p));
        b = Buf{};
      }
      const size_t alloc = bytes + bytes / 8;
      ZASR_HIP_CHECK(hipMalloc(&b.p, alloc));
      b.bytes = alloc;
    }
    return reinterpret_cast<T*>(b.p);
  }
  // free every buffer; the caller has synchronised the work that used them
  void clear() {
    for (auto& kv : bufs_)
      if (kv.second.p) ZASR_HIP_CHECK(hipFree(kv.second.p));
    bufs_.clear();
  }

 private:
  struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
  };
  std::map<std::string, Buf> bufs_;
};

}  // namespace zasr
