// Growable device buffer that owns its allocation: freed when the buffer goes out of scope or its owner is destroyed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "err.h"

namespace admp {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;              // two owners of one allocation would free it twice
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void need(size_t n) {
    if (n <= bytes) return;
    if (p) HIP_TRY(hipFree(p));
    p = nullptr;
    bytes = 0;
    void* q = nullptr;                         // a failed allocation leaves {nullptr, 0} whatever hipMalloc wrote
    HIP_TRY(hipMalloc(&q, n));
    p = q;
    bytes = n;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class U> U* as() const { return reinterpret_cast<U*>(p); }
};

}  // namespace admp
