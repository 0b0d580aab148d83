// Stand-in for the HIP runtime header, as far as admp_amd/csrc/dev_buf.h uses it: host allocations that are counted, and
// a switch that makes the next allocations fail (tests/devbuf_shim/main.cpp).
#pragma once
#include <cstddef>
#include <cstdlib>
#include <map>
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "invalid value"; }
struct StubHeap { std::map<void*, size_t> live; size_t bytes = 0; long mallocs = 0, frees = 0, bad_frees = 0; bool fail = false; };
inline StubHeap& stub_heap() { static StubHeap h; return h; }
inline hipError_t hipMalloc(void** p, size_t n) {
  StubHeap& h = stub_heap();
  if (h.fail) { *p = reinterpret_cast<void*>(0x1); return hipErrorOutOfMemory; }      // leaves rubbish behind, as a runtime may
  *p = std::malloc(n ? n : 1); h.live[*p] = n; h.bytes += n; h.mallocs += 1;
  return hipSuccess;
}
inline hipError_t hipFree(void* p) {
  StubHeap& h = stub_heap();
  if (!p) return hipSuccess;
  auto it = h.live.find(p);
  if (it == h.live.end()) { h.bad_frees += 1; return hipErrorInvalidValue; }      // a double free, or never allocated
  h.bytes -= it->second; h.live.erase(it); h.frees += 1; std::free(p);
  return hipSuccess;
}
