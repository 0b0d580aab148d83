// Host helpers shared by the translation units behind the C ABI (engine.hip, mesh_conv.hip, pair_list.hip, md_driver.hip): the error type and its macros
// (err.h), the per-label profiler, the box handed to the kernels and its heights.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "err.h"
#include "pme_math.h"

namespace admp {

// per-label launch timing with HIP events on the engine's stream
struct Profiler {
  bool on = false;
  std::string only;   // when non-empty, only sections with exactly this label are bracketed
  struct Rec { int label; hipEvent_t a, b; };
  std::vector<std::string> labels;
  std::map<std::string, int> index;
  std::vector<double> total_ms;
  std::vector<int64_t> count;
  std::vector<Rec> pending;
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    return e;
  }
  int id(const char* name) {
    auto it = index.find(name);
    if (it != index.end()) return it->second;
    int k = (int)labels.size();
    labels.push_back(name); index[name] = k; total_ms.push_back(0.0); count.push_back(0);
    return k;
  }
  void begin(const char* name, hipStream_t st, Rec& r) {
    r.label = id(name); r.a = get(); r.b = get();
    HIP_TRY(hipEventRecord(r.a, st));
  }
  void end(hipStream_t st, Rec& r) {
    HIP_TRY(hipEventRecord(r.b, st));
    pending.push_back(r);
  }
  void collect(hipStream_t st) {
    if (pending.empty()) return;
    HIP_TRY(hipStreamSynchronize(st));
    for (auto& r : pending) {
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
      total_ms[r.label] += ms; count[r.label] += 1;
      pool.push_back(r.a); pool.push_back(r.b);
    }
    pending.clear();
  }
  void reset(hipStream_t st) {
    collect(st);
    for (auto& v : total_ms) v = 0.0;
    for (auto& v : count) v = 0;
  }
  void destroy() {
    for (auto& r : pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : pool) (void)hipEventDestroy(e);
    pending.clear(); pool.clear();
  }
};

struct Scoped {
  Profiler& p; hipStream_t st; Profiler::Rec r; bool active;
  Scoped(Profiler& p_, const char* name, hipStream_t st_) : p(p_), st(st_), active(p_.on && (p_.only.empty() || p_.only == name)) {
    if (active) p.begin(name, st, r);
  }
  ~Scoped() { if (active) p.end(st, r); }
};
#define TIMED(name) Scoped scoped_timer_(prof, name, stream)

inline void invert3(const double* h, double* inv, double* det) {
  double d = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
  inv[0] = (h[4] * h[8] - h[5] * h[7]) / d; inv[1] = (h[2] * h[7] - h[1] * h[8]) / d; inv[2] = (h[1] * h[5] - h[2] * h[4]) / d;
  inv[3] = (h[5] * h[6] - h[3] * h[8]) / d; inv[4] = (h[0] * h[8] - h[2] * h[6]) / d; inv[5] = (h[2] * h[3] - h[0] * h[5]) / d;
  inv[6] = (h[3] * h[7] - h[4] * h[6]) / d; inv[7] = (h[1] * h[6] - h[0] * h[7]) / d; inv[8] = (h[0] * h[4] - h[1] * h[3]) / d;
  *det = d;
}

template <class T>
Box<T> make_box(const double* h, double* inv, double* vol) {
  Box<T> b;
  invert3(h, inv, vol);
  ARG_CHECK(std::fabs(*vol) > 1e-12, "singular box");
  for (int k = 0; k < 9; ++k) { b.h[k] = (T)h[k]; b.hinv[k] = (T)inv[k]; }
  return b;
}

// perpendicular heights of the cell along its lattice directions: h[d] = 1 / |column d of box^-1|
inline void cell_heights(const double* inv, double* h) {
  for (int d = 0; d < 3; ++d) h[d] = 1.0 / std::sqrt(inv[0 + d] * inv[0 + d] + inv[3 + d] * inv[3 + d] + inv[6 + d] * inv[6 + d]);
}
// ... for a minimum-image cutoff rc, which must not exceed half of any of them
inline void cell_heights_within(const double* inv, double* h, double rc) {
  cell_heights(inv, h);
  for (int d = 0; d < 3; ++d) ARG_CHECK(rc <= 0.5 * h[d] * (1 + 1e-12), "rc exceeds half the box height (minimum image)");
}

}  // namespace admp
