// The least a translation unit outside engine.hip needs from a handle: where it runs, how it is timed, and a slot for state of
// its own that dies with the handle.  EngineBase (engine.hip) derives from HandleCtx; md_driver.hip, mesh_conv.hip and pair_list.hip see
// a handle through it.
#pragma once
#include <memory>
#include <type_traits>

#include "host_util.h"

struct admp_handle;

namespace admp {

// state a driver outside engine.hip keeps on a handle (md_driver.hip MdDriver)
struct HandleExt {
  virtual ~HandleExt() {}
};

struct HandleCtx {
  int device = 0;
  int prec = 8;
  hipStream_t stream = nullptr;   // admp_set_stream / admp_use_default_stream may change it between calls: read it at every call
  bool own_stream = false;
  Profiler prof;
  int srank = 0, snranks = 1;     // x-slab decomposition (admp_slab_configure)
  std::unique_ptr<HandleExt> md;  // the MD driver, created by the first admp_md_* call
};

// runs fn(ctx, arg) as every entry point of engine.hip runs its body (guarded): device set, stale errors dropped, the launch
// check afterwards, Err turned into the return code and the text of admp_last_error
__attribute__((visibility("hidden"))) int handle_call(admp_handle* h, void (*fn)(HandleCtx&, void*), void* arg);

// ... with a callable taking HandleCtx&: no allocation, the callable lives in the caller's frame
template <class F>
inline int handle_call(admp_handle* h, F&& f) {
  using Fn = typename std::remove_reference<F>::type;
  return handle_call(h, [](HandleCtx& c, void* a) { (*static_cast<Fn*>(a))(c); }, (void*)&f);
}

}  // namespace admp
