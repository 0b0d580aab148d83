// The collectives of a slab-decomposed evaluation: the caller's callbacks (admp_set_comm) or the native RCCL communicator
// (admp_set_comm_rccl, rccl_comm.hip), behind three calls.  Every rank makes the same calls in the same order.  The engine's
// halo exchanges (engine.hip) and the ghost / transpose exchanges of the mesh convolution (mesh_conv.hip) go through here.
#pragma once
#include <string>

#include "../../include/admp_hip.h"
#include "err.h"
#include "rccl_comm.h"

namespace admp {

struct Comm {
  admp_comm cb{};               // the caller's communicator of the x-slab decomposition (admp_set_comm); unused with one rank
  bool have = false;
  admp_rccl* rccl = nullptr;    // native communicator (admp_set_comm_rccl): the collectives go straight to RCCL on the stream given
  void fail(const char* what, int rc) const {
    if (rccl) throw Err{ADMP_E_COMM, std::string(what) + ": " + rccl_error()};
    throw Err{ADMP_E_COMM, std::string("communicator callback ") + what + " returned " + std::to_string(rc)};
  }
  void all_reduce(hipStream_t st, void* buf, int64_t n, int dtype, int op, int tag) const {
    const int rc = rccl ? rccl_all_reduce(rccl, st, buf, n, dtype, op, tag) : cb.all_reduce(cb.ctx, buf, n, dtype, op, tag);
    if (rc != 0) fail("all_reduce", rc);
  }
  void all_to_all_v(hipStream_t st, const void* send, const int64_t* sc, void* recv, const int64_t* rc_, int dtype, int tag) const {
    const int rc = rccl ? rccl_all_to_all_v(rccl, st, send, sc, recv, rc_, dtype, tag)
                        : cb.all_to_all_v(cb.ctx, send, sc, recv, rc_, dtype, tag);
    if (rc != 0) fail("all_to_all_v", rc);
  }
  void shift(hipStream_t st, const void* send, void* recv, int64_t n, int dtype, int to_next, int tag) const {
    const int rc = rccl ? rccl_shift(rccl, st, send, recv, n, dtype, to_next, tag)
                        : cb.shift(cb.ctx, send, recv, n, dtype, to_next, tag);
    if (rc != 0) fail("shift", rc);
  }
};

}  // namespace admp
