// The error of the host code behind the C ABI: thrown anywhere below an entry point, turned into a return code and the text of
// admp_last_error at the boundary (engine.hip guarded).  One type for every translation unit of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/admp_hip.h"

namespace admp {

struct Err {
  int code;
  std::string msg;
};

#define HIP_TRY(x)                                                                                       \
  do {                                                                                                   \
    hipError_t e_ = (x);                                                                                 \
    if (e_ != hipSuccess) throw Err{ADMP_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)};          \
  } while (0)
#define ARG_CHECK(c, m) \
  do { if (!(c)) throw Err{ADMP_E_ARG, m}; } while (0)

}  // namespace admp
