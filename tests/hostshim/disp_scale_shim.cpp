// Host build of the fixed-point scale rules of the dispersion brick spreads (admp_amd/csrc/disp_math.h
// scalar_spread_exponent, typed_spread_exponent); tests/test_disp_scale_cpu.py.
#include <cstdint>

#include "../../admp_amd/csrc/disp_math.h"

extern "C" {
// bmax as the kernel forms it: the float maximum of |c| times 1.0001f, widened to double
void disp_scale_scalar(int single, int n, const float* cmax, const int32_t* cnt, int32_t* ex, double* bmax) {
  for (int i = 0; i < n; ++i) {
    const float b = cmax[i] > 0.f ? cmax[i] * 1.0001f : 0.f;
    bmax[i] = (double)b;
    ex[i] = admp::scalar_spread_exponent(single != 0, (double)b, cnt[i]);
  }
}
void disp_scale_typed(int single, int n, const int32_t* cnt, int32_t* ex) {
  for (int i = 0; i < n; ++i) ex[i] = admp::typed_spread_exponent(single != 0, cnt[i]);
}
}
