// Rule of the stochastic velocity-rescaling thermostat (vrescale_kernels.hip k_md_vr_scale; admp_amd/md.py VRescale), host and
// device: Bussi, Donadio, Parrinello, "Canonical sampling through velocity rescaling", J. Chem. Phys. 126, 014101 (2007), in the
// closed form of its appendix.  One pure function in double: (state, K, Nf, kT, c, seed, step) -> (state, alpha).
// tests/vrescale_shim compiles this header with a host compiler against the numpy restatement of tests/vrescale_ref.py.
//
// With K = sum v^2 / (2 inv_mass) before scaling (the driver's internal unit: kJ/mol times 1e-4), Nf degrees of freedom,
// kT_acc = kB T 1e-4 and c = exp(-dt / tau):
//     K'    = ( sqrt(c K) + sqrt((1 - c) kT_acc / 2) R1 )^2 + (1 - c) (kT_acc / 2) S,    R1 ~ N(0, 1), S ~ chi^2(Nf - 1)
//     alpha = sqrt(K' / K) >= 0      (the sign convention of GROMACS: a velocity never turns round)
// K = 0 and c = 1 are answered without a draw: alpha = 1 exactly, K' = K.
//
// The noise is a function of (seed, step) alone, on the stream kStreamVRescale of md_math.h.  Counter index 0: R1 = xi[0], and
// S starts at xi[1]^2 if Nf - 1 is odd, at 0 otherwise.  a = (Nf - 1) div 2 >= 1 adds 2 Gamma(a) by the rejection method of
// Marsaglia and Tsang ("A simple method for generating gamma variables", ACM TOMS 26, 363, 2000): d = a - 1/3, q = 1 / sqrt(9 d);
// try t = 0, 1, ... takes x = xi[0] and u = (w[2] + 1/2) 2^-32 of counter index 1 + t (x is made of w[0] and w[1]: the two are
// independent), v = (1 + q x)^3, and accepts d v iff v > 0 and ln u < x^2 / 2 + d - d v + d ln v.  After kVrMaxTries
// rejections the application fails.
#pragma once
#include <cmath>
#include <cstdint>

#include "md_math.h"

namespace admp {

// words of the state (8 doubles a slot), as include/admp_hip.h admp_md_vrescale lists them
enum { VR_K_BEFORE = 0, VR_K_AFTER, VR_ALPHA, VR_HEAT, VR_APPLICATIONS, VR_TRIES, VR_RESERVED, VR_FLAGS, VR_STATE_WORDS };
constexpr double kVrFailed = 1.0;      // value of the flags word
constexpr int kVrMaxTries = 64;

// R1 and S of (seed, step) for n_dof >= 1.  Returns the tries the gamma deviate took (0 if none was needed), or -1 when
// kVrMaxTries of them were rejected.
ADMP_HD int md_vrescale_noise(uint64_t seed, uint64_t step, int64_t n_dof, double* R1, double* S) {
  double xi[3];
  md_random_normals(seed, step, kStreamVRescale, 0u, xi);
  *R1 = xi[0];
  const int64_t rest = n_dof - 1, a = rest / 2;
  *S = (rest & 1) ? xi[1] * xi[1] : 0.0;
  if (a < 1) return 0;
  const double d = (double)a - 1.0 / 3.0, q = 1.0 / sqrt(9.0 * d);
  for (int t = 0; t < kVrMaxTries; ++t) {
    uint32_t w[4];
    md_random_normals(seed, step, kStreamVRescale, (uint32_t)(1 + t), xi);
    md_random_words(seed, step, kStreamVRescale, (uint32_t)(1 + t), w);
    const double x = xi[0], u = ((double)w[2] + 0.5) * (1.0 / 4294967296.0);
    const double p = 1.0 + q * x, v = p * p * p;
    if (v > 0.0 && log(u) < 0.5 * x * x + d - d * v + d * log(v)) {
      *S += 2.0 * d * v;
      return t + 1;
    }
  }
  return -1;
}

// One application for velocities of type T: `out` is the next state and the return value the factor in double -- the caller
// multiplies by (T)alpha, and out[VR_K_AFTER] is the kinetic energy of exactly those velocities, ((double)(T)alpha)^2 K.
// *scale = 0 tells the caller to leave the velocities alone: failed before (out = in) or now (out = in with the flag: a K that
// is not finite, a factor that is not finite, or a draw out of tries).
template <class T>
ADMP_HD double md_vrescale_rule(const double* in, double K, int64_t n_dof, double kT_acc, double c, uint64_t seed, uint64_t step,
                                double* out, int* scale) {
  for (int w = 0; w < VR_STATE_WORDS; ++w) out[w] = in[w];
  *scale = 0;
  if (in[VR_FLAGS] == kVrFailed) return 1.0;
  if (!std::isfinite(K)) {
    out[VR_FLAGS] = kVrFailed;
    return 1.0;
  }
  double alpha = 1.0, tries = 0.0;
  if (K > 0.0 && c < 1.0) {
    double R1, S;
    const int t = md_vrescale_noise(seed, step, n_dof, &R1, &S);
    const double g = (1.0 - c) * (0.5 * kT_acc);
    const double r = sqrt(c * K) + sqrt(g) * R1;
    alpha = sqrt((r * r + g * S) / K);
    if (t < 0 || !std::isfinite(alpha)) {
      out[VR_FLAGS] = kVrFailed;
      return 1.0;
    }
    tries = (double)t;
  }
  const double at = (double)(T)alpha;
  const double K_after = at * at * K;
  out[VR_K_BEFORE] = K;
  out[VR_K_AFTER] = K_after;
  out[VR_ALPHA] = alpha;
  out[VR_HEAT] = in[VR_HEAT] + (K_after - K);
  out[VR_APPLICATIONS] = in[VR_APPLICATIONS] + 1.0;
  out[VR_TRIES] = tries;
  out[VR_RESERVED] = 0.0;
  *scale = 1;
  return alpha;
}

}  // namespace admp
