// Random source of the MD drivers' thermostat (md_kernels.hip k_md_langevin / k_md_random), host and device: the counter-based
// generator Philox-4x32 with ten rounds (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and
// three standard normals per atom from one call of it.  Every word is a function of (seed, step, stream, atom) alone -- not of
// the grid, the launch order or an earlier call -- so a trajectory restarted at any step draws the same noise again, and
// tests/md_random_shim compiles this header with a host compiler against the generator's published known answers.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef ADMP_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ADMP_HD __host__ __device__ __forceinline__
#else
#define ADMP_HD inline
#endif
#endif

namespace admp {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;      // Weyl increments of the key
// streams of the drivers: the thermostat's noise, the initial velocities, the barostat's noise and the velocity-rescaling
// thermostat's (md_vrescale_math.h) never share a counter
constexpr uint32_t kStreamLangevin = 0, kStreamMaxwell = 1, kStreamBarostat = 2, kStreamVRescale = 3;

ADMP_HD uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

ADMP_HD void philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
    const uint32_t hi1 = mulhi32(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1;
    c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += kPhiloxW0; k1 += kPhiloxW1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// counter = (atom, step low, step high, stream), key = (seed low, seed high)
ADMP_HD void md_random_words(uint64_t seed, uint64_t step, uint32_t stream, uint32_t atom, uint32_t w[4]) {
  const uint32_t counter[4] = {atom, (uint32_t)(step & 0xffffffffu), (uint32_t)(step >> 32), stream};
  const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
  philox4x32_10(counter, key, w);
}

// Box-Muller on u_k = (w_k + 1/2) 2^-32 in (0, 1): in double whatever the caller's precision (it rounds last), so single- and
// double-precision runs see the same noise; u >= 2^-33 bounds |xi| by sqrt(66 ln 2) = 6.77 without a clamp.
ADMP_HD void md_random_normals(uint64_t seed, uint64_t step, uint32_t stream, uint32_t atom, double xi[3]) {
  uint32_t w[4];
  md_random_words(seed, step, stream, atom, w);
  const double s = 1.0 / 4294967296.0, two_pi = 6.283185307179586476925286766559;
  const double u0 = ((double)w[0] + 0.5) * s, u1 = ((double)w[1] + 0.5) * s, u2 = ((double)w[2] + 0.5) * s,
               u3 = ((double)w[3] + 0.5) * s;
  const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
  xi[0] = r0 * cos(two_pi * u1);
  xi[1] = r0 * sin(two_pi * u1);
  xi[2] = r1 * cos(two_pi * u3);
}

}  // namespace admp
