// Per-item arithmetic of the harmonic bonded terms and the per-atom updates of the multiple-time-step integrator
// (mts_kernels.hip k_md_mts), host and device: the kernel and the host program of tests/mts_shim compile this text.  The
// formulas are those of md_kernels.hip k_md_bonded -- minimum-image vectors, the clamp of cos theta, the floor of sin theta,
// acos in double -- with the item's contributions returned instead of added to the gradient with atomics.
#pragma once
#include "md_math.h"
#include "pme_math.h"

namespace admp {

// bond (i, j; k, r0): g = dE/dr_j = -dE/dr_i (kJ/mol/A); returns the energy in double
template <class T>
ADMP_HD double md_bond_item(const Box<T>& box, const T* ri, const T* rj, T k, T r0, T g[3]) {
  T d[3] = {rj[0] - ri[0], rj[1] - ri[1], rj[2] - ri[2]};
  min_image(box, d);
  const T r = m_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const T dr = r - r0;
  const T s = k * dr / r;                      // dE/dr / r
  for (int c = 0; c < 3; ++c) g[c] = s * d[c];
  return 0.5 * (double)k * (double)dr * (double)dr;
}

// angle (i, centre j, k; k_theta, theta0): gu = dE/dr_i, gv = dE/dr_k; the centre takes -(gu + gv)
template <class T>
ADMP_HD double md_angle_item(const Box<T>& box, const T* ri, const T* rj, const T* rk, T kt, T th0, T gu[3], T gv[3]) {
  T u[3] = {ri[0] - rj[0], ri[1] - rj[1], ri[2] - rj[2]};
  T v[3] = {rk[0] - rj[0], rk[1] - rj[1], rk[2] - rj[2]};
  min_image(box, u);
  min_image(box, v);
  const T ru = m_sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), rv = m_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  T c = (u[0] * v[0] + u[1] * v[1] + u[2] * v[2]) / (ru * rv);
  c = c > T(1) ? T(1) : (c < T(-1) ? T(-1) : c);
  const T th = (T)acos((double)c), dth = th - th0;
  // d theta / d u = -(v / (ru rv) - c u / ru^2) / sin theta
  T sn = m_sqrt(T(1) - c * c);
  sn = sn < T(1e-8) ? T(1e-8) : sn;
  const T f = -kt * dth / sn;
  for (int q = 0; q < 3; ++q) {
    gu[q] = f * (v[q] / (ru * rv) - c * u[q] / (ru * ru));
    gv[q] = f * (u[q] / (ru * rv) - c * v[q] / (rv * rv));
  }
  return 0.5 * (double)kt * (double)dth * (double)dth;
}

// How an atom refers to a force slot of its tile (mts_plan.h): reference = 4 * slot + kind.  A bond fills one slot (g of
// md_bond_item), an angle two consecutive ones (gu, gv).
constexpr int kMtsRefPlus = 0, kMtsRefMinus = 1, kMtsRefCentre = 2;      // + slot; - slot; -(slot + next slot)

// g[3] += the contribution a reference names, from the tile's slots (3 numbers each)
template <class T>
ADMP_HD void md_mts_add_ref(const T* slots, int ref, T g[3]) {
  const T* s = slots + 3 * (ref >> 2);
  const int kind = ref & 3;
  for (int c = 0; c < 3; ++c) g[c] += kind == kMtsRefPlus ? s[c] : (kind == kMtsRefMinus ? -s[c] : -(s[c] + s[3 + c]));
}

// The per-atom updates of one step (units of md_kernels.hip: half_dt_acc = (dt / 2) 1e-4).
template <class T>
ADMP_HD void md_mts_kick(T v[3], const T g[3], T im, T half_dt_acc) {
  for (int c = 0; c < 3; ++c) v[c] -= half_dt_acc * g[c] * im;
}
// A, O, A of an inner BAOAB step; noisy == false (c1 = 1) draws nothing.  xi is computed in double and rounded last.
template <class T>
ADMP_HD void md_mts_drift(T r[3], T v[3], T half_dt, bool noisy, T c1, T sig, uint64_t seed, uint64_t step, uint32_t atom) {
  for (int c = 0; c < 3; ++c) r[c] += half_dt * v[c];
  if (noisy) {
    double xi[3];
    md_random_normals(seed, step, kStreamLangevin, atom, xi);
    for (int c = 0; c < 3; ++c) v[c] = c1 * v[c] + sig * (T)xi[c];
  }
  for (int c = 0; c < 3; ++c) r[c] += half_dt * v[c];
}

}  // namespace admp
