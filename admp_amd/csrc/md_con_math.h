// Arithmetic of the distance constraints (con_kernels.hip), host and device: the kernels and the host program of
// tests/con_shim compile this text.  Constrained BAOAB in the splitting of OpenMM's LangevinMiddleIntegrator: the first half
// of a step solves SHAKE on the DISPLACEMENT delta of the step (a few 1e-2 A, against coordinates of tens of A: accurate in
// single precision, and no minimum image of the moved positions is needed), the second half solves RATTLE on the velocities.
// For a constraint (i, j, d): s = minimum image of x_j - x_i at the reference positions.
//
//   SHAKE    p = b + delta_j - delta_i (b = s in a step; in a projection the vector between the positions being moved),
//            diff = d^2 - |p|^2;  converged: |diff| <= 2 tol d^2;  else g = diff / (2 (1/m_i + 1/m_j) (s.p)),
//            delta_i -= (g/m_i) s, delta_j += (g/m_j) s.  s.p <= 0: no update, the cluster has failed (the reference
//            direction is useless and g unbounded).
//   RATTLE   dot = s.(v_j - v_i);  converged: |dot| dt <= tol d^2;  else k = dot / (|s|^2 (1/m_i + 1/m_j)),
//            v_i += (k/m_i) s, v_j -= (k/m_j) s.
//
// A cluster's constraints are swept in the plan's order (con_plan.h) until one whole sweep finds every constraint converged,
// at most max_sweeps times: no input can keep the loop running.  A converged constraint is left untouched.
#pragma once
#include "md_bonded_math.h"

namespace admp {

// s = minimum image of rj - ri
template <class T>
ADMP_HD void md_con_vector(const Box<T>& box, const T* ri, const T* rj, T s[3]) {
  s[0] = rj[0] - ri[0]; s[1] = rj[1] - ri[1]; s[2] = rj[2] - ri[2];
  min_image(box, s);
}

// one constraint of a SHAKE sweep on x (3 numbers per slot); tol2 = 2 tol.  Returns true when it is converged (x unchanged);
// bad is set when s.p <= 0 (or not a number)
template <class T>
ADMP_HD bool md_con_shake(T* xi, T* xj, const T* s, const T* b, T imi, T imj, T d2, T tol2, bool& bad) {
  const T p0 = b[0] + (xj[0] - xi[0]), p1 = b[1] + (xj[1] - xi[1]), p2 = b[2] + (xj[2] - xi[2]);
  const T diff = d2 - (p0 * p0 + p1 * p1 + p2 * p2);
  if (m_abs(diff) <= tol2 * d2) return true;
  const T sp = s[0] * p0 + s[1] * p1 + s[2] * p2;
  if (!(sp > T(0))) { bad = true; return false; }
  const T g = diff / (T(2) * (imi + imj) * sp);
  const T gi = g * imi, gj = g * imj;
  for (int c = 0; c < 3; ++c) { xi[c] -= gi * s[c]; xj[c] += gj * s[c]; }
  return false;
}

// one constraint of a RATTLE sweep on v; tol_dt = tol / dt.  Returns true when it is converged (v unchanged).  |s|^2 = 0 gives
// dot = 0, which is converged: no division by zero.
template <class T>
ADMP_HD bool md_con_rattle(T* vi, T* vj, const T* s, T imi, T imj, T d2, T tol_dt) {
  const T dot = s[0] * (vj[0] - vi[0]) + s[1] * (vj[1] - vi[1]) + s[2] * (vj[2] - vi[2]);
  if (m_abs(dot) <= tol_dt * d2) return true;
  const T k = dot / ((s[0] * s[0] + s[1] * s[1] + s[2] * s[2]) * (imi + imj));
  const T ki = k * imi, kj = k * imj;
  for (int c = 0; c < 3; ++c) { vi[c] += ki * s[c]; vj[c] -= kj * s[c]; }
  return false;
}

// What one lane does for a cluster: its constraints q0 .. q1 of the tile (slot: 2 local slots each) swept over x until a
// whole sweep changes nothing.  Returns the number of sweeps made; failed: max_sweeps reached without convergence, or a
// SHAKE update refused (the sweeping stops there).  A cluster without constraints makes no sweep and has not failed.
template <class T>
ADMP_HD int md_con_solve_shake(T* x, const T* im, const int* slot, const T* d2, const T* s, const T* b, int q0, int q1, T tol2,
                               int max_sweeps, bool& failed) {
  failed = false;
  if (q1 <= q0) return 0;
  bool done = false, bad = false;
  int sweeps = 0;
  while (sweeps < max_sweeps && !done && !bad) {
    done = true;
    for (int q = q0; q < q1 && !bad; ++q) {
      const int i = slot[2 * q], j = slot[2 * q + 1];
      if (!md_con_shake(x + 3 * i, x + 3 * j, s + 3 * q, b + 3 * q, im[i], im[j], d2[q], tol2, bad)) done = false;
    }
    sweeps += 1;
  }
  failed = !done;
  return sweeps;
}
template <class T>
ADMP_HD int md_con_solve_rattle(T* v, const T* im, const int* slot, const T* d2, const T* s, int q0, int q1, T tol_dt, int max_sweeps,
                                bool& failed) {
  failed = false;
  if (q1 <= q0) return 0;
  bool done = false;
  int sweeps = 0;
  while (sweeps < max_sweeps && !done) {
    done = true;
    for (int q = q0; q < q1; ++q) {
      const int i = slot[2 * q], j = slot[2 * q + 1];
      if (!md_con_rattle(v + 3 * i, v + 3 * j, s + 3 * q, im[i], im[j], d2[q], tol_dt)) done = false;
    }
    sweeps += 1;
  }
  failed = !done;
  return sweeps;
}

// The per-atom updates of the first half (units of md_kernels.hip: half_dt_acc = (dt / 2) 1e-4): B on v, then A, O, A on the
// displacement, which starts at zero -- delta = (dt/2) v; v = c1 v + sig xi; delta += (dt/2) v (md_mts_drift on delta; c1 = 1
// draws nothing).  The unconstrained displacement is what the caller keeps as delta_u.
template <class T>
ADMP_HD void md_con_half_step(T v[3], T delta[3], const T g[3], T im, T half_dt_acc, T half_dt, bool noisy, T c1, T sig,
                              uint64_t seed, uint64_t step, uint32_t atom) {
  md_mts_kick(v, g, im, half_dt_acc);
  delta[0] = delta[1] = delta[2] = T(0);
  md_mts_drift(delta, v, half_dt, noisy, c1, sig, seed, step, atom);
}
// after SHAKE: v += (delta - delta_u) / dt; r = r0 + delta
template <class T>
ADMP_HD void md_con_finish(T r[3], T v[3], const T r0[3], const T delta[3], const T delta_u[3], T dt) {
  for (int c = 0; c < 3; ++c) {
    v[c] += (delta[c] - delta_u[c]) / dt;
    r[c] = r0[c] + delta[c];
  }
}

}  // namespace admp
