// Arithmetic of the molecular (centre-of-mass) cell scaling (mol_kernels.hip), host and device: the kernels and the host
// program of tests/mol_shim compile this text.  A group's anchor a is its lowest-numbered atom; an atom may be wrapped into the
// cell independently of its group, and a group is smaller than half the cell.  For atom i of the group:
//
//   d_i = minimum image of r_i - r_a,  s_i = (r_i - r_a) - d_i  (the lattice translation the image applied; exactly zero when
//                                                                none was: image_shift of pme_math.h, as in k_md_bonded_box)
//   R_c = r_a + sum m_i d_i / M,  V_c = sum m_i v_i / M,  R_c(i) = R_c + s_i  (the image of the centre that belongs to atom i)
//
// One application with factor mu (box -> mu box):  r_i += (mu - 1) R_c(i),  v_i += (1/mu - 1) V_c.  The two factors come from
// the host in double (expm1); the products are formed in double and rounded to T once, so atoms of a group in the same image
// receive bitwise the same displacement, and relative velocities inside a group change by that one rounding only.
// The sums of a group run in double, in slot order, whatever T.
#pragma once
#include "pme_math.h"

namespace admp {

// d and s of one atom against its anchor
template <class T>
ADMP_HD void md_mol_image(const Box<T>& box, const T ri[3], const T ra[3], T d[3], T s[3]) {
  const T raw[3] = {ri[0] - ra[0], ri[1] - ra[1], ri[2] - ra[2]};
  image_shift(box, raw, s);
  for (int c = 0; c < 3; ++c) d[c] = raw[c] - s[c];
}

// what one lane does for a group: slots a0 .. a1 of the tile (d, v: 3 numbers per slot; im: 1/m per slot) summed in sequence.
// out: M, sum m d / M (3), sum m v / M (3)  (kMolGroupWords of mol_plan.h)
template <class T>
ADMP_HD void md_mol_group(const T* d, const T* v, const T* im, int a0, int a1, double out[7]) {
  double M = 0.0, md[3] = {0.0, 0.0, 0.0}, mv[3] = {0.0, 0.0, 0.0};
  for (int a = a0; a < a1; ++a) {
    const double m = 1.0 / (double)im[a];
    M += m;
    for (int c = 0; c < 3; ++c) { md[c] += m * (double)d[3 * a + c]; mv[c] += m * (double)v[3 * a + c]; }
  }
  out[0] = M;
  for (int c = 0; c < 3; ++c) { out[1 + c] = md[c] / M; out[4 + c] = mv[c] / M; }
}

// R_c(i) = (r_a + sum m d / M) + s_i
template <class T>
ADMP_HD void md_mol_centre(const T ra[3], const double grp[7], const T s[3], double Rc[3]) {
  for (int c = 0; c < 3; ++c) Rc[c] = ((double)ra[c] + grp[1 + c]) + (double)s[c];
}

// the two updates
template <class T>
ADMP_HD void md_mol_scale(T r[3], T v[3], const double Rc[3], const double grp[7], double mu_minus_1, double inv_mu_minus_1) {
  for (int c = 0; c < 3; ++c) {
    const T dr = (T)(mu_minus_1 * Rc[c]), dv = (T)(inv_mu_minus_1 * grp[4 + c]);
    r[c] += dr;
    v[c] += dv;
  }
}

}  // namespace admp
