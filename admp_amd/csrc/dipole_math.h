// Arithmetic of the dipole observable (dipole_kernels.hip; include/admp_hip.h admp_pme_dipoles), host and device: the kernel and
// the host program of tests/dipole_shim compile this text.  Groups are the labels of admp_amd.md.groups_of; a group's anchor a is
// its lowest-numbered atom (the first of its list), groups are narrower than half the cell, and an atom may be wrapped into the
// cell independently of its group.  For atom i of group c:
//
//   d_i  = minimum image of r_i - r_a  (md_mol_image: exactly r_i - r_a when no translation was applied)
//   D_c  = sum m_i d_i / M_c           (the centre of mass, seen from the anchor)
//   p_i  = x_loc X_i + y_loc Y_i + z_loc Z_i,  (z_loc, x_loc, y_loc) = Q_local[i, 1:4] (harmonics 10, 11c, 11s) and X_i, Y_i, Z_i
//          the frame rows of local_frame_fwd (frame_math.h), gathered as frame_of (atom_kernels.hip) gathers them
//   U_i  = the induced dipole, global Cartesian already; zero without an array
//   mu_c = sum_i [ q_i (d_i - D_c) + p_i + U_i ],  q_i = Q_local[i, 0]
//
// A neutral group's mu_c does not depend on the origin; a charged group's is taken about its centre of mass; a single atom gives
// p_i + U_i.  M = sum_c mu_c: the itinerant term q_c R_c of charged groups is NOT part of it (it has no definition under periodic
// boundaries).  Unit: that of Q_local, e A for positions in A.
// The frames and d_i are formed in T; every product and every sum runs in double, in list order, whatever T.
#pragma once
#include "frame_math.h"
#include "md_mol_math.h"

namespace admp {

constexpr int kDipoleOutWords = 16;   // admp_pme_dipoles out16: M charge (3), permanent (3), induced (3), sum |mu|, sum |mu|^2,
                                      // max |mu|, n_groups, 0, 0, 0
constexpr int kDipoleRowWords = 12;   // one workgroup's partial row: the first twelve of them
constexpr int kDipoleSumWords = 11;   // ... of which the first eleven are sums and the twelfth a maximum

// the frame of atom i: the gather of frame_of (atom_kernels.hip) -- a site without a z atom has the identity frame
template <class T>
ADMP_HD void dipole_frame(const int* axis_type, const int* axis_idx, const T* pos, const Box<T>& box, int i, FrameWork<T>& w) {
  int type = axis_type[i];
  const int iz = axis_idx[3 * i], ix = axis_idx[3 * i + 1], iy = axis_idx[3 * i + 2];
  T p[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}, pz[3] = {0, 0, 0}, px[3] = {0, 0, 0}, py[3] = {0, 0, 0};
  if (iz >= 0) { pz[0] = pos[3 * iz]; pz[1] = pos[3 * iz + 1]; pz[2] = pos[3 * iz + 2]; } else if (type != NoAxisType) type = NoAxisType;
  if (ix >= 0) { px[0] = pos[3 * ix]; px[1] = pos[3 * ix + 1]; px[2] = pos[3 * ix + 2]; }
  if (iy >= 0) { py[0] = pos[3 * iy]; py[1] = pos[3 * iy + 1]; py[2] = pos[3 * iy + 2]; }
  local_frame_fwd(type, box, p, pz, px, py, w);
}

// p_i in global Cartesian axes from the nine local harmonics of the atom
template <class T>
ADMP_HD void dipole_permanent(const T* ql, const FrameWork<T>& w, double p[3]) {
  const double z = (double)ql[1], x = (double)ql[2], y = (double)ql[3];
  for (int c = 0; c < 3; ++c) p[c] = x * (double)w.X[c] + y * (double)w.Y[c] + z * (double)w.Z[c];
}

// what one lane does for a group: its n atoms (list order, the anchor first) walked twice -- the masses for D_c, then the three
// parts.  An index outside 0 .. n_atoms - 1 is passed over (a list the caller did not check must not read out of bounds).
// part: charge (3), permanent (3), induced (3) of mu_c.  U may be null.
template <class T>
ADMP_HD void dipole_group(const int* axis_type, const int* axis_idx, int n_atoms, const T* pos, const Box<T>& box, const T* Ql,
                          const T* U, const T* inv_mass, const int* atoms, int n, double part[9]) {
  for (int k = 0; k < 9; ++k) part[k] = 0.0;
  if (n <= 0) return;
  const int a = atoms[0];
  if (a < 0 || a >= n_atoms) return;
  const T ra[3] = {pos[3 * a], pos[3 * a + 1], pos[3 * a + 2]};
  double M = 0.0, D[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < n; ++k) {
    const int i = atoms[k];
    if (i < 0 || i >= n_atoms) continue;
    T d[3], s[3];
    md_mol_image(box, pos + 3 * i, ra, d, s);
    const double m = 1.0 / (double)inv_mass[i];
    M += m;
    for (int c = 0; c < 3; ++c) D[c] += m * (double)d[c];
  }
  for (int c = 0; c < 3; ++c) D[c] /= M;
  for (int k = 0; k < n; ++k) {
    const int i = atoms[k];
    if (i < 0 || i >= n_atoms) continue;
    T d[3], s[3];
    md_mol_image(box, pos + 3 * i, ra, d, s);
    const double q = (double)Ql[9 * i];
    FrameWork<T> w;
    dipole_frame(axis_type, axis_idx, pos, box, i, w);
    double p[3];
    dipole_permanent(Ql + 9 * i, w, p);
    for (int c = 0; c < 3; ++c) {
      part[c] += q * ((double)d[c] - D[c]);
      part[3 + c] += p[c];
      if (U) part[6 + c] += (double)U[3 * i + c];
    }
  }
}

// mu_c and its length from the three parts
ADMP_HD double dipole_total(const double part[9], double mu[3]) {
  for (int c = 0; c < 3; ++c) mu[c] = part[c] + part[3 + c] + part[6 + c];
  return sqrt(mu[0] * mu[0] + mu[1] * mu[1] + mu[2] * mu[2]);
}

}  // namespace admp
