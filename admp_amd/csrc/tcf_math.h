// Arithmetic of the time correlation functions (tcf_kernels.hip; include/admp_hip.h admp_md_tcf), host and device: the kernels
// and the host program of tests/tcf_shim compile this text.
//
//   unwrap   every slot keeps the last position it saw (handle's precision) and a double accumulator d, its displacement since
//            the recorder's first frame.  A frame adds the minimum image, taken in the cell of THAT frame, of pos - last: under
//            a changing cell (NPT) the displacement between two frames is the minimum image in the newer cell.  All of it in
//            double whatever the handle's precision (the conversion of a float is exact), so d does not depend on whether the
//            caller wraps atoms into the cell: the lattice vectors a wrap adds are removed again.
//   jump     a fractional component of the minimum image of pos - last with |s| >= 0.25 is a move of a quarter of a cell height
//            or more between two frames, too close to the half height at which it cannot be told from the opposite move of the
//            periodic image.  The test is on the fractional components once the whole lattice vectors are gone and before they
//            are turned back into a Cartesian move: a caller who wraps atoms into the cell adds whole lattice vectors to
//            pos - last, and those are no jumps.  Counted, still applied.
//   ring     d is rounded once from the accumulator to the handle's precision; v is copied unchanged.
//   terms    of a slot at the lag k: |d(t) - d(t - k)|^2 and v(t) . v(t - k), in double from the ring's words (exact
//            conversions): differences, squares, products and sums round once each.
#pragma once
#include "pme_math.h"

namespace admp {

constexpr int kTcfMaxTypes = 8;

// s = d . box^-1: the fractional components of a Cartesian difference
ADMP_HD void tcf_fractional(const Box<double>& b, const double d[3], double s[3]) {
  s[0] = d[0] * b.hinv[0] + d[1] * b.hinv[3] + d[2] * b.hinv[6];
  s[1] = d[0] * b.hinv[1] + d[1] * b.hinv[4] + d[2] * b.hinv[7];
  s[2] = d[0] * b.hinv[2] + d[1] * b.hinv[5] + d[2] * b.hinv[8];
}
ADMP_HD bool tcf_large_jump(const double s[3]) { return m_abs(s[0]) >= 0.25 || m_abs(s[1]) >= 0.25 || m_abs(s[2]) >= 0.25; }

// acc += min_image(pos - last) in the cell b; returns whether the move was a large jump
ADMP_HD bool tcf_unwrap(const Box<double>& b, const double pos[3], const double last[3], double acc[3]) {
  const double d[3] = {pos[0] - last[0], pos[1] - last[1], pos[2] - last[2]};
  double s[3];
  tcf_fractional(b, d, s);
  s[0] -= m_floor(s[0] + 0.5);
  s[1] -= m_floor(s[1] + 0.5);
  s[2] -= m_floor(s[2] + 0.5);
  const bool jump = tcf_large_jump(s);
  acc[0] += s[0] * b.h[0] + s[1] * b.h[3] + s[2] * b.h[6];
  acc[1] += s[0] * b.h[1] + s[1] * b.h[4] + s[2] * b.h[7];
  acc[2] += s[0] * b.h[2] + s[1] * b.h[5] + s[2] * b.h[8];
  return jump;
}

// the accumulator as the ring holds it
template <class T>
ADMP_HD T tcf_ring_word(double d) { return (T)d; }

template <class T>
ADMP_HD double tcf_msd_term(T ax, T ay, T az, T bx, T by, T bz) {
  const double x = (double)ax - (double)bx, y = (double)ay - (double)by, z = (double)az - (double)bz;
  return x * x + y * y + z * z;
}
template <class T>
ADMP_HD double tcf_vacf_term(T ax, T ay, T az, T bx, T by, T bz) {
  return (double)ax * (double)bx + (double)ay * (double)by + (double)az * (double)bz;
}

}  // namespace admp
