// The matrix-core share of a line phase of the plane kernels (dft_kernels.hip k_dft_zy_fwd<double, 2, SPREAD, true> and, further
// down, k_dft_yz_inv<double, 2, true>): which
// (16-output tile, 8-column tile) units go to the matrix waves, which waves take them and which columns stay with the vector
// tasks.  Host arithmetic with no device-only construct (the kernel calls the same functions), next to dft_plan.h so that the
// host-compiled test shims can call it (tests/test_plane_mfma_plan_cpu.py, tests/test_plane_mfma_inv_plan_cpu.py).
//
// A pair-symmetric line transform (dft_math.h) is two real products, P = C a and R = S b, with the H x H matrices
// C[k][j] = cos(2 pi k j / N), S[k][j] = sin(2 pi k j / N), k, j = 1..H, H = (N - 1) / 2.  A unit is one 16 x 16 tile of both:
// 16 outputs k = 1 + 16 mt + i against the real and the imaginary parts of 8 complex columns c = 8 ct + (j & 7), summed over
// the pair positions in steps of 4 (v_mfma_f64_16x16x4_f64, operand maps in mfma.h).  Outputs beyond H and columns beyond the
// workgroup's are masked; positions are padded to a multiple of 4 with zero operands.  k = 0 and (N even) k = N / 2 are plain
// and alternating column sums: the units of the first output tile form them from the operands they fetch anyway.
// The forward z lines have a share of their own (PlaneMfmaZPlan below).
// Measured at 97^3 f64 (tools/ubench/plane_hybrid.hip, profiles/README.md r10a): the y lines of the forward kernel take 7.2 us
// in the vector form, 6.7 / 6.5 / 5.6 us with 1 / 2 / 3 column tiles as matrix units and 5.1 us with all four -- a vector wave
// takes as long for its 48 steps whether one or three share its SIMD, so the share that pays is every column.
#pragma once
#include "dft_math.h"

namespace admp {

struct PlaneMfmaPlan {
  int N, H, KP;        // line length, pair positions, positions padded to a multiple of 4
  int ncols;           // data columns of the workgroup
  int MT, CT;          // 16-output tiles of k = 1..H (the last one masked beyond H), 8-column tiles of the share
  int nm;              // columns [0, nm) are produced by the matrix units, [nm, ncols) by the vector tasks (every k)
  int nunits, Wm;      // unit u = mt + MT * ct; waves [0, Wm) walk u = wave, wave + Wm, ...; the other waves run the tasks
};
// y lines of a workgroup with ncols columns and nwaves wavefronts.  The share is cut by column tiles (an output tile cut off
// would leave a vector task per column anyway); H < 16 has no whole tile row: no share.
ADMP_HD PlaneMfmaPlan plane_mfma_y_plan(int N, int ncols, int nwaves) {
  PlaneMfmaPlan p;
  p.N = N; p.H = (N - 1) / 2; p.KP = (p.H + 3) & ~3;
  p.ncols = ncols;
  p.MT = (p.H + 15) / 16;
  p.CT = p.H < 16 ? 0 : (ncols + 7) / 8;
  p.nm = 8 * p.CT < ncols ? 8 * p.CT : ncols;
  p.nunits = p.MT * p.CT;
  p.Wm = p.nunits < nwaves ? p.nunits : nwaves;      // (the share is every column or none: no vector wave has to be kept)
  return p;
}
// what lane (0..63) of a unit holds: its twiddle row, its data column and component, its first pair position, and the
// output of accumulator word r (0..3)
ADMP_HD int plane_mfma_tw_row(int mt, int lane) { return 16 * mt + (lane & 15); }          // output k - 1 of the twiddle operand
ADMP_HD int plane_mfma_col(int ct, int lane) { return 8 * ct + (lane & 7); }
ADMP_HD int plane_mfma_comp(int lane) { return (lane >> 3) & 1; }                           // 0: real parts, 1: imaginary parts
ADMP_HD int plane_mfma_pos0(int lane) { return lane >> 4; }                                 // positions pos0, pos0 + 4, ...
ADMP_HD int plane_mfma_out_k(int mt, int lane, int r) { return 1 + 16 * mt + (lane >> 4) + 4 * r; }
ADMP_HD bool plane_mfma_operand_live(const PlaneMfmaPlan& p, int kk, int c) { return kk < p.H && c < p.ncols; }

// One unit on the host, in the order the matrix cores sum it (a step adds the products of 4 positions to the accumulator;
// within a step the order is the hardware's, taken here as ascending): Z = the workgroup's [N][ncols] lines with the rows
// paired in place (row j: x_j + x_{N-j}, row N - j: x_j - x_{N-j}), tw[m] = (cos, sin)(2 pi m / N) exact; writes the unit's
// outputs into X [N][ncols] and, where sums is not null, the four sums of output k and column c (P of the real and the
// imaginary parts, then R of both: Are, Aim, Bre, Bim of dft_pair_partial) into sums[(k * ncols + c) * 4 ..].
template <class T, int SIGN>
inline void plane_mfma_unit_host(const PlaneMfmaPlan& p, int u, const Cx<T>* Z, const Cx<T>* tw, Cx<T>* X, T* sums) {
  const int N = p.N, H = p.H, mt = u % p.MT, ct = u / p.MT;
  for (int c = 8 * ct; c < 8 * ct + 8 && c < p.ncols; ++c) {
    const Cx<T> x0 = Z[c], xn = (N & 1) ? Cx<T>{T(0), T(0)} : Z[(N / 2) * p.ncols + c];
    for (int i = 0; i < 16; ++i) {
      const int k = 1 + 16 * mt + i;
      if (k > H) continue;
      T P[2] = {T(0), T(0)}, R[2] = {T(0), T(0)};
      for (int kk = 0; kk < p.KP; ++kk) {
        const bool live = plane_mfma_operand_live(p, kk, c);
        const int m = (int)(((long)k * (1 + kk)) % N);
        const Cx<T> a = live ? Z[(1 + kk) * p.ncols + c] : Cx<T>{T(0), T(0)};
        const Cx<T> b = live ? Z[(N - 1 - kk) * p.ncols + c] : Cx<T>{T(0), T(0)};
        P[0] += tw[m].re * a.re; P[1] += tw[m].re * a.im;
        R[0] += tw[m].im * b.re; R[1] += tw[m].im * b.im;
      }
      T bre = x0.re + P[0], bim = x0.im + P[1];
      if ((N & 1) == 0) { bre += (k & 1) ? -xn.re : xn.re; bim += (k & 1) ? -xn.im : xn.im; }
      X[k * p.ncols + c] = Cx<T>{bre - T(SIGN) * R[1], bim + T(SIGN) * R[0]};
      X[(N - k) * p.ncols + c] = Cx<T>{bre + T(SIGN) * R[1], bim - T(SIGN) * R[0]};
      if (sums) { T* s = sums + (size_t)(k * p.ncols + c) * 4; s[0] = P[0]; s[1] = P[1]; s[2] = R[0]; s[3] = R[1]; }
    }
    if (mt == 0) {          // the column sums: four partial sums by position mod 4, as the four lane groups hold them
      T s[4][2] = {{T(0), T(0)}, {T(0), T(0)}, {T(0), T(0)}, {T(0), T(0)}};
      for (int kk = 0; kk < H; ++kk) { s[kk & 3][0] += Z[(1 + kk) * p.ncols + c].re; s[kk & 3][1] += Z[(1 + kk) * p.ncols + c].im; }
      X[c] = Cx<T>{x0.re + ((s[0][0] + s[1][0]) + (s[2][0] + s[3][0])) + xn.re, x0.im + ((s[0][1] + s[1][1]) + (s[2][1] + s[3][1])) + xn.im};
      if ((N & 1) == 0) {   // k = N/2: (-1)^j on position j = 1 + kk
        const T sg = ((N / 2) & 1) ? T(-1) : T(1);
        X[(N / 2) * p.ncols + c] = Cx<T>{x0.re + ((s[1][0] - s[0][0]) + (s[3][0] - s[2][0])) + sg * xn.re,
                                         x0.im + ((s[1][1] - s[0][1]) + (s[3][1] - s[2][1])) + sg * xn.im};
      }
    }
  }
}

// ---- z lines of the forward kernel: real lines l = 0 .. nlines-1, the workgroup's outputs k = k0 .. k0 + nout - 1 of 0 .. N/2.
// X[l][k] = x_0 + P - i R with P = sum_j cos(2 pi k j / N) (x_j + x_{N-j}), R = sum_j sin(2 pi k j / N) (x_j - x_{N-j}): a unit is
// 16 outputs against 16 lines, both sums in the same lane.  k = 0 and k = N / 2 are tile rows like any other (cos = 1 or
// (-1)^j, sin = 0 from the table); x_{N/2} of even N is added where rdft_outputs adds it.  The share is cut by whole units
// (every line and output or none): an output tile or a line tile left to the vector tasks would cost them a full round.
struct PlaneMfmaZPlan {
  int N, H, KP;        // line length, pair positions, positions padded to a multiple of 4
  int nlines, k0, nout;
  int MT, LT;          // 16-output tiles of k0 .. k0 + nout - 1 (the last one masked), 16-line tiles (the last one masked)
  int nunits, Wm;      // unit u = mt + MT * lt; waves [0, Wm) walk u = wave, wave + Wm, ...
};
ADMP_HD PlaneMfmaZPlan plane_mfma_z_plan(int N, int k0, int nout, int nlines, int nwaves) {
  PlaneMfmaZPlan p;
  p.N = N; p.H = (N - 1) / 2; p.KP = (p.H + 3) & ~3;
  p.nlines = nlines; p.k0 = k0; p.nout = nout;
  p.MT = p.H < 16 ? 0 : (nout + 15) / 16;
  p.LT = (nlines + 15) / 16;
  p.nunits = p.MT * p.LT;
  p.Wm = p.nunits < nwaves ? p.nunits : nwaves;
  return p;
}
ADMP_HD int plane_mfma_z_tw_k(const PlaneMfmaZPlan& p, int mt, int lane) { return p.k0 + 16 * mt + (lane & 15); }      // output of the twiddle operand
ADMP_HD int plane_mfma_z_line(int lt, int lane) { return 16 * lt + (lane & 15); }
ADMP_HD int plane_mfma_z_out_k(const PlaneMfmaZPlan& p, int mt, int lane, int r) { return p.k0 + 16 * mt + (lane >> 4) + 4 * r; }
ADMP_HD bool plane_mfma_z_operand_live(const PlaneMfmaZPlan& p, int kk, int l) { return kk < p.H && l < p.nlines; }

// One unit on the host in the matrix-core order: ps = the pair sums [H][nlines] ((x_j + x_{N-j}, x_j - x_{N-j}) of position
// j = 1 + jj), x0, xn [nlines]; writes X[l * nout + k - k0] and, where sums is not null, (P, R) into sums[(l * nout + k - k0) * 2 ..].
template <class T>
inline void plane_mfma_z_unit_host(const PlaneMfmaZPlan& p, int u, const Cx<T>* ps, const T* x0, const T* xn, const Cx<T>* tw,
                                   Cx<T>* X, T* sums) {
  const int N = p.N, mt = u % p.MT, lt = u / p.MT;
  for (int l = 16 * lt; l < 16 * lt + 16 && l < p.nlines; ++l)
    for (int k = p.k0 + 16 * mt; k < p.k0 + 16 * mt + 16 && k < p.k0 + p.nout; ++k) {
      T P = T(0), R = T(0);
      for (int kk = 0; kk < p.KP; ++kk) {
        const int m = (int)(((long)k * (1 + kk)) % N);
        const Cx<T> v = plane_mfma_z_operand_live(p, kk, l) ? ps[kk * p.nlines + l] : Cx<T>{T(0), T(0)};
        P += tw[m].re * v.re;
        R += tw[m].im * v.im;
      }
      T re = x0[l] + P;
      if ((N & 1) == 0) re += (k & 1) ? -xn[l] : xn[l];
      X[l * p.nout + k - p.k0] = Cx<T>{re, -R};
      if (sums) { sums[(size_t)(l * p.nout + k - p.k0) * 2] = P; sums[(size_t)(l * p.nout + k - p.k0) * 2 + 1] = R; }
    }
}

// ---- the inverse kernel (k_dft_yz_inv<double, 2, true>).  gridDim.z workgroups split a plane by groups of its y output pairs:
// workgroup z owns the groups g0 <= g < g1 of TK = ceil((N/2 + 1) / 2), that is the outputs kq = g (range 0) and kq = g + TK
// (range 1) with their partners N - kq.  PlaneInvSplit is that split, exactly as the vector kernel computes it.
// Measured at 97^3 f64 (profiles/README.md r11a): y lines 7.7 -> 6.9 us, z lines + stores 8.2 -> 5.0 us, the launch 21.7 -> 18.2 us.
struct PlaneInvSplit {
  int N, Kh2, TK, g0, g1;
  int kb[2], kn[2];    // the pair outputs 1 <= k <= H of the two ranges: k = kb[r] .. kb[r] + kn[r] - 1
  int own0, ownn;      // X[0] / X[N/2] (N even) are this workgroup's
  int nlines;          // lines it produces: both members of its pairs, 0 and N/2 once
};
ADMP_HD PlaneInvSplit plane_inv_split(int N, int z, int nz) {
  PlaneInvSplit s;
  const int H = (N - 1) / 2;
  s.N = N; s.Kh2 = N / 2 + 1; s.TK = (s.Kh2 + 1) / 2;
  s.g0 = (int)(((long)s.TK * z) / nz); s.g1 = (int)(((long)s.TK * (z + 1)) / nz);
  for (int r = 0; r < 2; ++r) {
    int b = s.g0 + r * s.TK, e = s.g1 + r * s.TK;
    if (b < 1) b = 1;
    if (e > H + 1) e = H + 1;
    s.kb[r] = b; s.kn[r] = e > b ? e - b : 0;
  }
  s.own0 = s.g0 == 0 && s.g1 > 0;
  const int gn = N / 2 - s.TK;                      // the group whose second output is N/2
  s.ownn = (N & 1) == 0 && ((N / 2 >= s.g0 && N / 2 < s.g1) || (gn >= s.g0 && gn < s.g1));
  s.nlines = 2 * (s.kn[0] + s.kn[1]) + s.own0 + s.ownn;
  return s;
}
// The lines in the order the matrix units take them (the z phase reads 16 lines of a tile at once: neighbours in the list are
// neighbouring rows of V, which fall into different LDS banks): the ranges ascending, then their partners, then 0 and N/2.
ADMP_HD int plane_inv_line(const PlaneInvSplit& s, int idx) {
  if (idx < s.kn[0]) return s.kb[0] + idx;
  idx -= s.kn[0];
  if (idx < s.kn[1]) return s.kb[1] + idx;
  idx -= s.kn[1];
  if (idx < s.kn[0]) return s.N - (s.kb[0] + idx);
  idx -= s.kn[0];
  if (idx < s.kn[1]) return s.N - (s.kb[1] + idx);
  idx -= s.kn[1];
  if (idx == 0 && s.own0) return 0;
  return s.N / 2;
}

// Inverse y lines, every column of the plane: a unit is 16 pair outputs of ONE range (tile mt < T[0]: range 0) against 8 complex
// columns, summed like the forward unit; the rows beyond the range's end are masked.  The units of the first tile form the
// column sums X[0], X[N/2] where they are the workgroup's.
struct PlaneMfmaInvYPlan {
  int N, H, KP, ncols;
  PlaneInvSplit s;
  int T[2], MT, CT;    // 16-output tiles of the two ranges, 8-column tiles
  int nunits, Wm;      // unit u = mt + MT * ct; waves [0, Wm) walk u = wave, wave + Wm, ...
};
ADMP_HD PlaneMfmaInvYPlan plane_mfma_inv_y_plan(int N, int ncols, int z, int nz, int nwaves) {
  PlaneMfmaInvYPlan p;
  p.N = N; p.H = (N - 1) / 2; p.KP = (p.H + 3) & ~3;
  p.ncols = ncols;
  p.s = plane_inv_split(N, z, nz);
  const bool share = p.H >= 16;
  p.T[0] = share ? (p.s.kn[0] + 15) / 16 : 0;
  p.T[1] = share ? (p.s.kn[1] + 15) / 16 : 0;
  p.MT = p.T[0] + p.T[1];
  p.CT = p.MT > 0 ? (ncols + 7) / 8 : 0;
  p.nunits = p.MT * p.CT;
  p.Wm = p.nunits < nwaves ? p.nunits : nwaves;
  return p;
}
// first output k of tile mt and one past its last
ADMP_HD int plane_mfma_inv_y_kb(const PlaneMfmaInvYPlan& p, int mt) {
  return mt < p.T[0] ? p.s.kb[0] + 16 * mt : p.s.kb[1] + 16 * (mt - p.T[0]);
}
ADMP_HD int plane_mfma_inv_y_ke(const PlaneMfmaInvYPlan& p, int mt) {
  const int r = mt < p.T[0] ? 0 : 1, e = p.s.kb[r] + p.s.kn[r], t = plane_mfma_inv_y_kb(p, mt) + 16;
  return t < e ? t : e;
}
// the lane maps are the forward unit's (plane_mfma_col, _comp, _pos0) with the tile's rows from the plan: twiddle row
// k = kb + (lane & 15), accumulator word r = output k = kb + (lane >> 4) + 4 r, both masked at ke
ADMP_HD bool plane_mfma_inv_y_operand_live(const PlaneMfmaInvYPlan& p, int kk, int c) { return kk < p.H && c < p.ncols; }
// One unit on the host in the matrix-core order; Z, tw, X, sums as for plane_mfma_unit_host (SIGN = +1)
template <class T>
inline void plane_mfma_inv_y_unit_host(const PlaneMfmaInvYPlan& p, int u, const Cx<T>* Z, const Cx<T>* tw, Cx<T>* X, T* sums) {
  const int N = p.N, H = p.H, mt = u % p.MT, ct = u / p.MT;
  const int kb = plane_mfma_inv_y_kb(p, mt), ke = plane_mfma_inv_y_ke(p, mt);
  for (int c = 8 * ct; c < 8 * ct + 8 && c < p.ncols; ++c) {
    const Cx<T> x0 = Z[c], xn = (N & 1) ? Cx<T>{T(0), T(0)} : Z[(N / 2) * p.ncols + c];
    for (int k = kb; k < ke; ++k) {
      T P[2] = {T(0), T(0)}, R[2] = {T(0), T(0)};
      for (int kk = 0; kk < p.KP; ++kk) {
        const bool live = plane_mfma_inv_y_operand_live(p, kk, c);
        const int m = (int)(((long)k * (1 + kk)) % N);
        const Cx<T> a = live ? Z[(1 + kk) * p.ncols + c] : Cx<T>{T(0), T(0)};
        const Cx<T> b = live ? Z[(N - 1 - kk) * p.ncols + c] : Cx<T>{T(0), T(0)};
        P[0] += tw[m].re * a.re; P[1] += tw[m].re * a.im;
        R[0] += tw[m].im * b.re; R[1] += tw[m].im * b.im;
      }
      T bre = x0.re + P[0], bim = x0.im + P[1];
      if ((N & 1) == 0) { bre += (k & 1) ? -xn.re : xn.re; bim += (k & 1) ? -xn.im : xn.im; }
      X[k * p.ncols + c] = Cx<T>{bre - R[1], bim + R[0]};
      X[(N - k) * p.ncols + c] = Cx<T>{bre + R[1], bim - R[0]};
      if (sums) { T* s = sums + (size_t)(k * p.ncols + c) * 4; s[0] = P[0]; s[1] = P[1]; s[2] = R[0]; s[3] = R[1]; }
    }
    if (mt == 0 && (p.s.own0 || p.s.ownn)) {      // the column sums: four partial sums by position mod 4
      T s[4][2] = {{T(0), T(0)}, {T(0), T(0)}, {T(0), T(0)}, {T(0), T(0)}};
      for (int kk = 0; kk < H; ++kk) { s[kk & 3][0] += Z[(1 + kk) * p.ncols + c].re; s[kk & 3][1] += Z[(1 + kk) * p.ncols + c].im; }
      if (p.s.own0)
        X[c] = Cx<T>{x0.re + ((s[0][0] + s[1][0]) + (s[2][0] + s[3][0])) + xn.re, x0.im + ((s[0][1] + s[1][1]) + (s[2][1] + s[3][1])) + xn.im};
      if (p.s.ownn) {
        const T sg = ((N / 2) & 1) ? T(-1) : T(1);
        X[(N / 2) * p.ncols + c] = Cx<T>{x0.re + ((s[1][0] - s[0][0]) + (s[3][0] - s[2][0])) + sg * xn.re,
                                         x0.im + ((s[1][1] - s[0][1]) + (s[3][1] - s[2][1])) + sg * xn.im};
      }
    }
  }
}

// Inverse z lines (c2r) of the workgroup's nlines lines (plane_inv_line order): x_j = X0.re + 2 (P - R), x_{N-j} = X0.re + 2 (P + R),
// P = sum_k cos(2 pi j k / N) X_k.re, R = sum_k sin(2 pi j k / N) X_k.im (+ (-1)^j X[N/2].re, N even).  A unit is 16 lines against
// 16 outputs j = 1 + 16 jt + i <= H with the operand roles swapped against the forward unit -- the data operand is
// A[line][position], the twiddle operand B[position][j] -- so that an accumulator column is one j and a store instruction
// writes runs of 16 neighbouring words of 4 lines.  j = 0 and j = N/2 are column sums of the units of the first output tile.
struct PlaneMfmaInvZPlan {
  int N, H, KP, nlines;
  int JT, LT;          // 16-output tiles of j = 1..H (the last one masked), 16-line tiles (the last one masked)
  int nunits, Wm;      // unit u = jt + JT * lt
};
ADMP_HD PlaneMfmaInvZPlan plane_mfma_inv_z_plan(int N, int nlines, int nwaves) {
  PlaneMfmaInvZPlan p;
  p.N = N; p.H = (N - 1) / 2; p.KP = (p.H + 3) & ~3;
  p.nlines = nlines;
  p.JT = p.H < 16 ? 0 : (p.H + 15) / 16;
  p.LT = (nlines + 15) / 16;
  p.nunits = p.JT * p.LT;
  p.Wm = p.nunits < nwaves ? p.nunits : nwaves;
  return p;
}
ADMP_HD int plane_mfma_inv_z_op_line(int lt, int lane) { return 16 * lt + (lane & 15); }                // list index of the data operand
ADMP_HD int plane_mfma_inv_z_tw_j(int jt, int lane) { return 1 + 16 * jt + (lane & 15); }               // output of the twiddle operand
ADMP_HD int plane_mfma_inv_z_out_line(int lt, int lane, int r) { return 16 * lt + (lane >> 4) + 4 * r; }  // accumulator word r
ADMP_HD bool plane_mfma_inv_z_operand_live(const PlaneMfmaInvZPlan& p, int kk, int li) { return kk < p.H && li < p.nlines; }
// One unit on the host in the matrix-core order: V = the half spectra [nlines][Kh] of the listed lines (Kh = N/2 + 1); writes
// x [nlines][N] and, where sums is not null, (P, R) of output j = 1..H into sums[(li * (H + 1) + j) * 2 ..].
template <class T>
inline void plane_mfma_inv_z_unit_host(const PlaneMfmaInvZPlan& p, int u, const Cx<T>* V, const Cx<T>* tw, T* x, T* sums) {
  const int N = p.N, H = p.H, Kh = N / 2 + 1, jt = u % p.JT, lt = u / p.JT;
  for (int li = 16 * lt; li < 16 * lt + 16 && li < p.nlines; ++li) {
    const Cx<T>* v = V + (size_t)li * Kh;
    const T X0 = v[0].re, Xn = (N & 1) ? T(0) : v[N / 2].re;
    for (int j = 1 + 16 * jt; j < 17 + 16 * jt && j <= H; ++j) {
      T P = T(0), R = T(0);
      for (int kk = 0; kk < p.KP; ++kk) {
        const int m = (int)(((long)j * (1 + kk)) % N);
        const Cx<T> a = plane_mfma_inv_z_operand_live(p, kk, li) ? v[1 + kk] : Cx<T>{T(0), T(0)};
        P += a.re * tw[m].re;
        R += a.im * tw[m].im;
      }
      T base = X0 + T(2) * P;
      if ((N & 1) == 0) base += (j & 1) ? -Xn : Xn;
      x[(size_t)li * N + j] = base - T(2) * R;
      x[(size_t)li * N + N - j] = base + T(2) * R;
      if (sums) { sums[((size_t)li * (H + 1) + j) * 2] = P; sums[((size_t)li * (H + 1) + j) * 2 + 1] = R; }
    }
    if (jt == 0) {
      T s[4] = {T(0), T(0), T(0), T(0)};
      for (int kk = 0; kk < H; ++kk) s[kk & 3] += v[1 + kk].re;
      x[(size_t)li * N] = X0 + T(2) * ((s[0] + s[1]) + (s[2] + s[3])) + Xn;
      if ((N & 1) == 0) x[(size_t)li * N + N / 2] = X0 + T(2) * ((s[1] - s[0]) + (s[3] - s[2])) + (((N / 2) & 1) ? -Xn : Xn);
    }
  }
}

}  // namespace admp
