// Host build of the matrix-core share of the inverse plane kernel (admp_amd/csrc/plane_mfma_plan.h: PlaneInvSplit,
// PlaneMfmaInvYPlan, PlaneMfmaInvZPlan): the split, the plans, the lane maps the kernel uses and one unit's sums in the
// matrix-core order; tests/test_plane_mfma_inv_plan_cpu.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../admp_amd/csrc/plane_mfma_plan.h"

using namespace admp;

namespace {
std::vector<Cx<double>> table(int N) {
  std::vector<Cx<double>> tw(N);
  for (int m = 0; m < N; ++m) tw[m] = Cx<double>{circ_cos(m, N), std::sin(2.0 * M_PI * (double)m / (double)N)};
  return tw;
}
}  // namespace

extern "C" {
// the lines of workgroup z as the VECTOR kernel lists them (k_dft_yz_inv's thread 0, copied here so that the plan is checked
// against the kernel's own text and not against itself); returns their number
int inv_lines_vector(int N2, int z, int nz, int KQ, int64_t* lines) {
  const int Kh2 = N2 / 2 + 1, TK2 = (Kh2 + KQ - 1) / KQ;
  const int g0 = (int)(((long)TK2 * z) / nz), g1 = (int)(((long)TK2 * (z + 1)) / nz);
  int n = 0;
  for (int g = g0; g < g1; ++g)
    for (int q = 0; q < KQ; ++q) {
      const int kq = g + q * TK2;
      if (kq >= Kh2) continue;
      lines[n++] = kq;
      if (kq != 0 && 2 * kq != N2) lines[n++] = N2 - kq;
    }
  return n;
}
// the same from the plan, in the order of the matrix units; out[10] = TK, g0, g1, kb0, kn0, kb1, kn1, own0, ownn, nlines
int inv_lines_plan(int N2, int z, int nz, int64_t* lines, int64_t* out) {
  const PlaneInvSplit s = plane_inv_split(N2, z, nz);
  out[0] = s.TK; out[1] = s.g0; out[2] = s.g1; out[3] = s.kb[0]; out[4] = s.kn[0]; out[5] = s.kb[1]; out[6] = s.kn[1];
  out[7] = s.own0; out[8] = s.ownn; out[9] = s.nlines;
  for (int t = 0; t < s.nlines; ++t) lines[t] = plane_inv_line(s, t);
  return s.nlines;
}
// out[8] = H, KP, T0, T1, MT, CT, nunits, Wm
void inv_y_plan(int N, int ncols, int z, int nz, int nwaves, int64_t* out) {
  const PlaneMfmaInvYPlan p = plane_mfma_inv_y_plan(N, ncols, z, nz, nwaves);
  out[0] = p.H; out[1] = p.KP; out[2] = p.T[0]; out[3] = p.T[1]; out[4] = p.MT; out[5] = p.CT; out[6] = p.nunits; out[7] = p.Wm;
}
// Walks workgroup z as the kernel does (dft_y_unit_rows with the tile's rows from the plan): cnt[(row * ncols + c) * 2 + comp]
// += 1 for every word of V that a unit writes.  pad[0] = operands fetched at padded positions or dead columns, pad[1] = how
// many of those plane_mfma_inv_y_operand_live lets through (must be 0), pad[2] = live operands, pad[3] = masked output rows.
void inv_y_cover(int N, int ncols, int z, int nz, int nwaves, int64_t* cnt, int64_t* pad) {
  const PlaneMfmaInvYPlan p = plane_mfma_inv_y_plan(N, ncols, z, nz, nwaves);
  pad[0] = pad[1] = pad[2] = pad[3] = 0;
  for (int wave = 0; wave < p.Wm; ++wave)
    for (int u = wave; u < p.nunits; u += p.Wm) {
      const int mt = u % p.MT, ct = u / p.MT;
      const int kb = plane_mfma_inv_y_kb(p, mt), ke = plane_mfma_inv_y_ke(p, mt);
      for (int lane = 0; lane < 64; ++lane) {
        const int c = plane_mfma_col(ct, lane), comp = plane_mfma_comp(lane), hi = plane_mfma_pos0(lane);
        for (int kk = hi; kk < p.KP; kk += 4) {
          const bool inside = kk < p.H && c < ncols;
          if (!inside) { ++pad[0]; if (plane_mfma_inv_y_operand_live(p, kk, c)) ++pad[1]; }
          else if (plane_mfma_inv_y_operand_live(p, kk, c)) ++pad[2];
        }
        for (int r = 0; r < 4; ++r) {
          const int k = kb + (lane >> 4) + 4 * r;
          if (k >= ke) { if (c == 8 * ct && comp == 0) ++pad[3]; continue; }
          if (c < ncols) { ++cnt[(k * ncols + c) * 2 + comp]; ++cnt[((N - k) * ncols + c) * 2 + comp]; }
        }
        if (mt == 0 && hi == 0 && c < ncols) {
          if (p.s.own0) ++cnt[c * 2 + comp];
          if (p.s.ownn) ++cnt[((N / 2) * ncols + c) * 2 + comp];
        }
      }
    }
}
// The lines x [N][ncols] (complex, interleaved), inverse direction: Xm = every unit of both workgroups' plans in the matrix-core
// order, Xv = dft_pair_core<+1> in double per output pair; both [N][ncols].  Sm, Sv [N/2+1][ncols][4]: the four sums of the
// outputs k = 1..H.  sabs[c] = the sum over the column's pair positions of its largest |operand word| per position.
// Returns the number of units of the two workgroups.
int inv_y_lines(int N, int ncols, int nwaves, const double* x, double* Xm, double* Xv, double* Sm, double* Sv, double* sabs) {
  const int H = (N - 1) / 2;
  std::vector<Cx<double>> Z((size_t)N * ncols);
  const std::vector<Cx<double>> tw = table(N);
  const Cx<double>* xin = reinterpret_cast<const Cx<double>*>(x);
  for (int c = 0; c < ncols; ++c) {
    Z[c] = xin[c];
    if ((N & 1) == 0) Z[(N / 2) * ncols + c] = xin[(N / 2) * ncols + c];
    sabs[c] = 0.0;
    for (int j = 1; j <= H; ++j) {
      const Cx<double> a = xin[j * ncols + c], b = xin[(N - j) * ncols + c];
      Z[j * ncols + c] = Cx<double>{a.re + b.re, a.im + b.im};
      Z[(N - j) * ncols + c] = Cx<double>{a.re - b.re, a.im - b.im};
      sabs[c] += std::fmax(std::fmax(std::fabs(a.re + b.re), std::fabs(a.im + b.im)), std::fmax(std::fabs(a.re - b.re), std::fabs(a.im - b.im)));
    }
  }
  int nu = 0;
  for (int z = 0; z < 2; ++z) {
    const PlaneMfmaInvYPlan p = plane_mfma_inv_y_plan(N, ncols, z, 2, nwaves);
    for (int u = 0; u < p.nunits; ++u) plane_mfma_inv_y_unit_host<double>(p, u, Z.data(), tw.data(), reinterpret_cast<Cx<double>*>(Xm), Sm);
    nu += p.nunits;
  }
  Cx<double>* V = reinterpret_cast<Cx<double>*>(Xv);
  for (int c = 0; c < ncols; ++c)
    for (int k = 0; k <= N / 2; ++k) {
      Cx<double> Xk, Xnk;
      dft_pair_outputs_rows<double, +1, 1>(N, &k, ncols, Z.data() + c, tw.data(), &Xk, &Xnk);
      V[k * ncols + c] = Xk;
      if (k != 0 && 2 * k != N) V[(N - k) * ncols + c] = Xnk;
      if (k >= 1 && k <= H) {
        const Cx<double>* col = Z.data() + c;
        double* s = Sv + (size_t)(k * ncols + c) * 4;
        s[0] = s[1] = s[2] = s[3] = 0.0;
        dft_pair_partial<double, 1>(N, &k, [=](int j) {
          const Cx<double> a = col[(1 + j) * ncols], b = col[(N - 1 - j) * ncols];
          return PairCx<double>{a.re, a.im, b.re, b.im};
        }, tw.data(), 0, H, s, s + 1, s + 2, s + 3);
      }
    }
  return nu;
}

// ---- inverse z lines
// out[6] = H, KP, JT, LT, nunits, Wm
void inv_z_plan(int N, int nlines, int nwaves, int64_t* out) {
  const PlaneMfmaInvZPlan p = plane_mfma_inv_z_plan(N, nlines, nwaves);
  out[0] = p.H; out[1] = p.KP; out[2] = p.JT; out[3] = p.LT; out[4] = p.nunits; out[5] = p.Wm;
}
// cnt[li * N + j] += 1 for every word of line li (index into the workgroup's list) that a unit stores, walking waves, units,
// lanes and accumulator words as the kernel does; pad[0] = operands at padded positions or dead lines, pad[1] = those that
// plane_mfma_inv_z_operand_live lets through
void inv_z_cover(int N, int nlines, int nwaves, int64_t* cnt, int64_t* pad) {
  const PlaneMfmaInvZPlan p = plane_mfma_inv_z_plan(N, nlines, nwaves);
  pad[0] = pad[1] = 0;
  for (int wave = 0; wave < p.Wm; ++wave)
    for (int u = wave; u < p.nunits; u += p.Wm) {
      const int jt = u % p.JT, lt = u / p.JT;
      for (int lane = 0; lane < 64; ++lane) {
        const int li = plane_mfma_inv_z_op_line(lt, lane), j = plane_mfma_inv_z_tw_j(jt, lane), hi = lane >> 4;
        for (int kk = hi; kk < p.KP; kk += 4)
          if (!(kk < p.H && li < nlines)) { ++pad[0]; if (plane_mfma_inv_z_operand_live(p, kk, li)) ++pad[1]; }
        for (int r = 0; r < 4; ++r) {
          const int lo = plane_mfma_inv_z_out_line(lt, lane, r);
          if (lo < nlines && j <= p.H) { ++cnt[lo * N + j]; ++cnt[lo * N + N - j]; }
        }
        if (jt == 0 && hi == 0 && li < nlines) {
          ++cnt[li * N];
          if ((N & 1) == 0) ++cnt[li * N + N / 2];
        }
      }
    }
}
// half spectra V [nlines][N/2+1] (complex): xm = every unit in the matrix-core order, xv = irdft_pair_outputs in double, both
// [nlines][N]; Sm, Sv [nlines][H+1][2] = (P, R) of j = 1..H; sabs[l] = sum over k = 1..H of max(|re|, |im|) of V[l][k]
int inv_z_lines(int N, int nlines, int nwaves, const double* V, double* xm, double* xv, double* Sm, double* Sv, double* sabs) {
  const PlaneMfmaInvZPlan p = plane_mfma_inv_z_plan(N, nlines, nwaves);
  const int H = p.H, Kh = N / 2 + 1;
  const std::vector<Cx<double>> tw = table(N);
  const Cx<double>* v = reinterpret_cast<const Cx<double>*>(V);
  for (int u = 0; u < p.nunits; ++u) plane_mfma_inv_z_unit_host<double>(p, u, v, tw.data(), xm, Sm);
  for (int l = 0; l < nlines; ++l) {
    const Cx<double>* vl = v + (size_t)l * Kh;
    sabs[l] = 0.0;
    for (int k = 1; k <= H; ++k) sabs[l] += std::fmax(std::fabs(vl[k].re), std::fabs(vl[k].im));
    for (int j = 0; j <= N / 2; ++j) {
      double a, b;
      irdft_pair_outputs<double, 1>(N, &j, 1, vl + 1, vl[0].re, (N & 1) ? 0.0 : vl[N / 2].re, tw.data(), &a, &b);
      xv[(size_t)l * N + j] = a;
      if (j != 0 && 2 * j != N) xv[(size_t)l * N + N - j] = b;
      if (j >= 1 && j <= H) real_pair_sums<double, 1>(N, &j, 1, vl + 1, tw.data(), Sv + ((size_t)l * (H + 1) + j) * 2, Sv + ((size_t)l * (H + 1) + j) * 2 + 1);
    }
  }
  return p.nunits;
}
}
