// Host build of the matrix-core share of the plane kernels' y lines (admp_amd/csrc/plane_mfma_plan.h): the plan, the lane
// maps the kernel uses and one unit's sums in the matrix-core order; tests/test_plane_mfma_plan_cpu.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../admp_amd/csrc/plane_mfma_plan.h"

using namespace admp;

extern "C" {
// out[9] = N, H, KP, ncols, MT, CT, nm, nunits, Wm
void plane_y_plan(int N, int ncols, int nwaves, int64_t* out) {
  const PlaneMfmaPlan p = plane_mfma_y_plan(N, ncols, nwaves);
  out[0] = p.N; out[1] = p.H; out[2] = p.KP; out[3] = p.ncols; out[4] = p.MT; out[5] = p.CT; out[6] = p.nm; out[7] = p.nunits;
  out[8] = p.Wm;
}
// Walks the workgroup as the kernel does: waves [0, Wm) over their units, lane by lane and accumulator word by word, then
// the vector tasks of the other waves (KQ output pairs per task).  cnt[(k * ncols + c) * 2 + comp] += 1 for every word of
// X[k] (k = 0 .. N/2; X[N-k] is written with it) that is produced, mat[...] += 1 where a matrix unit produced it.
// pad[0] = operands fetched at padded positions or dead columns, pad[1] = how many of those plane_mfma_operand_live lets
// through (must be 0), pad[2] = live operands, pad[3] = masked output rows (k > H) over all units.
void plane_y_cover(int N, int ncols, int nwaves, int KQ, int64_t* cnt, int64_t* mat, int64_t* pad) {
  const PlaneMfmaPlan p = plane_mfma_y_plan(N, ncols, nwaves);
  pad[0] = pad[1] = pad[2] = pad[3] = 0;
  for (int wave = 0; wave < p.Wm; ++wave)
    for (int u = wave; u < p.nunits; u += p.Wm) {
      const int mt = u % p.MT, ct = u / p.MT;
      for (int lane = 0; lane < 64; ++lane) {
        const int c = plane_mfma_col(ct, lane), comp = plane_mfma_comp(lane), hi = plane_mfma_pos0(lane);
        for (int kk = hi; kk < p.KP; kk += 4) {
          const bool inside = kk < p.H && c < ncols;
          if (!inside) { ++pad[0]; if (plane_mfma_operand_live(p, kk, c)) ++pad[1]; }
          else if (plane_mfma_operand_live(p, kk, c)) ++pad[2];
        }
        for (int r = 0; r < 4; ++r) {
          const int k = plane_mfma_out_k(mt, lane, r);
          if (k > p.H) { if (c == 8 * ct && comp == 0) ++pad[3]; continue; }
          if (c < ncols) { ++cnt[(k * ncols + c) * 2 + comp]; ++mat[(k * ncols + c) * 2 + comp]; }
        }
        if (mt == 0 && hi == 0 && c < ncols) {
          ++cnt[c * 2 + comp]; ++mat[c * 2 + comp];
          if ((N & 1) == 0) { ++cnt[((N / 2) * ncols + c) * 2 + comp]; ++mat[((N / 2) * ncols + c) * 2 + comp]; }
        }
      }
    }
  const int Kh = N / 2 + 1, TK = (Kh + KQ - 1) / KQ, nv = ncols - p.nm, nthr = 64 * (nwaves - p.Wm);
  for (int t0 = 0; t0 < nthr; ++t0)
    for (int task = t0; task < TK * nv; task += nthr) {
      const int g = task / nv, c = p.nm + task - g * nv;
      for (int q = 0; q < KQ; ++q)
        if (g + q * TK < Kh) { ++cnt[((g + q * TK) * ncols + c) * 2]; ++cnt[((g + q * TK) * ncols + c) * 2 + 1]; }
    }
}
// The lines x [N][ncols] (complex, interleaved), direction sign: Xm = every unit of the plan in the matrix-core order
// (plane_mfma_unit_host), Xv = dft_pair_core in double per output pair; both [N][ncols].  Sm, Sv [N/2+1][ncols][4]: the four
// sums (Are, Aim, Bre, Bim) of the outputs k = 1..H in the two forms.  big[c] = the largest |word| of the paired column c (the
// largest term of its sums).  Returns the number of units.
int plane_y_lines(int N, int ncols, int nwaves, int sign, const double* x, double* Xm, double* Xv, double* Sm, double* Sv,
                  double* big) {
  const PlaneMfmaPlan p = plane_mfma_y_plan(N, ncols, nwaves);
  std::vector<Cx<double>> Z((size_t)N * ncols), tw(N);
  for (int m = 0; m < N; ++m) tw[m] = Cx<double>{circ_cos(m, N), std::sin(2.0 * M_PI * (double)m / (double)N)};
  const Cx<double>* xin = reinterpret_cast<const Cx<double>*>(x);
  for (int c = 0; c < ncols; ++c) {
    Z[c] = xin[c];
    if ((N & 1) == 0) Z[(N / 2) * ncols + c] = xin[(N / 2) * ncols + c];
    for (int j = 1; j <= p.H; ++j) {
      const Cx<double> a = xin[j * ncols + c], b = xin[(N - j) * ncols + c];
      Z[j * ncols + c] = Cx<double>{a.re + b.re, a.im + b.im};
      Z[(N - j) * ncols + c] = Cx<double>{a.re - b.re, a.im - b.im};
    }
    big[c] = 0.0;
    for (int j = 0; j < N; ++j) big[c] = std::fmax(big[c], std::fmax(std::fabs(Z[j * ncols + c].re), std::fabs(Z[j * ncols + c].im)));
  }
  Cx<double>* M = reinterpret_cast<Cx<double>*>(Xm);
  Cx<double>* V = reinterpret_cast<Cx<double>*>(Xv);
  for (int u = 0; u < p.nunits; ++u) {
    if (sign < 0) plane_mfma_unit_host<double, -1>(p, u, Z.data(), tw.data(), M, Sm);
    else plane_mfma_unit_host<double, +1>(p, u, Z.data(), tw.data(), M, Sm);
  }
  for (int c = 0; c < ncols; ++c)
    for (int k = 0; k <= N / 2; ++k) {
      Cx<double> Xk, Xnk;
      if (sign < 0) dft_pair_outputs_rows<double, -1, 1>(N, &k, ncols, Z.data() + c, tw.data(), &Xk, &Xnk);
      else dft_pair_outputs_rows<double, +1, 1>(N, &k, ncols, Z.data() + c, tw.data(), &Xk, &Xnk);
      V[k * ncols + c] = Xk;
      if (k != 0 && 2 * k != N) V[(N - k) * ncols + c] = Xnk;
      if (k >= 1 && k <= p.H) {
        const Cx<double>* col = Z.data() + c;
        double* s = Sv + (size_t)(k * ncols + c) * 4;
        s[0] = s[1] = s[2] = s[3] = 0.0;
        dft_pair_partial<double, 1>(N, &k, [=](int j) {
          const Cx<double> a = col[(1 + j) * ncols], b = col[(N - 1 - j) * ncols];
          return PairCx<double>{a.re, a.im, b.re, b.im};
        }, tw.data(), 0, p.H, s, s + 1, s + 2, s + 3);
      }
    }
  return p.nunits;
}

// ---- forward z lines
// out[10] = N, H, KP, nlines, k0, nout, MT, LT, nunits, Wm
void plane_z_plan(int N, int k0, int nout, int nlines, int nwaves, int64_t* out) {
  const PlaneMfmaZPlan p = plane_mfma_z_plan(N, k0, nout, nlines, nwaves);
  out[0] = p.N; out[1] = p.H; out[2] = p.KP; out[3] = p.nlines; out[4] = p.k0; out[5] = p.nout; out[6] = p.MT; out[7] = p.LT;
  out[8] = p.nunits; out[9] = p.Wm;
}
// cnt[l * nout + k - k0] += 1 for every output a matrix unit produces, walking waves, units, lanes and accumulator words as the
// kernel does; pad[0] = operands at padded positions or dead lines, pad[1] = those that plane_mfma_z_operand_live lets through
void plane_z_cover(int N, int k0, int nout, int nlines, int nwaves, int64_t* cnt, int64_t* pad) {
  const PlaneMfmaZPlan p = plane_mfma_z_plan(N, k0, nout, nlines, nwaves);
  pad[0] = pad[1] = 0;
  for (int wave = 0; wave < nwaves; ++wave)
    for (int u = wave; u < p.nunits; u += p.Wm) {
      const int mt = u % p.MT, lt = u / p.MT;
      for (int lane = 0; lane < 64; ++lane) {
        const int l = plane_mfma_z_line(lt, lane);
        for (int kk = lane >> 4; kk < p.KP; kk += 4)
          if (!(kk < p.H && l < nlines)) { ++pad[0]; if (plane_mfma_z_operand_live(p, kk, l)) ++pad[1]; }
        for (int r = 0; r < 4; ++r) {
          const int k = plane_mfma_z_out_k(p, mt, lane, r);
          if (l < nlines && k < k0 + nout) ++cnt[l * nout + k - k0];
        }
      }
    }
}
// real lines x [nlines][N]: Xm, Sm = every unit in the matrix-core order; Xv, Sv = rdft_outputs / real_pair_sums in double;
// X [nlines][nout] complex, S [nlines][nout][2] = (P, R); big[l] = the largest |pair sum| of line l
int plane_z_lines(int N, int k0, int nout, int nlines, int nwaves, const double* x, double* Xm, double* Xv, double* Sm, double* Sv,
                  double* big) {
  const PlaneMfmaZPlan p = plane_mfma_z_plan(N, k0, nout, nlines, nwaves);
  const int H = p.H;
  std::vector<Cx<double>> ps((size_t)H * nlines), tw(N);
  std::vector<double> x0(nlines), xn(nlines);
  for (int m = 0; m < N; ++m) tw[m] = Cx<double>{circ_cos(m, N), std::sin(2.0 * M_PI * (double)m / (double)N)};
  for (int l = 0; l < nlines; ++l) {
    const double* xl = x + (size_t)l * N;
    x0[l] = xl[0];
    xn[l] = (N & 1) ? 0.0 : xl[N / 2];
    big[l] = 0.0;
    for (int jj = 0; jj < H; ++jj) {
      const double a = xl[1 + jj], b = xl[N - 1 - jj];
      ps[(size_t)jj * nlines + l] = Cx<double>{a + b, a - b};
      big[l] = std::fmax(big[l], std::fmax(std::fabs(a + b), std::fabs(a - b)));
    }
  }
  for (int u = 0; u < p.nunits; ++u)
    plane_mfma_z_unit_host<double>(p, u, ps.data(), x0.data(), xn.data(), tw.data(), reinterpret_cast<Cx<double>*>(Xm), Sm);
  for (int l = 0; l < nlines; ++l)
    for (int k = k0; k < k0 + nout; ++k) {
      Cx<double> X;
      rdft_outputs<double, 1>(N, &k, nlines, ps.data() + l, x0[l], xn[l], tw.data(), &X);
      reinterpret_cast<Cx<double>*>(Xv)[l * nout + k - k0] = X;
      real_pair_sums<double, 1>(N, &k, nlines, ps.data() + l, tw.data(), Sv + (size_t)(l * nout + k - k0) * 2,
                                Sv + (size_t)(l * nout + k - k0) * 2 + 1);
    }
  return p.nunits;
}
}
