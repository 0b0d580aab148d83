// Direct (O(N^2) per line) discrete Fourier transforms for PME meshes whose dimensions rocFFT can only do with
// Bluestein's algorithm (a prime factor above 13 -- e.g. the 97^3 mesh the reference's setup_ewald_parameters,
// admp/pme.py:717-744, gives for examples/water_pol_1024).  Replaces jnp.fft.fftn / ifftn of the reference
// (admp/recip.py:410,414) exactly like the rocFFT path does (unnormalised both ways).
//
// Every line transform uses the j <-> N-j symmetry of the twiddles, w^(jk) = c_jk + i s_jk with c even and s odd in j:
//     X[k], X[N-k] = x_0 + sum_{j=1..H} (x_j + x_{N-j}) c_jk  +-  sgn i sum_{j=1..H} (x_j - x_{N-j}) s_jk   (+ x_{N/2} (-1)^k, N even)
// with H = (N-1)/2: one pass over the H pair sums yields two outputs, a quarter of the multiplications of the plain sum.
// The kernels are bound by LDS reads, not by arithmetic, so one thread produces KQ output pairs from one read of the
// pair sums and carries the twiddles by rotation instead of fetching them.
// The functions here are the per-output-pair arithmetic, shared by dft_kernels.hip and the host-compiled test shim.
#pragma once
#include "pme_math.h"

namespace admp {

template <class T>
struct alignas(2 * sizeof(T)) Cx {
  T re, im;
};
// pair sums of one line position: a = x_j + x_{N-j}, b = x_j - x_{N-j}
template <class T>
struct alignas(4 * sizeof(T)) PairCx {
  T are, aim, bre, bim;
};

// Each call produces KQ output pairs of one line (k[0..KQ)): the pair sums are read once for all of them, and the
// twiddle of output k is advanced by the rotation w^k from j to j+1, re-seeded from the exact table every kDftReseed
// steps (so the recurrence never runs longer than that; entries of k outside 0..N/2 may be passed as 0 and ignored).
constexpr int kDftReseed = 8;

template <class T>
ADMP_HD Cx<T> cx_mul(Cx<T> a, Cx<T> b) {
  return Cx<T>{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

// Twiddle of output k carried from line position j to j + 1.  f32: the rotation w <- w * w^k (4 operations).  f64, where an
// operation costs twice as much and the 97^3 headline mesh spends 40 % of its step in these loops: the three-term recurrence
// w_{j+1} = 2 cos(theta) w_j - w_{j-1}, one FMA per component; its error grows with j^2, which the re-seeding from the exact
// table every kDftReseed steps bounds at ~64 ulp of f64 (in f32 that would show, so f32 keeps the rotation).
template <class T>
struct TwStep {
  Cx<T> w, aux;     // f32: aux = w^k (the rotation); f64: aux = w_{j-1}
  T t;              // f64: 2 cos(theta)
  ADMP_HD void seed(const Cx<T>* tw, int m, int k, int N) {
    w = tw[m];
    if (sizeof(T) == 8) {
      int mp = m - k;
      if (mp < 0) mp += N;
      aux = tw[mp];
      t = T(2) * tw[k].re;
    } else {
      aux = tw[k];
      t = T(0);
    }
  }
  ADMP_HD void next() {
    if (sizeof(T) == 8) {
      const Cx<T> n{t * w.re - aux.re, t * w.im - aux.im};
      aux = w;
      w = n;
    } else {
      w = cx_mul(w, aux);
    }
  }
};

// complex line, direction SIGN (-1 forward, +1 inverse): outputs X[k] and X[N-k] (k = 0 .. N/2)
//   load(j), j = 0..H-1, returns the pair sums of line positions j+1 / N-1-j;  x0 = x_0;  xn = x_{N/2} (used when N is
//   even);  tw[m] = (cos, sin)(2 pi m / N)
// partial sums over the pair positions j = jb0 .. je0-1 (0-based: line positions j+1 / N-1-j), ADDED to Are .. Bim;
// jb0 must be a multiple of kDftReseed steps away from nothing in particular: the twiddle is seeded exactly at jb0
template <class T, int KQ, class LoadAB>
ADMP_HD void dft_pair_partial(int N, const int* k, LoadAB load, const Cx<T>* tw, int jb0, int je0, T* Are, T* Aim, T* Bre,
                              T* Bim) {
  TwStep<T> w[KQ];
  int m[KQ], step[KQ];
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    m[q] = jb0 == 0 ? k[q] : (int)(((long)k[q] * (jb0 + 1)) % N);
    step[q] = (kDftReseed * k[q]) % N;
  }
  for (int jb = jb0; jb < je0; jb += kDftReseed) {
#pragma unroll
    for (int q = 0; q < KQ; ++q) w[q].seed(tw, m[q], k[q], N);
    const int je = (je0 - jb) < kDftReseed ? (je0 - jb) : kDftReseed;
    if (je == kDftReseed) {
#pragma unroll
      for (int jj = 0; jj < kDftReseed; ++jj) {
        const PairCx<T> p = load(jb + jj);
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          Are[q] += p.are * w[q].w.re;
          Aim[q] += p.aim * w[q].w.re;
          Bre[q] += p.bre * w[q].w.im;
          Bim[q] += p.bim * w[q].w.im;
          w[q].next();
        }
      }
    } else {
      for (int jj = 0; jj < je; ++jj) {
        const PairCx<T> p = load(jb + jj);
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          Are[q] += p.are * w[q].w.re;
          Aim[q] += p.aim * w[q].w.re;
          Bre[q] += p.bre * w[q].w.im;
          Bim[q] += p.bim * w[q].w.im;
          w[q].next();
        }
      }
    }
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      m[q] += step[q];
      if (m[q] >= N) m[q] -= N;
    }
  }
}
// outputs from the complete sums
template <class T, int SIGN, int KQ>
ADMP_HD void dft_pair_finish(int N, const int* k, Cx<T> x0, Cx<T> xn, const T* Are, const T* Aim, const T* Bre, const T* Bim,
                             Cx<T>* Xk, Cx<T>* Xnk) {
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    T bre = x0.re + Are[q], bim = x0.im + Aim[q];
    if ((N & 1) == 0) {
      const T s = (k[q] & 1) ? T(-1) : T(1);
      bre += s * xn.re;
      bim += s * xn.im;
    }
    // sgn * i * B = sgn * (-Bim, Bre)
    Xk[q].re = bre - T(SIGN) * Bim[q];
    Xk[q].im = bim + T(SIGN) * Bre[q];
    Xnk[q].re = bre + T(SIGN) * Bim[q];
    Xnk[q].im = bim - T(SIGN) * Bre[q];
  }
}
template <class T, int SIGN, int KQ, class LoadAB>
ADMP_HD void dft_pair_core(int N, const int* k, LoadAB load, Cx<T> x0, Cx<T> xn, const Cx<T>* tw, Cx<T>* Xk, Cx<T>* Xnk) {
  T Are[KQ], Aim[KQ], Bre[KQ], Bim[KQ];
#pragma unroll
  for (int q = 0; q < KQ; ++q) Are[q] = Aim[q] = Bre[q] = Bim[q] = T(0);
  dft_pair_partial<T, KQ>(N, k, load, tw, 0, (N - 1) / 2, Are, Aim, Bre, Bim);
  dft_pair_finish<T, SIGN, KQ>(N, k, x0, xn, Are, Aim, Bre, Bim, Xk, Xnk);
}
// where a line is split between two threads: the first takes positions 0 .. dft_split(N)-1 (whole re-seed blocks)
ADMP_HD int dft_split(int N) {
  const int H = (N - 1) / 2, mid = ((H / 2 + kDftReseed - 1) / kDftReseed) * kDftReseed;
  return mid < H ? mid : H;
}
// pair sums stored as one record per position: ab[(j-1)*stride], j = 1..H
template <class T, int SIGN, int KQ>
ADMP_HD void dft_pair_outputs(int N, const int* k, int stride, const PairCx<T>* ab, Cx<T> x0, Cx<T> xn, const Cx<T>* tw,
                              Cx<T>* Xk, Cx<T>* Xnk) {
  dft_pair_core<T, SIGN, KQ>(N, k, [=](int j) { return ab[j * stride]; }, x0, xn, tw, Xk, Xnk);
}
// pair sums formed in place in a [N][stride] array of line values: row j holds x_j + x_{N-j}, row N-j holds x_j - x_{N-j}
template <class T, int SIGN, int KQ>
ADMP_HD void dft_pair_outputs_rows(int N, const int* k, int stride, const Cx<T>* col, const Cx<T>* tw, Cx<T>* Xk,
                                   Cx<T>* Xnk) {
  const Cx<T> x0 = col[0];
  const Cx<T> xn = (N & 1) ? Cx<T>{T(0), T(0)} : col[(N / 2) * stride];
  dft_pair_core<T, SIGN, KQ>(N, k, [=](int j) {
    const Cx<T> a = col[(1 + j) * stride], b = col[(N - 1 - j) * stride];
    return PairCx<T>{a.re, a.im, b.re, b.im};
  }, x0, xn, tw, Xk, Xnk);
}

// real pair sums shared by the r2c and c2r lines: P = sum_j p_j.re c_jk, R = sum_j p_j.im s_jk
template <class T, int KQ>
ADMP_HD void real_pair_partial(int N, const int* k, int stride, const Cx<T>* p, const Cx<T>* tw, int jb0, int je0, T* P, T* R) {
  TwStep<T> w[KQ];
  int m[KQ], step[KQ];
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    m[q] = jb0 == 0 ? k[q] : (int)(((long)k[q] * (jb0 + 1)) % N);
    step[q] = (kDftReseed * k[q]) % N;
  }
  for (int jb = jb0; jb < je0; jb += kDftReseed) {
#pragma unroll
    for (int q = 0; q < KQ; ++q) w[q].seed(tw, m[q], k[q], N);
    const int je = (je0 - jb) < kDftReseed ? (je0 - jb) : kDftReseed;
    if (je == kDftReseed) {
#pragma unroll
      for (int jj = 0; jj < kDftReseed; ++jj) {
        const Cx<T> v = p[(jb + jj) * stride];
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          P[q] += v.re * w[q].w.re;
          R[q] += v.im * w[q].w.im;
          w[q].next();
        }
      }
    } else {
      for (int jj = 0; jj < je; ++jj) {
        const Cx<T> v = p[(jb + jj) * stride];
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          P[q] += v.re * w[q].w.re;
          R[q] += v.im * w[q].w.im;
          w[q].next();
        }
      }
    }
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      m[q] += step[q];
      if (m[q] >= N) m[q] -= N;
    }
  }
}
template <class T, int KQ>
ADMP_HD void real_pair_sums(int N, const int* k, int stride, const Cx<T>* p, const Cx<T>* tw, T* P, T* R) {
#pragma unroll
  for (int q = 0; q < KQ; ++q) P[q] = R[q] = T(0);
  real_pair_partial<T, KQ>(N, k, stride, p, tw, 0, (N - 1) / 2, P, R);
}

// r2c line: p_j = (x_j + x_{N-j}, x_j - x_{N-j}) real pair sums; X[k] = x0 + P - i R  (+ xn (-1)^k), k = 0 .. N/2
template <class T, int KQ>
ADMP_HD void rdft_outputs(int N, const int* k, int stride, const Cx<T>* p, T x0, T xn, const Cx<T>* tw, Cx<T>* X) {
  T P[KQ], R[KQ];
  real_pair_sums<T, KQ>(N, k, stride, p, tw, P, R);
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    X[q].re = x0 + P[q];
    if ((N & 1) == 0) X[q].re += (k[q] & 1) ? -xn : xn;
    X[q].im = -R[q];
  }
}

// c2r line of a Hermitian half spectrum: p_k = X[k], k = 1..H; x_j = X0.re + 2(P - R), x_{N-j} = X0.re + 2(P + R)
// (+ X[N/2].re (-1)^j); the imaginary parts of X[0] and X[N/2] are ignored like rocFFT's c2r does.
template <class T, int KQ>
ADMP_HD void irdft_pair_outputs(int N, const int* j, int stride, const Cx<T>* p, T X0re, T Xnre, const Cx<T>* tw, T* xj,
                                T* xnj) {
  T P[KQ], R[KQ];
  real_pair_sums<T, KQ>(N, j, stride, p, tw, P, R);
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    T base = X0re + T(2) * P[q];
    if ((N & 1) == 0) base += (j[q] & 1) ? -Xnre : Xnre;
    xj[q] = base - T(2) * R[q];
    xnj[q] = base + T(2) * R[q];
  }
}

// ---- the x pass of the convolution as ONE real circulant product ---------------------------------------------------------
// For one column (ky, kz) the x pass is out = F^-1 diag(G) F in (both unnormalised).  Where G(k) = G(N - k) along the line --
// every orthorhombic cell, both k-point orders -- that is the circulant matrix with the real, even first column
//     c[d] = sum_k G(k) e^(2 pi i k d / N) = G(0) + sum_{k=1..H} (G(k) + G(N-k)) cos(2 pi k d / N)   (+ (-1)^d G(N/2), N even)
// and with the pair sums a_j = x_j + x_{N-j}, b_j = x_j - x_{N-j} the kernels stage anyway
//     P_i = out_i + out_{N-i} = 2 c[i] x_0 + sum_j (c[i-j] + c[i+j]) a_j    (+ 2 c[i - N/2] x_{N/2}, N even)
//     M_i = out_i - out_{N-i} =              sum_j (c[i-j] - c[i+j]) b_j
// one loop over the H pair positions instead of a forward and an inverse transform, no twiddles, no spectrum S.  The energy
// the pass sums in k space follows from Parseval: sum_k G |S_k|^2 = sum_x Re(conj(in_x) out_x), and for a pair of outputs
// conj(x_i) out_i + conj(x_{N-i}) out_{N-i} = (conj(a_i) P_i + conj(b_i) M_i) / 2.
// The column's table is passed EXTENDED so that the loop has no index arithmetic: ce[e * cstride] = c[e mod N], e running
// from -(N/2) to N/2 + H (circ_ext_len entries, ce pointing at e = 0).

// entry d of the first column in double; gs(k) = G(k) + G(N-k), k = 1..H
ADMP_HD double circ_cos(int m, int N) {          // cos(2 pi m / N), 0 <= m < N, argument reduced to [0, pi/2]
  if (2 * m > N) m = N - m;
  const double pi = 3.141592653589793;
  return 4 * m > N ? -cos(pi * (double)(N - 2 * m) / (double)N) : cos(pi * (double)(2 * m) / (double)N);
}
// cosm(m) = cos(2 pi m / N), 0 <= m < N: circ_cos, or a table of it
template <class LoadGs, class CosM>
ADMP_HD double circ_table_entry(int N, int d, double G0, LoadGs gs, double Gn, CosM cosm) {
  const int H = (N - 1) / 2;
  double c = G0;
  int m = 0;
  for (int k = 1; k <= H; ++k) {
    m += d;
    if (m >= N) m -= N;
    c += gs(k) * cosm(m);
  }
  if ((N & 1) == 0) c += (d & 1) ? -Gn : Gn;
  return c;
}
// The premise, checked per column on the STORED table (type T, unit roundoff ulp): G(k) and G(N-k) come out of the same
// formula at mirrored integer frequencies, so in a cell where they are equal they differ by the rounding of that evaluation
// in double (a product chain of ~20 operations and one exp: a few ulp of double, nothing in f32) plus half an ulp of T each
// from the store.  kCircEvenUlps = 8 ulp of T of the column's largest |G| covers that; a triclinic cell misses it by many
// orders (its mixed terms change G by O(1) relative amounts).
constexpr double kCircEvenUlps = 8.0;
template <class LoadG>
ADMP_HD bool circ_column_even(int N, LoadG G, double ulp) {
  const int H = (N - 1) / 2;
  double gmax = fabs(G(0));
  for (int k = 1; k < N; ++k) { const double g = fabs(G(k)); gmax = g > gmax ? g : gmax; }
  bool ok = true;
  for (int k = 1; k <= H; ++k) ok = ok && fabs(G(k) - G(N - k)) <= kCircEvenUlps * ulp * gmax;
  return ok;
}
ADMP_HD int circ_ext_len(int N) { return N / 2 + N / 2 + (N - 1) / 2 + 1; }
// index into c[0 .. N/2] of extended position e (-(N/2) <= e <= N/2 + H)
ADMP_HD int circ_fold(int e, int N) {
  if (e < 0) e = -e;
  return 2 * e > N ? N - e : e;
}

// KQ pairs (P_i, M_i) of one line, i = i[0..KQ) in 0 .. N/2 (entries outside may be passed as 0 and ignored):
// pair sums ab[(j-1) * stride], j = 1..H; x0 = x_0; xn = x_{N/2} (N even)
template <class T>
ADMP_HD void circ_step(const PairCx<T>& p, T c1, T c2, Cx<T>& P, Cx<T>& M) {
  const T s = c1 + c2, d = c1 - c2;
  P.re += s * p.are;
  P.im += s * p.aim;
  M.re += d * p.bre;
  M.im += d * p.bim;
}
// steps unrolled together (their LDS reads are in flight at once).  Measured at 97^3 f64: 2 -> +1.1 us on the plain kernel;
// 8 -> -0.5 us there, but the rider kernel (pair_kernels.hip k_xconv_pair) then needs 191 registers instead of the field
// workgroups' 165, drops to two waves per SIMD and loses 3 us.
constexpr int kCircUnroll = 4;
template <class T, int KQ>
ADMP_HD void circ_pair_outputs(int N, const int* i, int cstride, const T* ce, int stride, const PairCx<T>* ab, Cx<T> x0,
                               Cx<T> xn, Cx<T>* P, Cx<T>* M) {
  const int H = (N - 1) / 2;
  const T* cm[KQ];
  const T* cp[KQ];
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    const T c0 = T(2) * ce[i[q] * cstride];
    P[q] = Cx<T>{c0 * x0.re, c0 * x0.im};
    M[q] = Cx<T>{T(0), T(0)};
    if ((N & 1) == 0) {
      const T cn = T(2) * ce[(i[q] - N / 2) * cstride];
      P[q].re += cn * xn.re;
      P[q].im += cn * xn.im;
    }
    cm[q] = ce + (i[q] - 1) * cstride;      // c[i - j] at j = 1, walking down
    cp[q] = ce + (i[q] + 1) * cstride;      // c[i + j] at j = 1, walking up
  }
  int j = 0;
  for (; j + kCircUnroll <= H; j += kCircUnroll) {
#pragma unroll
    for (int jj = 0; jj < kCircUnroll; ++jj) {
      const PairCx<T> p = ab[(j + jj) * stride];
#pragma unroll
      for (int q = 0; q < KQ; ++q) circ_step(p, cm[q][-(j + jj) * cstride], cp[q][(j + jj) * cstride], P[q], M[q]);
    }
  }
  for (; j < H; ++j) {
    const PairCx<T> p = ab[j * stride];
#pragma unroll
    for (int q = 0; q < KQ; ++q) circ_step(p, cm[q][-j * cstride], cp[q][j * cstride], P[q], M[q]);
  }
}
// sum over the outputs i and N - i of Re(conj(in) out), in double: ai = the pair sums of position i (unused for i = 0, N/2)
template <class T>
ADMP_HD double circ_pair_energy(int N, int i, Cx<T> P, Cx<T> M, const PairCx<T>& ai, Cx<T> x0, Cx<T> xn) {
  if (i == 0) return 0.5 * ((double)x0.re * P.re + (double)x0.im * P.im);
  if (2 * i == N) return 0.5 * ((double)xn.re * P.re + (double)xn.im * P.im);
  return 0.5 * ((double)ai.are * P.re + (double)ai.aim * P.im + (double)ai.bre * M.re + (double)ai.bim * M.im);
}

// largest prime factor (host): rocFFT has radix kernels for 2, 3, 5, 7, 11, 13 and falls back to Bluestein above
inline int largest_prime_factor(int n) {
  int best = 1;
  for (int p = 2; (long)p * p <= n; ++p)
    while (n % p == 0) {
      best = p;
      n /= p;
    }
  return n > 1 ? (n > best ? n : best) : best;
}

}  // namespace admp
