// Pieces of the direct-DFT line kernels shared between dft_kernels.hip and the kernels that run an x pass next to other
// work (pair_kernels.hip k_xconv_pair): task helpers, the pair-sum loader and the body of the x pass (block size and launch
// shape: dft_plan.h).
#pragma once
#include "dft_math.h"
#include "dft_plan.h"
#include "launch.h"
#include "reduce.h"
#include "rider_layout.h"

namespace admp {

extern __shared__ __align__(32) unsigned char dft_smem[];

// task index of a thread and which half of the pair positions it sums (JS = 2: lanes 2i, 2i+1 share task i)
template <int JS>
__device__ __forceinline__ void dft_task_of_thread(int& tid, int& half) {
  tid = JS == 2 ? (int)(threadIdx.x >> 1) : (int)threadIdx.x;
  half = JS == 2 ? (int)(threadIdx.x & 1) : 0;
}
template <class T>
__device__ __forceinline__ T pair_lane_sum(T v) { return v + __shfl_xor(v, 1, 64); }

// dft_pair_core / real_pair_sums over this thread's share of the positions, shares combined: every lane gets the full outputs
template <class T, int SIGN, int KQ, int JS>
__device__ __forceinline__ void dft_pair_outputs_js(int N, const int* k, int stride, const PairCx<T>* ab, Cx<T> x0, Cx<T> xn,
                                                    const Cx<T>* tw, int half, Cx<T>* Xk, Cx<T>* Xnk) {
  T Are[KQ], Aim[KQ], Bre[KQ], Bim[KQ];
#pragma unroll
  for (int q = 0; q < KQ; ++q) Are[q] = Aim[q] = Bre[q] = Bim[q] = T(0);
  const int H = (N - 1) / 2, mid = JS == 2 ? dft_split(N) : H;
  dft_pair_partial<T, KQ>(N, k, [=](int j) { return ab[j * stride]; }, tw, half ? mid : 0, half ? H : mid, Are, Aim, Bre, Bim);
  if (JS == 2) {
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      Are[q] = pair_lane_sum(Are[q]); Aim[q] = pair_lane_sum(Aim[q]);
      Bre[q] = pair_lane_sum(Bre[q]); Bim[q] = pair_lane_sum(Bim[q]);
    }
  }
  dft_pair_finish<T, SIGN, KQ>(N, k, x0, xn, Are, Aim, Bre, Bim, Xk, Xnk);
}
template <class T, int KQ, int JS>
__device__ __forceinline__ void real_pair_sums_js(int N, const int* k, int stride, const Cx<T>* p, const Cx<T>* tw, int half,
                                                  T* P, T* R) {
#pragma unroll
  for (int q = 0; q < KQ; ++q) P[q] = R[q] = T(0);
  const int H = (N - 1) / 2, mid = JS == 2 ? dft_split(N) : H;
  real_pair_partial<T, KQ>(N, k, stride, p, tw, half ? mid : 0, half ? H : mid, P, R);
  if (JS == 2) {
#pragma unroll
    for (int q = 0; q < KQ; ++q) { P[q] = pair_lane_sum(P[q]); R[q] = pair_lane_sum(R[q]); }
  }
}

// stage a tile of NC strided complex lines as pair sums: element (j, c) at spec[base + j * jstride + c]
template <class T>
__device__ __forceinline__ void load_pairs(int N, int NC, int nca, const Cx<T>* __restrict__ spec, long base, long jstride,
                                           PairCx<T>* ab, Cx<T>* x0, Cx<T>* xn) {
  const int H = (N - 1) / 2;
  for (int t = threadIdx.x; t < H * NC; t += kDftBlock) {
    const int jj = t / NC, c = t - jj * NC;
    PairCx<T> v{T(0), T(0), T(0), T(0)};
    if (c < nca) {
      const Cx<T> a = spec[base + (long)(1 + jj) * jstride + c], b = spec[base + (long)(N - 1 - jj) * jstride + c];
      v = PairCx<T>{a.re + b.re, a.im + b.im, a.re - b.re, a.im - b.im};
    }
    ab[t] = v;
  }
  if (threadIdx.x < NC) {
    const int c = threadIdx.x;
    Cx<T> a{T(0), T(0)}, b{T(0), T(0)};
    if (c < nca) {
      a = spec[base + c];
      if ((N & 1) == 0) b = spec[base + (long)(N / 2) * jstride + c];
    }
    x0[c] = a;
    xn[c] = b;
  }
}

// ---- x lines: forward, multiply by G (accumulating sum w G |S|^2, recip.py:400-414 / pme.py:240), inverse; in place
// (the body of k_dft_x_conv as a device function: bx, by, bz = the block's tile, y row and batch channel -- also run by the
// workgroups of k_xconv_pair, pair_kernels.hip, next to the workgroups of a real-space field kernel)
template <class T>
struct XConvArgs {
  int N, ncols, NC, TK;
  long jstride, fixstride;
  int K3;
  Cx<T>* spec;
  DftTabs<T> tabs;
  const Cx<T>* twg;
  double* energies;
  int slot;
  long spec_stride;
  const T* ctab = nullptr;      // circulant form (dft_x_circ_body): first columns [N/2+1][K2][K3/2+1] of the slot-0 G table
};
// the arguments of an x pass of shape p (dft_plan.h: dft_x_plan(K, sizeof(T), ctab != nullptr)) over the spectrum of mesh K;
// spec_stride: reals between the spectra of a batch (the transform form only)
template <class T>
inline XConvArgs<T> dft_x_args(const XPassPlan& p, const int K[3], const T* tw, T* spec, const DftTabs<T>& tabs, double* energies,
                               int slot, const T* ctab = nullptr, long spec_stride = 0) {
  static_assert(sizeof(Cx<T>) == 2 * sizeof(T) && sizeof(PairCx<T>) == 4 * sizeof(T), "dft_plan.h counts LDS in words");
  XConvArgs<T> xa{p.N, p.Kh, p.NC, p.TK, (long)K[1] * p.Kh, (long)p.Kh, K[2], reinterpret_cast<Cx<T>*>(spec), tabs,
                  reinterpret_cast<const Cx<T>*>(tw), energies, slot, spec_stride / 2};
  xa.ctab = ctab;
  return xa;
}
template <class T, int KQ, int JS>
__device__ __forceinline__ void dft_x_conv_body(const XConvArgs<T>& xa, int bx, int by, int bz) {
  const int N = xa.N, ncols = xa.ncols, NC = xa.NC, TK = xa.TK, K3 = xa.K3, slot = xa.slot;
  const long jstride = xa.jstride, fixstride = xa.fixstride;
  const Cx<T>* __restrict__ twg = xa.twg;
  double* energies = xa.energies;
  Cx<T>* __restrict__ spec = xa.spec + bz * xa.spec_stride;
  const T* __restrict__ gtab = xa.tabs.p[bz];
  const int H = (N - 1) / 2, Kh = N / 2 + 1;
  PairCx<T>* ab = reinterpret_cast<PairCx<T>*>(dft_smem);   // [H][NC]
  Cx<T>* tw = reinterpret_cast<Cx<T>*>(ab + H * NC);          // [N]
  Cx<T>* x0 = tw + N;                                         // [NC]
  Cx<T>* xn = x0 + NC;                                        // [NC]
  Cx<T>* S = xn + NC;                                         // [N][NC]
  const int col0 = bx * NC;
  const int nca = min(NC, ncols - col0);
  const long base = (long)by * fixstride + col0;
  for (int t = threadIdx.x; t < N; t += kDftBlock) tw[t] = twg[t];
  // the G values this thread multiplies with after the forward transform: fetched now, so that their latency hides
  // behind the transform instead of sitting between two barriers (H * NC < KQ * kDftBlock by construction of NC)
  T Gp[KQ][2], G0 = T(0), Gn = T(0);
#pragma unroll
  for (int u = 0; u < KQ; ++u) {
    Gp[u][0] = Gp[u][1] = T(0);
    const int t = threadIdx.x + u * kDftBlock;
    if (t < H * NC) {
      const int jj = t / NC, cc = t - jj * NC;
      if (cc < nca) {
        Gp[u][0] = gtab[base + (long)(1 + jj) * jstride + cc];
        Gp[u][1] = gtab[base + (long)(N - 1 - jj) * jstride + cc];
      }
    }
  }
  if (threadIdx.x < nca) {
    G0 = gtab[base + threadIdx.x];
    if ((N & 1) == 0) Gn = gtab[base + (long)(N / 2) * jstride + threadIdx.x];
  }
  load_pairs<T>(N, NC, nca, spec, base, jstride, ab, x0, xn);
  __syncthreads();
  int tid, half;
  dft_task_of_thread<JS>(tid, half);
  const int g = tid / NC, c = tid - g * NC;
  const bool task = g < TK && c < nca;
  int k[KQ];
#pragma unroll
  for (int q = 0; q < KQ; ++q) k[q] = (g + q * TK < Kh) ? g + q * TK : 0;
  if (task) {
    Cx<T> Xk[KQ], Xnk[KQ];
    dft_pair_outputs_js<T, -1, KQ, JS>(N, k, NC, ab + c, x0[c], xn[c], tw, half, Xk, Xnk);
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const int kq = g + q * TK;
      if (kq < Kh) {
        if (JS == 1 || half == 0) S[kq * NC + c] = Xk[q];
        if ((JS == 1 || half == 1) && kq != 0 && 2 * kq != N) S[(N - kq) * NC + c] = Xnk[q];
      }
    }
  }
  __syncthreads();
  double e = 0.0;
#pragma unroll
  for (int u = 0; u < KQ; ++u) {
    const int t = threadIdx.x + u * kDftBlock;
    if (t >= H * NC) continue;
    const int jj = t / NC, cc = t - jj * NC;
    PairCx<T> v{T(0), T(0), T(0), T(0)};
    if (cc < nca) {
      const int k1 = 1 + jj, k2 = N - 1 - jj, kz = col0 + cc;
      const T G1 = Gp[u][0], G2 = Gp[u][1];
      const Cx<T> s1 = S[k1 * NC + cc], s2 = S[k2 * NC + cc];
      const double w = (kz == 0 || ((K3 & 1) == 0 && kz == K3 / 2)) ? 0.5 : 1.0;
      e += w * ((double)G1 * ((double)s1.re * s1.re + (double)s1.im * s1.im) +
                (double)G2 * ((double)s2.re * s2.re + (double)s2.im * s2.im));
      const T ar = G1 * s1.re, ai = G1 * s1.im, br = G2 * s2.re, bi = G2 * s2.im;
      v = PairCx<T>{ar + br, ai + bi, ar - br, ai - bi};
    }
    ab[t] = v;
  }
  if (threadIdx.x < NC) {
    const int cc = threadIdx.x;
    Cx<T> a{T(0), T(0)}, b{T(0), T(0)};
    if (cc < nca) {
      const int kz = col0 + cc;
      const double w = (kz == 0 || ((K3 & 1) == 0 && kz == K3 / 2)) ? 0.5 : 1.0;
      const Cx<T> s0 = S[cc];
      e += w * (double)G0 * ((double)s0.re * s0.re + (double)s0.im * s0.im);
      a = Cx<T>{G0 * s0.re, G0 * s0.im};
      if ((N & 1) == 0) {
        const Cx<T> sn = S[(N / 2) * NC + cc];
        e += w * (double)Gn * ((double)sn.re * sn.re + (double)sn.im * sn.im);
        b = Cx<T>{Gn * sn.re, Gn * sn.im};
      }
    }
    x0[cc] = a;
    xn[cc] = b;
  }
  __syncthreads();
  if (task) {
    Cx<T> Xk[KQ], Xnk[KQ];
    dft_pair_outputs_js<T, +1, KQ, JS>(N, k, NC, ab + c, x0[c], xn[c], tw, half, Xk, Xnk);
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const int kq = g + q * TK;
      if (kq < Kh) {
        if (JS == 1 || half == 0) spec[base + (long)kq * jstride + c] = Xk[q];
        if ((JS == 1 || half == 1) && kq != 0 && 2 * kq != N) spec[base + (long)(N - kq) * jstride + c] = Xnk[q];
      }
    }
  }
  e = block_reduce_sum<kDftBlock>(e);
  if (threadIdx.x == 0) atomicAdd(&energies[slot], e);
}

// ---- x lines as one real circulant product (dft_math.h circ_pair_outputs): same tile, same in-place store and the same
// energy word as dft_x_conv_body, for G tables that are even along x (xa.ctab: built and checked by k_ctab, dft_kernels.hip).
// One loop over the pair positions, one barrier; LDS: the pair sums and the tile's extended table [circ_ext_len][NC].
// The energy sum is skipped for slot E_SCRATCH (convolutions whose energy nobody reads: the SCF increments).
template <class T, int KQ>
__device__ __forceinline__ void dft_x_circ_body(const XConvArgs<T>& xa, int bx, int by) {
  const bool ENERGY = xa.slot != E_SCRATCH;      // (workgroup-uniform)
  const int N = xa.N, ncols = xa.ncols, NC = xa.NC, TK = xa.TK, K3 = xa.K3;
  const long jstride = xa.jstride;
  Cx<T>* __restrict__ spec = xa.spec;
  const T* __restrict__ ctab = xa.ctab;
  const int H = (N - 1) / 2, Kh = N / 2 + 1;
  PairCx<T>* ab = reinterpret_cast<PairCx<T>*>(dft_smem);   // [H][NC]
  Cx<T>* x0 = reinterpret_cast<Cx<T>*>(ab + H * NC);          // [NC]
  Cx<T>* xn = x0 + NC;                                        // [NC]
  T* cext = reinterpret_cast<T*>(xn + NC);                    // [circ_ext_len(N)][NC], row 0 = extended position -(N/2)
  const int col0 = bx * NC;
  const int nca = min(NC, ncols - col0);
  const long base = (long)by * xa.fixstride + col0;
  for (int t = threadIdx.x; t < Kh * NC; t += kDftBlock) {      // c[d] sits at the extended positions d, -d and N - d
    const int d = t / NC, cc = t - d * NC;
    const T v = cc < nca ? ctab[base + (long)d * jstride + cc] : T(0);
    cext[(N / 2 + d) * NC + cc] = v;
    cext[(N / 2 - d) * NC + cc] = v;
    if (N - d <= N / 2 + H) cext[(N / 2 + N - d) * NC + cc] = v;
  }
  load_pairs<T>(N, NC, nca, spec, base, jstride, ab, x0, xn);
  __syncthreads();
  const int g = (int)threadIdx.x / NC, c = (int)threadIdx.x - g * NC;
  double e = 0.0;
  if (g < TK && c < nca) {
    int i[KQ];
#pragma unroll
    for (int q = 0; q < KQ; ++q) i[q] = (g + q * TK < Kh) ? g + q * TK : 0;
    Cx<T> P[KQ], M[KQ];
    circ_pair_outputs<T, KQ>(N, i, NC, cext + (N / 2) * NC + c, NC, ab + c, x0[c], xn[c], P, M);
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const int iq = g + q * TK;
      if (iq < Kh) {
        const bool single = iq == 0 || 2 * iq == N;
        if (ENERGY) e += circ_pair_energy<T>(N, iq, P[q], M[q], ab[(single ? 0 : iq - 1) * NC + c], x0[c], xn[c]);
        spec[base + (long)iq * jstride + c] = Cx<T>{T(0.5) * (P[q].re + M[q].re), T(0.5) * (P[q].im + M[q].im)};
        if (!single) spec[base + (long)(N - iq) * jstride + c] = Cx<T>{T(0.5) * (P[q].re - M[q].re), T(0.5) * (P[q].im - M[q].im)};
      }
    }
    const int kz = col0 + c;
    if (ENERGY && (kz == 0 || ((K3 & 1) == 0 && kz == K3 / 2))) e *= 0.5;
  }
  if (ENERGY) {
    e = block_reduce_sum<kDftBlock>(e);
    if (threadIdx.x == 0) atomicAdd(&xa.energies[xa.slot], e);
  }
}

}  // namespace admp
