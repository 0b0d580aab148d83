// Do matrix-core tiles pay next to the vector form INSIDE a line phase of the plane kernels (dft_kernels.hip k_dft_zy_fwd)?
// Part 1: the y-line phase of the forward kernel at 97^3 f64 on synthetic data -- one 1024-thread workgroup per CU on 194 CUs,
// LDS carved as ZyLayout<double>(97, 97), 24 / 25 complex columns, 49 output pairs -- in three forms in one binary:
//   S = 0      vector only: dft_pair_outputs_rows<double, -1, 2>, task loop and stores as the kernel has them
//   S = 1,2,3  hybrid: waves [0, 3 S) each take one (16-output tile, 8-column tile) unit as Mfma<double>::mma tiles indexed
//              by TwIdx (k = 0, a plain column sum, rides in the operand fetches of the first output tile); the other
//              waves run the kernel's task loop over the remaining columns
//   S = 4      matrix only: every column in tiles (the fourth column tile masked down to 0 / 1 column)
// The phase is repeated between barriers and stamped with wall_clock64 (100 MHz) by thread 0, as ADMP_DFTM_TRACE did.
// Part 2: the phases of the library's k_dft_zy_fwd<double, 2, false / true> in the vector form (ADMP_DFT_PLANE_MFMA=0) and with
// the matrix-core share, and of k_dft_yz_inv<double, 2, false / true> the same way, at 97^3 (ADMP_ZY_TRACE).
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -fno-slp-vectorize -DADMP_ZY_TRACE \
//     -Iadmp_amd/csrc -Iinclude tools/ubench/plane_hybrid.hip -o plane_hybrid
// run: plane_hybrid [out.json]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../admp_amd/csrc/dft_kernels.hip"
#include "../../admp_amd/csrc/mfma.h"

using namespace admp;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 1; } } while (0)

constexpr int kReps = 8;          // phases per launch (the first one is left out of the means)

// one (16-output tile mt, 8-column tile ct) unit of the y lines: P = C S, R = S' D with the paired rows of Z as the data
// operand (row 1 + jj: sums, row N - 1 - jj: differences; the 16 data columns are the real, then the imaginary parts of 8
// complex columns) and the exact table twiddles as the other
template <int SIGN>
__device__ __forceinline__ void y_unit(int lane, int N, int Kl, int Kh, int kz0, int mt, int ct, const Cx<double>* Z, const Cx<double>* tw,
                                       Cx<double>* out) {
  typedef Mfma<double>::Acc Acc;
  const int H = (N - 1) / 2, KP = (H + 3) & ~3;
  const int lo = lane & 15, hi = lane >> 4;
  const int i = 16 * mt + lo;
  TwIdx ti(i < H ? i : 0, hi, N);
  const int c = 8 * ct + (lo & 7), comp = lo >> 3;
  const bool live = c < Kl;
  const double* zc = reinterpret_cast<const double*>(Z + (live ? c : 0)) + comp;
  const int rs = 2 * Kl;                                      // row stride in words
  struct Ops { Cx<double> w; double b[2]; };
  auto fetch = [&](Ops& o, int kk) {
    o.w = tw[ti.m];
    ti.step();
    const bool ok = live && kk < H;
    o.b[0] = ok ? zc[(1 + kk) * rs] : 0.0;
    o.b[1] = ok ? zc[(N - 1 - kk) * rs] : 0.0;
  };
  Acc P = {0, 0, 0, 0}, R = {0, 0, 0, 0};
  double s0 = 0.0;                                            // this lane's share of the column sum (output k = 0)
  auto mul = [&](const Ops& o) {
    s0 += o.b[0];
    P = Mfma<double>::mma(o.w.re, o.b[0], P);
    R = Mfma<double>::mma(o.w.im, o.b[1], R);
  };
  Ops A, B;
  fetch(A, hi);
  for (int kk = hi; kk < KP; kk += 8) {
    const bool two = kk + 4 < KP;
    if (two) fetch(B, kk + 4);
    mul(A);
    if (kk + 8 < KP) fetch(A, kk + 8);
    if (two) mul(B);
  }
  const double x0 = zc[0], xn = (N & 1) ? 0.0 : zc[(N / 2) * rs];
  double* o = reinterpret_cast<double*>(out + kz0 + c) + comp;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = 1 + 16 * mt + Mfma<double>::row(lane, r);
    const double other = __shfl_xor(R[r], 8, 64);
    if (live && k <= H) {
      double base = x0 + P[r];
      if ((N & 1) == 0) base += (k & 1) ? -xn : xn;
      const double q = comp ? double(SIGN) * other : -double(SIGN) * other;      // im: + sgn R.re ; re: - sgn R.im
      o[2 * (long)k * Kh] = base + q;
      o[2 * (long)(N - k) * Kh] = base - q;
    }
  }
  s0 += __shfl_xor(s0, 16, 64);
  s0 += __shfl_xor(s0, 32, 64);
  if (mt == 0 && hi == 0 && live) o[0] = x0 + s0 + xn;        // X_0 = x_0 + sum_j (x_j + x_{N-j}) (+ x_{N/2}, N even)
}

template <int S>
__global__ __launch_bounds__(kZyBlock) void k_yphase(int N2, int N3, Cx<double>* __restrict__ spec,
                                                    const Cx<double>* __restrict__ tw2g, long long* __restrict__ stamps) {
  constexpr int KQ = 2;
  const ZyLayout<double> L(N2, N3);
  const int Kh = N3 / 2 + 1, H2 = (N2 - 1) / 2;
  const int kz0 = (int)(((long)Kh * blockIdx.z) / gridDim.z), kz1 = (int)(((long)Kh * (blockIdx.z + 1)) / gridDim.z);
  const int Kl = kz1 - kz0;
  Cx<double>* tw2 = reinterpret_cast<Cx<double>*>(dft_smem + L.tw2);
  Cx<double>* Z = reinterpret_cast<Cx<double>*>(dft_smem + L.b);          // [N2][Kl], rows paired along y
  Cx<double>* out = spec + (long)blockIdx.x * N2 * Kh;
  for (int t = threadIdx.x; t < N2; t += kZyBlock) tw2[t] = tw2g[t];
  for (int t = threadIdx.x; t < N2 * Kl; t += kZyBlock) {
    const int j = t / Kl, c = t - j * Kl;
    const double a = 0.37 * (double)(j * Kh + kz0 + c) + 0.11 * (double)blockIdx.x, b = 1.7 * a;      // words in [-0.5, 0.5)
    Z[t] = Cx<double>{a - floor(a) - 0.5, b - floor(b) - 0.5};
  }
  long long* st = stamps + (size_t)(blockIdx.z * gridDim.x + blockIdx.x) * 2 * kReps;
  const int MT = (H2 + 15) / 16;
  const int Wm = S * MT;                                     // matrix waves
  const int nm = S == 0 ? 0 : min(8 * S, Kl);                // matrix columns [0, nm)
  const int Kh2 = N2 / 2 + 1, TK2 = (Kh2 + KQ - 1) / KQ;
  __syncthreads();
  for (int rep = 0; rep < kReps; ++rep) {
    if (threadIdx.x == 0) st[2 * rep] = wall_clock64();
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));      // every repetition sets up its indices and addresses, as a launch of the kernel does
    const int wave = tid >> 6;
    if (S > 0 && wave < Wm) {
      y_unit<-1>(tid & 63, N2, Kl, Kh, kz0, wave % MT, wave / MT, Z, tw2, out);
    } else {
      // vector tasks: (group g, column c) over the columns [nm, Kl)
      const int nv = Kl - nm;
      for (int task = tid - 64 * Wm; task < TK2 * nv; task += kZyBlock - 64 * Wm) {
        const int g = task / nv, c = nm + task - g * nv;
        int k[KQ];
#pragma unroll
        for (int q = 0; q < KQ; ++q) k[q] = (g + q * TK2 < Kh2) ? g + q * TK2 : 0;
        Cx<double> Xk[KQ], Xnk[KQ];
        dft_pair_outputs_rows<double, -1, KQ>(N2, k, Kl, Z + c, tw2, Xk, Xnk);
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          const int kq = g + q * TK2;
          if (kq < Kh2) {
            out[(long)kq * Kh + kz0 + c] = Xk[q];
            if (kq != 0 && 2 * kq != N2) out[(long)(N2 - kq) * Kh + kz0 + c] = Xnk[q];
          }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) st[2 * rep + 1] = wall_clock64();
  }
}

struct Stat { double mean, z0, z1, worst; };
static Stat phase_stat(const std::vector<long long>& t, int nx) {      // ns; reps 1 .. kReps-1
  Stat s{0, 0, 0, 0};
  for (int z = 0; z < 2; ++z)
    for (int b = 0; b < nx; ++b)
      for (int r = 1; r < kReps; ++r) {
        const size_t o = (size_t)(z * nx + b) * 2 * kReps + 2 * r;
        const double d = (double)(t[o + 1] - t[o]) * 10.0;
        (z ? s.z1 : s.z0) += d / (nx * (kReps - 1));
        s.worst = std::max(s.worst, d);
      }
  s.mean = 0.5 * (s.z0 + s.z1);
  return s;
}

typedef void (*YKern)(int, int, Cx<double>*, const Cx<double>*, long long*);

int main(int argc, char** argv) {
  const int K[3] = {97, 97, 97};
  const int N = 97, Kh = N / 2 + 1, nx = 97;
  FILE* js = argc > 1 ? fopen(argv[1], "w") : nullptr;
  const size_t nspec = (size_t)nx * N * Kh, nmesh = (size_t)nx * N * N;
  std::vector<double> tw(2 * 3 * N);
  for (int d = 0; d < 3; ++d)
    for (int m = 0; m < N; ++m) { tw[2 * (d * N + m)] = std::cos(2 * M_PI * m / N); tw[2 * (d * N + m) + 1] = std::sin(2 * M_PI * m / N); }
  double *spec, *twd, *mesh;
  long long* tr;
  const size_t ntr = std::max<size_t>((size_t)2 * nx * 2 * kReps, (size_t)2 * nx * 8);
  CHECK(hipMalloc(&spec, nspec * 16)); CHECK(hipMalloc(&twd, tw.size() * 8)); CHECK(hipMalloc(&mesh, nmesh * 8));
  CHECK(hipMalloc(&tr, ntr * 8));
  CHECK(hipMemcpy(twd, tw.data(), tw.size() * 8, hipMemcpyHostToDevice));
  const Cx<double>* t1 = reinterpret_cast<const Cx<double>*>(twd) + N;
  const size_t sh = ZyLayout<double>(N, N).total;
  const dim3 grid(nx, 1, 2);

  // ---- part 1
  const YKern kern[5] = {k_yphase<0>, k_yphase<1>, k_yphase<2>, k_yphase<3>, k_yphase<4>};
  const char* name[5] = {"vector", "hybrid1", "hybrid2", "hybrid3", "matrix"};
  for (int f = 0; f < 5; ++f) CHECK(hipFuncSetAttribute((const void*)kern[f], hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
  std::vector<double> ref(2 * nspec), got(2 * nspec);
  std::vector<long long> t(ntr);
  const int nrun = 6;
  double means[5][nrun];
  if (js) fprintf(js, "{\n \"y_phase_ns\": {\n");
  for (int f = 0; f < 5; ++f) {               // results first: every form against the vector form
    CHECK(hipMemset(spec, 0, nspec * 16));
    kern[f]<<<grid, kZyBlock, sh, 0>>>(N, N, reinterpret_cast<Cx<double>*>(spec), t1, tr);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(f ? got.data() : ref.data(), spec, nspec * 16, hipMemcpyDeviceToHost));
    if (f) {
      double big = 0, diff = 0;
      for (size_t i = 0; i < ref.size(); ++i) { big = std::max(big, std::fabs(ref[i])); diff = std::max(diff, std::fabs(ref[i] - got[i])); }
      printf("%-8s against vector: largest difference %.3e of largest word %.3e (%.2e relative)\n", name[f], diff, big, diff / big);
    }
  }
  for (int run = 0; run < nrun; ++run)        // forms alternating
    for (int f = 0; f < 5; ++f) {
      hipEvent_t a, b; CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
      CHECK(hipEventRecord(a));
      kern[f]<<<grid, kZyBlock, sh, 0>>>(N, N, reinterpret_cast<Cx<double>*>(spec), t1, tr);
      CHECK(hipEventRecord(b));
      CHECK(hipDeviceSynchronize());
      float ms; CHECK(hipEventElapsedTime(&ms, a, b));
      CHECK(hipMemcpy(t.data(), tr, ntr * 8, hipMemcpyDeviceToHost));
      const Stat s = phase_stat(t, nx);
      means[f][run] = s.mean;
      printf("run %d %-8s phase mean %.0f ns (25 columns %.0f, 24 columns %.0f, slowest %.0f) | launch of %d phases %.1f us\n", run,
             name[f], s.mean, s.z0, s.z1, s.worst, kReps, ms * 1e3);
    }
  for (int f = 0; f < 5; ++f) {
    double lo = 1e30, hi = 0, sum = 0;
    for (int r = 1; r < nrun; ++r) { lo = std::min(lo, means[f][r]); hi = std::max(hi, means[f][r]); sum += means[f][r]; }
    printf("%-8s runs 1..%d: mean %.0f ns, range %.0f .. %.0f (spread %.0f)\n", name[f], nrun - 1, sum / (nrun - 1), lo, hi, hi - lo);
    if (js) {
      fprintf(js, "  \"%s\": [", name[f]);
      for (int r = 0; r < nrun; ++r) fprintf(js, "%s%.0f", r ? ", " : "", means[f][r]);
      fprintf(js, "]%s\n", f < 4 ? "," : "");
    }
  }
  if (js) fprintf(js, " },\n");

  // ---- part 2: the library's kernels
  CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_zy_trace), &tr, sizeof(tr)));
  {
    std::vector<double> h(nmesh);
    for (size_t i = 0; i < nmesh; ++i) h[i] = std::sin(0.37 * (double)i);
    CHECK(hipMemcpy(mesh, h.data(), nmesh * 8, hipMemcpyHostToDevice));
  }
  // sites of a 1024-water box for the spread form: positions uniform in a cube of 31.3 A, charges and dipoles of order one
  const int na = 3072;
  const double box = 31.3;
  std::vector<Site<double>> sites(na);
  unsigned long long seed = 12345;
  auto rnd = [&]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
  for (auto& s : sites) {
    s = Site<double>{};
    for (int d = 0; d < 3; ++d) s.r[d] = box * rnd();
    for (int q = 0; q < 9; ++q) s.Q[q] = rnd() - 0.5;
    for (int d = 0; d < 3; ++d) s.U[d] = 0.1 * (rnd() - 0.5);
  }
  Site<double>* dsites;
  CHECK(hipMalloc(&dsites, sizeof(Site<double>) * na));
  CHECK(hipMemcpy(dsites, sites.data(), sizeof(Site<double>) * na, hipMemcpyHostToDevice));
  PlaneSpread<double> sp;
  sp.na = na; sp.lpol = 1; sp.sites = dsites; sp.bases = nullptr;
  for (int d = 0; d < 3; ++d) sp.g.K[d] = N;
  for (int e = 0; e < 9; ++e) sp.g.hinv[e] = sp.g.Aop[e] = sp.g.Jac[e] = 0.0;
  for (int d = 0; d < 3; ++d) { sp.g.hinv[4 * d] = 1.0 / box; sp.g.Aop[4 * d] = -(double)N / box; sp.g.Jac[4 * d] = (double)N / box; }
  sp.g.whole_mesh();
  if (!dft_zy_spread_fits<double>(K, na)) { printf("the spread form does not fit\n"); return 1; }
  constexpr int NK = 6;
  const char* kname[NK] = {"k_dft_zy_fwd<double,2,false,false>", "k_dft_zy_fwd<double,2,false,true>", "k_dft_zy_fwd<double,2,true,false>",
                           "k_dft_zy_fwd<double,2,true,true>", "k_dft_yz_inv<double,2,false>", "k_dft_yz_inv<double,2,true>"};
  const char* pname[NK][4] = {{"load", "z lines", "pairing", "y lines + stores"}, {"load", "z lines", "pairing", "y lines + stores"},
                              {"spread", "z lines", "pairing", "y lines + stores"}, {"spread", "z lines", "pairing", "y lines + stores"},
                              {"load + pairing", "y lines", "z lines + stores", ""}, {"load + pairing", "y lines", "z lines + stores", ""}};
  const int np[NK] = {4, 4, 4, 4, 3, 3};
  if (js) fprintf(js, " \"kernel_phases_ns\": {\n");
  for (int kk = 0; kk < NK; ++kk) {
    setenv("ADMP_DFT_PLANE_MFMA", (kk & 1) ? "1" : "0", 1);
    double ph[4][nrun], ev[nrun];
    for (int run = 0; run < nrun; ++run) {
      hipEvent_t a, b; CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
      CHECK(hipEventRecord(a));
      launch_dft_zy<double>(0, K, twd, mesh, spec, kk >= 4, 1, 0, 0, nullptr, (kk == 2 || kk == 3) ? &sp : nullptr);
      CHECK(hipEventRecord(b));
      CHECK(hipDeviceSynchronize());
      float ms; CHECK(hipEventElapsedTime(&ms, a, b));
      ev[run] = ms * 1e3;
      CHECK(hipMemcpy(t.data(), tr, ntr * 8, hipMemcpyDeviceToHost));
      for (int p = 0; p < np[kk]; ++p) {
        ph[p][run] = 0;
        for (int b2 = 0; b2 < 2 * nx; ++b2) ph[p][run] += (double)(t[8 * b2 + p + 1] - t[8 * b2 + p]) * 10.0 / (2 * nx);
      }
    }
    printf("%s (with the stamps and their closing barrier), runs 1..%d:\n", kname[kk], nrun - 1);
    if (js) fprintf(js, "  \"%s\": {", kname[kk]);
    for (int p = 0; p < np[kk]; ++p) {
      double lo = 1e30, hi = 0, sum = 0;
      for (int r = 1; r < nrun; ++r) { lo = std::min(lo, ph[p][r]); hi = std::max(hi, ph[p][r]); sum += ph[p][r]; }
      printf("  %-18s mean %.0f ns, range %.0f .. %.0f\n", pname[kk][p], sum / (nrun - 1), lo, hi);
      if (js) fprintf(js, "\"%s\": %.0f, ", pname[kk][p], sum / (nrun - 1));
    }
    double sum = 0;
    for (int r = 1; r < nrun; ++r) sum += ev[r];
    printf("  %-18s mean %.1f us\n", "launch (events)", sum / (nrun - 1));
    if (js) fprintf(js, "\"launch_us\": %.1f}%s\n", sum / (nrun - 1), kk < NK - 1 ? "," : "");
  }
  if (js) { fprintf(js, " }\n}\n"); fclose(js); }
  return 0;
}
