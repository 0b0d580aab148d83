// MD-driver kernels (the reference has no integrator): the harmonic bonded terms of the drivers' force
// field (examples/*/mpidwater.xml:16-21, OpenMM's HarmonicBondForce / HarmonicAngleForce: E = k/2 (r - r0)^2, k/2 (theta -
// theta0)^2) as ONE kernel over explicit bond / angle lists, and the two half steps of velocity Verlet as one elementwise
// kernel each.  Round 3's driver did this with ~60 torch launches per step (autograd through acos / norm, elementwise updates).
// The Langevin thermostat is one more elementwise kernel: the first half of a BAOAB step with its noise drawn in registers
// from the counter-based generator of md_math.h (k_md_random writes the same words / normals to memory for the callers that
// want them: the tests and the Maxwell-Boltzmann start of admp_amd/md.py).
// The isotropic barostat (stochastic cell rescaling, admp_amd/md.py CRescaleBarostat) adds three: the box-gradient pass of
// the bonded terms, the two 3x3 sums a pressure needs with the barostat's normal in the same launch, and the rescaling.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "md_math.h"
#include "reduce.h"

namespace admp {

// items 0 .. nb-1: bonds (i, j; k, r0); items nb .. nb+na-1: angles (i, centre j, k; k_theta, theta0).  grad is ADDED to
// (hardware float atomics: two or three atoms per item); E[0] += bond energy, E[1] += angle energy.
template <class T>
__global__ __launch_bounds__(256) void k_md_bonded(int nb, const int* __restrict__ bidx, const T* __restrict__ bpar, int na,
                                                   const int* __restrict__ aidx, const T* __restrict__ apar,
                                                   const T* __restrict__ pos, Box<T> box, T* __restrict__ grad, double* E) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  double eb = 0.0, ea = 0.0;
  if (t < nb) {
    const int i = bidx[2 * t], j = bidx[2 * t + 1];
    T d[3] = {pos[3 * j] - pos[3 * i], pos[3 * j + 1] - pos[3 * i + 1], pos[3 * j + 2] - pos[3 * i + 2]};
    min_image(box, d);
    const T r = m_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const T k = bpar[2 * t], dr = r - bpar[2 * t + 1];
    eb = 0.5 * (double)k * (double)dr * (double)dr;
    const T s = k * dr / r;                      // dE/dr / r
#pragma unroll
    for (int c = 0; c < 3; ++c) { atomicAdd(&grad[3 * j + c], s * d[c]); atomicAdd(&grad[3 * i + c], -s * d[c]); }
  } else if (t < nb + na) {
    const int a = t - nb;
    const int i = aidx[3 * a], j = aidx[3 * a + 1], k3 = aidx[3 * a + 2];
    T u[3] = {pos[3 * i] - pos[3 * j], pos[3 * i + 1] - pos[3 * j + 1], pos[3 * i + 2] - pos[3 * j + 2]};
    T v[3] = {pos[3 * k3] - pos[3 * j], pos[3 * k3 + 1] - pos[3 * j + 1], pos[3 * k3 + 2] - pos[3 * j + 2]};
    min_image(box, u);
    min_image(box, v);
    const T ru = m_sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), rv = m_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    T c = (u[0] * v[0] + u[1] * v[1] + u[2] * v[2]) / (ru * rv);
    c = c > T(1) ? T(1) : (c < T(-1) ? T(-1) : c);
    const T th = (T)acos((double)c), kt = apar[2 * a], dth = th - apar[2 * a + 1];
    ea = 0.5 * (double)kt * (double)dth * (double)dth;
    // d theta / d u = -(v / (ru rv) - c u / ru^2) / sin theta
    T sn = m_sqrt(T(1) - c * c);
    sn = sn < T(1e-8) ? T(1e-8) : sn;
    const T f = -kt * dth / sn;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const T gu = f * (v[q] / (ru * rv) - c * u[q] / (ru * ru)), gv = f * (u[q] / (ru * rv) - c * v[q] / (rv * rv));
      atomicAdd(&grad[3 * i + q], gu);
      atomicAdd(&grad[3 * k3 + q], gv);
      atomicAdd(&grad[3 * j + q], -(gu + gv));
    }
  }
  eb = block_reduce_sum<256>(eb);
  ea = block_reduce_sum<256>(ea);
  if (threadIdx.x == 0) {
    if (eb != 0.0) atomicAdd(&E[0], eb);
    if (ea != 0.0) atomicAdd(&E[1], ea);
  }
}

// Box-gradient pass of k_md_bonded (same item layout): for every bond and angle vector, shift = d_min - d_raw, the lattice
// translation min_image applied (image_shift: -n . box with integer n, exactly zero for a vector inside the cell), and
// S[3 c + b] += shift_c dE/dd_b.  dE/dbox = box^-T S at fixed Cartesian positions is formed by the caller (pme_math.h
// image_shift: d(d_min)/d(box[a][b]) = -n_a e_b).  E[0] += bond energy, E[1] += angle energy as in k_md_bonded; no gradient
// is written.  Products and sums in double; one atomic per word and workgroup.
template <class T>
__global__ __launch_bounds__(256) void k_md_bonded_box(int nb, const int* __restrict__ bidx, const T* __restrict__ bpar, int na,
                                                       const int* __restrict__ aidx, const T* __restrict__ apar,
                                                       const T* __restrict__ pos, Box<T> box, double* E, double* S) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  double eb = 0.0, ea = 0.0, s9[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < nb) {
    const int i = bidx[2 * t], j = bidx[2 * t + 1];
    T d[3] = {pos[3 * j] - pos[3 * i], pos[3 * j + 1] - pos[3 * i + 1], pos[3 * j + 2] - pos[3 * i + 2]};
    T sh[3];
    const bool crosses = image_shift(box, d, sh);
    min_image(box, d);
    const T r = m_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const T k = bpar[2 * t], dr = r - bpar[2 * t + 1];
    eb = 0.5 * (double)k * (double)dr * (double)dr;
    const T s = k * dr / r;                      // dE/dd = s d
    if (crosses)
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int b = 0; b < 3; ++b) s9[3 * c + b] -= (double)sh[c] * (double)(s * d[b]);
  } else if (t < nb + na) {
    const int a = t - nb;
    const int i = aidx[3 * a], j = aidx[3 * a + 1], k3 = aidx[3 * a + 2];
    T u[3] = {pos[3 * i] - pos[3 * j], pos[3 * i + 1] - pos[3 * j + 1], pos[3 * i + 2] - pos[3 * j + 2]};
    T v[3] = {pos[3 * k3] - pos[3 * j], pos[3 * k3 + 1] - pos[3 * j + 1], pos[3 * k3 + 2] - pos[3 * j + 2]};
    T shu[3], shv[3];
    const bool cu = image_shift(box, u, shu), cv = image_shift(box, v, shv);
    min_image(box, u);
    min_image(box, v);
    const T ru = m_sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), rv = m_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    T c = (u[0] * v[0] + u[1] * v[1] + u[2] * v[2]) / (ru * rv);
    c = c > T(1) ? T(1) : (c < T(-1) ? T(-1) : c);
    const T th = (T)acos((double)c), kt = apar[2 * a], dth = th - apar[2 * a + 1];
    ea = 0.5 * (double)kt * (double)dth * (double)dth;
    T sn = m_sqrt(T(1) - c * c);
    sn = sn < T(1e-8) ? T(1e-8) : sn;
    const T f = -kt * dth / sn;
    if (cu || cv)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const T gu = f * (v[q] / (ru * rv) - c * u[q] / (ru * ru)), gv = f * (u[q] / (ru * rv) - c * v[q] / (rv * rv));
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          if (cu) s9[3 * p + q] -= (double)shu[p] * (double)gu;
          if (cv) s9[3 * p + q] -= (double)shv[p] * (double)gv;
        }
      }
  }
  eb = block_reduce_sum<256>(eb);
  ea = block_reduce_sum<256>(ea);
#pragma unroll
  for (int w = 0; w < 9; ++w) s9[w] = block_reduce_sum<256>(s9[w]);
  if (threadIdx.x == 0) {
    if (eb != 0.0) atomicAdd(&E[0], eb);
    if (ea != 0.0) atomicAdd(&E[1], ea);
#pragma unroll
    for (int w = 0; w < 9; ++w)
      if (s9[w] != 0.0) atomicAdd(&S[w], s9[w]);
  }
}

// v -= half_dt_acc grad / m (grad = +dE/dr); then, if dt != 0, r += dt v; ekin (optional) += sum m v^2 / 2 AFTER the kick
template <class T>
__global__ __launch_bounds__(256) void k_md_kick_drift(int n, T* __restrict__ pos, T* __restrict__ vel, const T* __restrict__ grad,
                                                       const T* __restrict__ inv_mass, T half_dt_acc, T dt, double* ekin) {
  double ek = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const T im = inv_mass[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const T v = vel[3 * i + c] - half_dt_acc * grad[3 * i + c] * im;
      vel[3 * i + c] = v;
      if (dt != T(0)) pos[3 * i + c] += dt * v;
      ek += 0.5 * (double)v * (double)v / (double)im;
    }
  }
  if (ekin) {
    ek = block_reduce_sum<256>(ek);
    if (threadIdx.x == 0) atomicAdd(ekin, ek);
  }
}

// First half of a BAOAB Langevin step (Leimkuhler, Matthews 2013), one pass: B v -= half_dt_acc grad / m; A r += half_dt v;
// O v = c1 v + sqrt(c2sq_kT_acc / m) xi; A r += half_dt v.  xi: three normals of (seed, step, stream 0, atom), computed in
// double and rounded to T.  ekin (optional) += sum m v^2 / 2 after O.  The second half is k_md_kick_drift with dt = 0.
template <class T>
__global__ __launch_bounds__(256) void k_md_langevin(int n, T* __restrict__ pos, T* __restrict__ vel, const T* __restrict__ grad,
                                                     const T* __restrict__ inv_mass, T half_dt_acc, T half_dt, T c1, T c2sq_kT_acc,
                                                     uint64_t seed, uint64_t step, double* ekin) {
  double ek = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const T im = inv_mass[i], sig = m_sqrt(c2sq_kT_acc * im);
    double xi[3];
    md_random_normals(seed, step, kStreamLangevin, (uint32_t)i, xi);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T v = vel[3 * i + c] - half_dt_acc * grad[3 * i + c] * im;
      T r = pos[3 * i + c] + half_dt * v;
      v = c1 * v + sig * (T)xi[c];
      r += half_dt * v;
      vel[3 * i + c] = v;
      pos[3 * i + c] = r;
      ek += 0.5 * (double)v * (double)v / (double)im;
    }
  }
  if (ekin) {
    ek = block_reduce_sum<256>(ek);
    if (threadIdx.x == 0) atomicAdd(ekin, ek);
  }
}

// What one barostat application reads from the device, in one pass: out[0..8] += sum_i v_i (x) v_i / inv_mass_i, out[9..17] +=
// sum_i r_i (x) g_i (row-major, the first factor's component first; the caller zeroes the 18 words), out[18..20] = the three
// normals of (seed, step, stream 2, atom 0), written by one lane.  Products and sums in double whatever T.
template <class T>
__global__ __launch_bounds__(256) void k_md_virial(int n, const T* __restrict__ pos, const T* __restrict__ vel,
                                                   const T* __restrict__ grad, const T* __restrict__ inv_mass, uint64_t seed,
                                                   uint64_t step, double* __restrict__ out) {
  double acc[18];
#pragma unroll
  for (int w = 0; w < 18; ++w) acc[w] = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double m = 1.0 / (double)inv_mass[i];
    const double v[3] = {(double)vel[3 * i], (double)vel[3 * i + 1], (double)vel[3 * i + 2]};
    const double r[3] = {(double)pos[3 * i], (double)pos[3 * i + 1], (double)pos[3 * i + 2]};
    const double g[3] = {(double)grad[3 * i], (double)grad[3 * i + 1], (double)grad[3 * i + 2]};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        acc[3 * a + b] += v[a] * v[b] * m;
        acc[9 + 3 * a + b] += r[a] * g[b];
      }
  }
#pragma unroll
  for (int w = 0; w < 18; ++w) acc[w] = block_reduce_sum<256>(acc[w]);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < 18; ++w)
      if (acc[w] != 0.0) atomicAdd(&out[w], acc[w]);
    if (blockIdx.x == 0) {
      double xi[3];
      md_random_normals(seed, step, kStreamBarostat, 0u, xi);
      out[18] = xi[0]; out[19] = xi[1]; out[20] = xi[2];
    }
  }
}

// isotropic rescaling: r *= mu, v *= inv_mu (both factors from the host in double, rounded to T once)
template <class T>
__global__ __launch_bounds__(256) void k_md_scale(int n3, T* __restrict__ pos, T* __restrict__ vel, T mu, T inv_mu) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n3; i += gridDim.x * 256) {
    pos[i] *= mu;
    vel[i] *= inv_mu;
  }
}

// kind 0: out (n,4) uint32 = the words of (seed, step, stream, atom); kind 1: out (n,3) T = the normals
template <class T>
__global__ __launch_bounds__(256) void k_md_random(int kind, int64_t n, uint64_t seed, uint64_t step, uint32_t stream,
                                                   void* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (kind == 0) {
      uint32_t w[4];
      md_random_words(seed, step, stream, (uint32_t)i, w);
      uint32_t* o = reinterpret_cast<uint32_t*>(out) + 4 * i;
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = w[c];
    } else {
      double xi[3];
      md_random_normals(seed, step, stream, (uint32_t)i, xi);
      T* o = reinterpret_cast<T*>(out) + 3 * i;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (T)xi[c];
    }
  }
}

template <class T>
void launch_md_bonded(hipStream_t st, int nb, const int* bidx, const T* bpar, int na, const int* aidx, const T* apar, const T* pos,
                      const Box<T>& box, T* grad, double* E) {
  const int n = nb + na;
  if (n > 0) k_md_bonded<T><<<(n + 255) / 256, 256, 0, st>>>(nb, bidx, bpar, na, aidx, apar, pos, box, grad, E);
}
template <class T>
void launch_md_kick_drift(hipStream_t st, int n, T* pos, T* vel, const T* grad, const T* inv_mass, double half_dt_acc, double dt,
                          double* ekin) {
  if (n <= 0) return;
  int blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;      // (<= 1024 atomics on the kinetic-energy word)
  k_md_kick_drift<T><<<blocks, 256, 0, st>>>(n, pos, vel, grad, inv_mass, (T)half_dt_acc, (T)dt, ekin);
}
template <class T>
void launch_md_langevin(hipStream_t st, int n, T* pos, T* vel, const T* grad, const T* inv_mass, double half_dt_acc, double dt,
                        double c1, double c2sq_kT_acc, uint64_t seed, uint64_t step, double* ekin) {
  if (n <= 0) return;
  int blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  k_md_langevin<T><<<blocks, 256, 0, st>>>(n, pos, vel, grad, inv_mass, (T)half_dt_acc, (T)(0.5 * dt), (T)c1, (T)c2sq_kT_acc, seed,
                                           step, ekin);
}
template <class T>
void launch_md_random(hipStream_t st, int kind, int64_t n, uint64_t seed, uint64_t step, uint32_t stream, void* out) {
  if (n <= 0) return;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  k_md_random<T><<<(int)blocks, 256, 0, st>>>(kind, n, seed, step, stream, out);
}
template <class T>
void launch_md_bonded_box(hipStream_t st, int nb, const int* bidx, const T* bpar, int na, const int* aidx, const T* apar,
                          const T* pos, const Box<T>& box, double* E, double* S) {
  const int n = nb + na;
  if (n > 0) k_md_bonded_box<T><<<(n + 255) / 256, 256, 0, st>>>(nb, bidx, bpar, na, aidx, apar, pos, box, E, S);
}
// (one workgroup even for n = 0: the normals are written whatever n)
template <class T>
void launch_md_virial(hipStream_t st, int n, const T* pos, const T* vel, const T* grad, const T* inv_mass, uint64_t seed,
                      uint64_t step, double* out) {
  int blocks = n > 0 ? (n + 255) / 256 : 1;
  if (blocks > 1024) blocks = 1024;      // (<= 1024 atomics on each of the 18 words)
  k_md_virial<T><<<blocks, 256, 0, st>>>(n, pos, vel, grad, inv_mass, seed, step, out);
}
template <class T>
void launch_md_scale(hipStream_t st, int n, T* pos, T* vel, double mu, double inv_mu) {
  if (n <= 0) return;
  int blocks = (3 * n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  k_md_scale<T><<<blocks, 256, 0, st>>>(3 * n, pos, vel, (T)mu, (T)inv_mu);
}
#define INST(T)                                                                                                              \
  template void launch_md_bonded<T>(hipStream_t, int, const int*, const T*, int, const int*, const T*, const T*, const Box<T>&, \
                                    T*, double*);                                                                            \
  template void launch_md_kick_drift<T>(hipStream_t, int, T*, T*, const T*, const T*, double, double, double*);             \
  template void launch_md_langevin<T>(hipStream_t, int, T*, T*, const T*, const T*, double, double, double, double, uint64_t,  \
                                      uint64_t, double*);                                                                      \
  template void launch_md_random<T>(hipStream_t, int, int64_t, uint64_t, uint64_t, uint32_t, void*);                       \
  template void launch_md_bonded_box<T>(hipStream_t, int, const int*, const T*, int, const int*, const T*, const T*,           \
                                        const Box<T>&, double*, double*);                                                      \
  template void launch_md_virial<T>(hipStream_t, int, const T*, const T*, const T*, const T*, uint64_t, uint64_t, double*);    \
  template void launch_md_scale<T>(hipStream_t, int, T*, T*, double, double);
INST(float)
INST(double)
#undef INST

}  // namespace admp
