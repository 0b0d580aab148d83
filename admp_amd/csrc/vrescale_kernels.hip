// The stochastic velocity-rescaling thermostat of the MD drivers (admp_amd/md.py VRescale; the rule is md_vrescale_math.h): one
// application is two kernels behind one C entry (admp_md_vrescale), its draw and its decision on the device, nothing read back.
//
//   k_md_vr_sums   grid-stride over the atoms, <= 256 workgroups of 256 lanes.  With a gradient it first makes the closing half
//                  kick of the step on its atoms -- the expression of k_md_kick_drift (md_kernels.hip) with dt = 0, in T, so that
//                  the stored velocities are that kernel's bit for bit -- and then every workgroup writes ONE double, its share
//                  of sum v^2 / inv_mass / 2 over the stored velocities, to the driver's rows buffer.
//   k_md_vr_scale  the same grid: every workgroup folds the rows in one fixed order (lane t holds row t, then the workgroup
//                  reduction of reduce.h), its lane 0 evaluates md_vrescale_rule -- the gamma deviate's rejection loop included,
//                  once per workgroup, redundantly -- and hands (T)alpha to the other lanes through LDS, and the workgroup
//                  multiplies its velocities by it.  Workgroup 0, lane 0 writes the next state.
//
// No atomics anywhere: for a given n the rows, the fold and therefore velocities and state are functions of the inputs alone,
// bit for bit.  The state is double-buffered by the caller's call counter (an application reads slot call & 1 and writes the
// other in full), so no workgroup reads a word another one writes and nothing waits for a last workgroup.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "md_vrescale_math.h"
#include "reduce.h"

namespace admp {

constexpr int kVrMaxRows = 256;      // one lane of k_md_vr_scale per row

constexpr int kVrBatch = 4;          // atoms (sums) or words (scale) a lane loads before it computes: a grid of <= 256 workgroups
                                     // has four waves per CU, so the loads in flight have to come from each lane

// the closing half kick of one atom, in the expression of k_md_kick_drift (md_kernels.hip), and its share of sum v^2 / inv_mass / 2
template <class T>
__device__ __forceinline__ double vr_kick_atom(T* __restrict__ vel, int i, T v[3], const T g[3], T im, T half_dt_acc, bool kick) {
  double ek = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (kick) {
      v[c] = v[c] - half_dt_acc * g[c] * im;
      vel[3 * i + c] = v[c];
    }
    ek += 0.5 * (double)v[c] * (double)v[c] / (double)im;
  }
  return ek;
}

template <class T>
__global__ __launch_bounds__(256) void k_md_vr_sums(int n, T* __restrict__ vel, const T* __restrict__ grad,
                                                    const T* __restrict__ inv_mass, T half_dt_acc, double* __restrict__ rows) {
  const int stride = gridDim.x * 256;
  const bool kick = grad != nullptr;
  double ek = 0.0;
  int i = blockIdx.x * 256 + threadIdx.x;
  for (; (long)i + (long)(kVrBatch - 1) * stride < n; i += kVrBatch * stride) {
    T im[kVrBatch], v[kVrBatch][3], g[kVrBatch][3];
#pragma unroll
    for (int u = 0; u < kVrBatch; ++u) {
      const int j = i + u * stride;
      im[u] = inv_mass[j];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[u][c] = vel[3 * j + c];
        g[u][c] = kick ? grad[3 * j + c] : T(0);
      }
    }
#pragma unroll
    for (int u = 0; u < kVrBatch; ++u) ek += vr_kick_atom<T>(vel, i + u * stride, v[u], g[u], im[u], half_dt_acc, kick);
  }
  for (; i < n; i += stride) {
    const T im = inv_mass[i];
    T v[3], g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c] = vel[3 * i + c];
      g[c] = kick ? grad[3 * i + c] : T(0);
    }
    ek += vr_kick_atom<T>(vel, i, v, g, im, half_dt_acc, kick);
  }
  ek = block_reduce_sum<256>(ek);
  if (threadIdx.x == 0) rows[blockIdx.x] = ek;
}

struct VrArgs {
  int64_t n_dof;
  double kT_acc, c;
  uint64_t seed, step;
};

template <class T>
__global__ __launch_bounds__(256) void k_md_vr_scale(int n3, T* __restrict__ vel, const double* __restrict__ rows, int n_rows,
                                                     VrArgs args, const double* __restrict__ state_in,
                                                     double* __restrict__ state_out) {
  __shared__ double alpha_s;
  __shared__ int scale_s;
  const double K = block_reduce_sum<256>((int)threadIdx.x < n_rows ? rows[threadIdx.x] : 0.0);
  if (threadIdx.x == 0) {
    double in[VR_STATE_WORDS], out[VR_STATE_WORDS];
#pragma unroll
    for (int w = 0; w < VR_STATE_WORDS; ++w) in[w] = state_in[w];
    int scale;
    alpha_s = md_vrescale_rule<T>(in, K, args.n_dof, args.kT_acc, args.c, args.seed, args.step, out, &scale);
    scale_s = scale;
    if (blockIdx.x == 0)
#pragma unroll
      for (int w = 0; w < VR_STATE_WORDS; ++w) state_out[w] = out[w];
  }
  __syncthreads();
  if (!scale_s) return;
  const T a = (T)alpha_s;      // rounded to T once
  if (a == T(1)) return;       // (c = 1, K = 0: the velocities are the sums kernel's)
  const int stride = gridDim.x * 256;
  int i = blockIdx.x * 256 + threadIdx.x;
  for (; (long)i + (long)(kVrBatch - 1) * stride < n3; i += kVrBatch * stride) {
    T v[kVrBatch];
#pragma unroll
    for (int u = 0; u < kVrBatch; ++u) v[u] = vel[i + u * stride];
#pragma unroll
    for (int u = 0; u < kVrBatch; ++u) vel[i + u * stride] = v[u] * a;
  }
  for (; i < n3; i += stride) vel[i] *= a;
}

// rows: at least kVrRowsBytes.  state16: two slots of 8 doubles; reads slot call & 1, writes slot (call + 1) & 1.  n = 0: no
// launch, the slot is copied forward on the stream.  n <= INT_MAX / 4 is the caller's to check.  Returns hipError_t as int.
template <class T>
int launch_md_vrescale(hipStream_t st, int n, T* vel, const T* grad, const T* inv_mass, double half_dt_acc, int64_t n_dof,
                       double kT_acc, double c, uint64_t seed, uint64_t step, uint64_t call, double* rows, double* state16) {
  const double* in = state16 + VR_STATE_WORDS * (call & 1u);
  double* out = state16 + VR_STATE_WORDS * ((call + 1u) & 1u);
  if (n <= 0) return (int)hipMemcpyAsync(out, in, VR_STATE_WORDS * sizeof(double), hipMemcpyDeviceToDevice, st);
  int blocks = (n + 255) / 256;
  if (blocks > kVrMaxRows) blocks = kVrMaxRows;
  const VrArgs args{n_dof, kT_acc, c, seed, step};
  k_md_vr_sums<T><<<blocks, 256, 0, st>>>(n, vel, grad, inv_mass, (T)half_dt_acc, rows);
  k_md_vr_scale<T><<<blocks, 256, 0, st>>>(3 * n, vel, rows, blocks, args, in, out);
  return (int)hipGetLastError();
}
template int launch_md_vrescale<float>(hipStream_t, int, float*, const float*, const float*, double, int64_t, double, double,
                                       uint64_t, uint64_t, uint64_t, double*, double*);
template int launch_md_vrescale<double>(hipStream_t, int, double*, const double*, const double*, double, int64_t, double, double,
                                        uint64_t, uint64_t, uint64_t, double*, double*);

}  // namespace admp
