// The FIRE energy minimiser of the MD drivers (admp_amd/md.py FireMinimizer; the rule is md_fire_math.h): one iteration is two
// kernels behind one C entry (admp_md_fire_step), its decision logic on the device, nothing read back.
//
//   k_md_fire_sums  grid-stride over the atoms, <= 256 workgroups of 256 lanes: every workgroup writes ONE row of the six words
//                   (Fv, FF, vv sums; vmax, fmax, amax maxima; all in double whatever T) to the handle's partials buffer.
//   k_md_fire_step  the same grid: every workgroup folds the rows in one fixed order (lane t holds row t, then the workgroup
//                   reduction of reduce.h), its lane 0 evaluates md_fire_control and hands the four coefficients to the other
//                   lanes through LDS, and the workgroup updates its atoms.  Workgroup 0, lane 0 writes the next state.
//
// No atomics anywhere: for a given n the rows, the fold and therefore positions, velocities and state are functions of the
// inputs alone, bit for bit.  The state is double-buffered by the caller's call counter (the step reads slot call & 1 and
// writes the other in full), so no workgroup reads a word another one writes and nothing waits for a last workgroup.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "md_fire_math.h"
#include "reduce.h"

namespace admp {

constexpr int kFireMaxRows = 256;      // one lane of k_md_fire_step per row
constexpr double kFireAcc = 1e-4;      // 1 kJ/mol/A/amu = 1e-4 A/fs^2 (admp_amd/md.py VelocityVerlet.ACC)

template <class T>
__global__ __launch_bounds__(256) void k_md_fire_sums(int n, const T* __restrict__ vel, const T* __restrict__ grad,
                                                      const T* __restrict__ inv_mass, double* __restrict__ rows) {
  double Fv = 0.0, FF = 0.0, vv = 0.0, vmax2 = 0.0, fmax2 = 0.0, amax = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double v[3] = {(double)vel[3 * i], (double)vel[3 * i + 1], (double)vel[3 * i + 2]};
    const double F[3] = {-(double)grad[3 * i], -(double)grad[3 * i + 1], -(double)grad[3 * i + 2]};
    const double f2 = F[0] * F[0] + F[1] * F[1] + F[2] * F[2], v2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    Fv += F[0] * v[0] + F[1] * v[1] + F[2] * v[2];
    FF += f2;
    vv += v2;
    vmax2 = fmax(vmax2, v2);
    fmax2 = fmax(fmax2, f2);
    amax = fmax(amax, kFireAcc * (double)inv_mass[i] * sqrt(f2));
  }
  Fv = block_reduce_sum<256>(Fv);
  FF = block_reduce_sum<256>(FF);
  vv = block_reduce_sum<256>(vv);
  vmax2 = block_reduce_max<256>(vmax2);
  fmax2 = block_reduce_max<256>(fmax2);
  amax = block_reduce_max<256>(amax);
  if (threadIdx.x == 0) {
    double* r = rows + (size_t)FIRE_SUM_WORDS * blockIdx.x;
    r[FIRE_S_FV] = Fv; r[FIRE_S_FF] = FF; r[FIRE_S_VV] = vv;
    r[FIRE_S_VMAX] = sqrt(vmax2); r[FIRE_S_FMAX] = sqrt(fmax2); r[FIRE_S_AMAX] = amax;
  }
}

struct FireArgs {
  double par[FIRE_PARAM_WORDS];
  double ftol;
};

template <class T>
__global__ __launch_bounds__(256) void k_md_fire_step(int n, T* __restrict__ pos, T* __restrict__ vel, const T* __restrict__ grad,
                                                      const T* __restrict__ inv_mass, const double* __restrict__ rows, int n_rows,
                                                      FireArgs args, const double* __restrict__ state_in,
                                                      double* __restrict__ state_out) {
  __shared__ double coef_s[4];
  __shared__ int move_s;
  double s[FIRE_SUM_WORDS];
#pragma unroll
  for (int w = 0; w < FIRE_SUM_WORDS; ++w) s[w] = (int)threadIdx.x < n_rows ? rows[FIRE_SUM_WORDS * threadIdx.x + w] : 0.0;
  s[FIRE_S_FV] = block_reduce_sum<256>(s[FIRE_S_FV]);
  s[FIRE_S_FF] = block_reduce_sum<256>(s[FIRE_S_FF]);
  s[FIRE_S_VV] = block_reduce_sum<256>(s[FIRE_S_VV]);
  s[FIRE_S_VMAX] = block_reduce_max<256>(s[FIRE_S_VMAX]);
  s[FIRE_S_FMAX] = block_reduce_max<256>(s[FIRE_S_FMAX]);
  s[FIRE_S_AMAX] = block_reduce_max<256>(s[FIRE_S_AMAX]);
  if (threadIdx.x == 0) {
    double in[FIRE_STATE_WORDS], out[FIRE_STATE_WORDS], coef[4];
#pragma unroll
    for (int w = 0; w < FIRE_STATE_WORDS; ++w) in[w] = state_in[w];
    move_s = md_fire_control(in, s, args.par, args.ftol, out, coef);
#pragma unroll
    for (int w = 0; w < 4; ++w) coef_s[w] = coef[w];
    if (blockIdx.x == 0)
#pragma unroll
      for (int w = 0; w < FIRE_STATE_WORDS; ++w) state_out[w] = out[w];
  }
  __syncthreads();
  if (!move_s) return;
  const T a = (T)coef_s[0], b = (T)coef_s[1], back = (T)coef_s[2], dtv = (T)coef_s[3];      // rounded to T once
  const T acc = (T)kFireAcc;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const T dtw = dtv * (acc * inv_mass[i]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const T F = -grad[3 * i + c];
      T v = vel[3 * i + c];
      T x = pos[3 * i + c] - back * v;
      v = a * v + b * F;
      v += dtw * F;
      x += dtv * v;
      vel[3 * i + c] = v;
      pos[3 * i + c] = x;
    }
  }
}

// rows: at least 256 * 6 doubles.  state16: two slots of 8 doubles; reads slot call & 1, writes slot (call + 1) & 1.  n = 0:
// no launch, the slot is copied forward on the stream.  Returns hipError_t as int.
template <class T>
int launch_md_fire(hipStream_t st, int n, T* pos, T* vel, const T* grad, const T* inv_mass, const double* par9, double ftol,
                   uint64_t call, double* rows, double* state16) {
  const double* in = state16 + FIRE_STATE_WORDS * (call & 1u);
  double* out = state16 + FIRE_STATE_WORDS * ((call + 1u) & 1u);
  if (n <= 0) return (int)hipMemcpyAsync(out, in, FIRE_STATE_WORDS * sizeof(double), hipMemcpyDeviceToDevice, st);
  int blocks = (n + 255) / 256;
  if (blocks > kFireMaxRows) blocks = kFireMaxRows;
  FireArgs args;
  for (int w = 0; w < FIRE_PARAM_WORDS; ++w) args.par[w] = par9[w];
  args.ftol = ftol;
  k_md_fire_sums<T><<<blocks, 256, 0, st>>>(n, vel, grad, inv_mass, rows);
  k_md_fire_step<T><<<blocks, 256, 0, st>>>(n, pos, vel, grad, inv_mass, rows, blocks, args, in, out);
  return (int)hipGetLastError();
}
template int launch_md_fire<float>(hipStream_t, int, float*, float*, const float*, const float*, const double*, double, uint64_t,
                                   double*, double*);
template int launch_md_fire<double>(hipStream_t, int, double*, double*, const double*, const double*, const double*, double,
                                    uint64_t, double*, double*);

}  // namespace admp
