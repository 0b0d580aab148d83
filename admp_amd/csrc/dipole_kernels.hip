// The dipole observable (include/admp_hip.h admp_pme_dipoles; the arithmetic is dipole_math.h): molecular dipoles and the cell
// dipole, split into their charge, permanent and induced parts.  One call is two kernels, nothing read back.
//
//   k_dipole_groups  one lane per group, 256 lanes a workgroup.  The lane walks its group's atoms in list order -- the atoms
//                    come from a CSR pair (group_start, group_atoms), the anchor first -- so a group has no size cap and the
//                    kernel no LDS plan.  Frames and minimum images in T, every product and sum in double.  The lane writes
//                    mu_c (3 doubles) when asked, and every workgroup writes ONE row of kDipoleRowWords partial sums.
//   k_dipole_fold    one workgroup: lane t adds rows t, t + 256, ... in that order, then the workgroup reduction of reduce.h,
//                    and lane 0 writes the 16 words.
//
// No atomics: for given inputs the rows, the fold and so the 16 words are the same bit for bit from run to run (the scheme of
// fire_kernels.hip and vrescale_kernels.hip).  Gather-bound and small: the CSR reads are coalesced and nothing else is tuned.
#include <hip/hip_runtime.h>

#include "dipole_math.h"
#include "launch.h"
#include "reduce.h"

namespace admp {

constexpr int kDipBlock = 256;

template <class T>
__global__ __launch_bounds__(kDipBlock) void k_dipole_groups(Topology top, const T* __restrict__ pos, Box<T> box,
                                                             const T* __restrict__ Ql, const T* __restrict__ U,
                                                             const T* __restrict__ inv_mass, int n_groups,
                                                             const int* __restrict__ group_start,
                                                             const int* __restrict__ group_atoms, double* __restrict__ mu_groups,
                                                             double* __restrict__ rows) {
  const int g = blockIdx.x * kDipBlock + threadIdx.x;
  double w[kDipoleRowWords];
#pragma unroll
  for (int k = 0; k < kDipoleRowWords; ++k) w[k] = 0.0;
  if (g < n_groups) {
    int a0 = group_start[g], a1 = group_start[g + 1];
    if (a0 < 0 || a1 > top.na || a1 < a0) a0 = a1 = 0;      // a list the caller did not check: an empty group
    dipole_group<T>(top.axis_type, top.axis_idx, top.na, pos, box, Ql, U, inv_mass, group_atoms + a0, a1 - a0, w);
    double mu[3];
    const double len = dipole_total(w, mu);
    if (mu_groups) { mu_groups[3 * (size_t)g] = mu[0]; mu_groups[3 * (size_t)g + 1] = mu[1]; mu_groups[3 * (size_t)g + 2] = mu[2]; }
    w[9] = len;
    w[10] = mu[0] * mu[0] + mu[1] * mu[1] + mu[2] * mu[2];
    w[11] = len;
  }
#pragma unroll
  for (int k = 0; k < kDipoleRowWords; ++k) {
    const double r = k < kDipoleSumWords ? block_reduce_sum<kDipBlock>(w[k]) : block_reduce_max<kDipBlock>(w[k]);
    if (threadIdx.x == 0) rows[(size_t)blockIdx.x * kDipoleRowWords + k] = r;
  }
}

__global__ __launch_bounds__(kDipBlock) void k_dipole_fold(const double* __restrict__ rows, int n_rows, int n_groups,
                                                           double* __restrict__ out16) {
  double w[kDipoleRowWords];
#pragma unroll
  for (int k = 0; k < kDipoleRowWords; ++k) w[k] = 0.0;
  for (int r = threadIdx.x; r < n_rows; r += kDipBlock)
#pragma unroll
    for (int k = 0; k < kDipoleRowWords; ++k) {
      const double v = rows[(size_t)r * kDipoleRowWords + k];
      w[k] = k < kDipoleSumWords ? w[k] + v : fmax(w[k], v);
    }
#pragma unroll
  for (int k = 0; k < kDipoleRowWords; ++k) {
    const double r = k < kDipoleSumWords ? block_reduce_sum<kDipBlock>(w[k]) : block_reduce_max<kDipBlock>(w[k]);
    if (threadIdx.x == 0) out16[k] = r;
  }
  if (threadIdx.x == 0) {
    out16[kDipoleRowWords] = (double)n_groups;
#pragma unroll
    for (int k = kDipoleRowWords + 1; k < kDipoleOutWords; ++k) out16[k] = 0.0;
  }
}

int dipole_rows(int n_groups) { return (n_groups + kDipBlock - 1) / kDipBlock; }

// rows: dipole_rows(n_groups) * kDipoleRowWords doubles.  n_groups = 0: no launch, out16 zeroed on the stream.  Returns
// hipError_t as int.
template <class T>
int launch_dipoles(hipStream_t st, const Topology& top, const T* pos, const Box<T>& box, const T* Ql, const T* U, const T* inv_mass,
                   int n_groups, const int* group_start, const int* group_atoms, double* mu_groups, double* rows, double* out16) {
  if (n_groups <= 0) return (int)hipMemsetAsync(out16, 0, kDipoleOutWords * sizeof(double), st);
  const int blocks = dipole_rows(n_groups);
  k_dipole_groups<T><<<blocks, kDipBlock, 0, st>>>(top, pos, box, Ql, U, inv_mass, n_groups, group_start, group_atoms, mu_groups, rows);
  k_dipole_fold<<<1, kDipBlock, 0, st>>>(rows, blocks, n_groups, out16);
  return (int)hipGetLastError();
}
template int launch_dipoles<float>(hipStream_t, const Topology&, const float*, const Box<float>&, const float*, const float*,
                                   const float*, int, const int*, const int*, double*, double*, double*);
template int launch_dipoles<double>(hipStream_t, const Topology&, const double*, const Box<double>&, const double*, const double*,
                                    const double*, int, const int*, const int*, double*, double*, double*);

}  // namespace admp
