// Radial distribution functions (include/admp_hip.h admp_md_rdf; the arithmetic is rdf_math.h, the plan rdf_plan.h): the typed
// pair-distance counts of one frame, ADDED to a caller-owned histogram of 64-bit counters, channels x n_bins.
//
// Both forms keep the histogram as 32-bit counters in LDS, add to it with LDS integer atomics whose result is not used (the
// non-returning ds_add_u32), and at the end add only their non-zero counters to the global histogram with 64-bit integer
// atomicAdd.  Integers only, no float atomics: the counts do not depend on the order of anything, so a result is the same bit
// for bit from run to run and from form to form wherever the same pairs fall into the same bins.
//
//   k_rdf_tiles  one workgroup per pair (I <= J) of tiles of kRdfTile atoms.  Both tiles' positions and tags are staged in LDS;
//                lane i holds atom i of tile I and walks tile J from LDS, every lane at the same j: a broadcast read.  On the
//                diagonal (I = J) only j > i counts.
//   k_rdf_cells  one workgroup per home cell of a grid of cell width >= r_max, the atoms binned and their records packed cell by
//                cell by cell_bin_pack (cell_kernels.hip: the binning of the table builders without their sort inside a cell,
//                which integer counts do not need).  The half sweep of rdf_math.h: the home cell once (slot j > slot i) and, of
//                every pair of neighbouring cells, the visit whose first non-zero sign is positive.  A neighbour cell is staged
//                through LDS in chunks of kRdfChunk records; a cell holding more loops.  A home cell of nh atoms gives the
//                lanes as 256 / H2 groups of H2 = 2^ceil(log2 nh) <= 256 lanes: lane l of group g holds home atom l and takes
//                the staged atoms g, g + 256 / H2, ...; a home cell above 256 atoms takes several passes.
//
// No LDS counter can wrap before it is flushed.  A counter grows by at most one per pair test.  k_rdf_tiles tests at most
// 256 x 256 = 2^16 pairs per workgroup and flushes once.  k_rdf_cells tests at most H2 x kRdfChunk <= 2^16 pairs per staged
// chunk, counts the chunks, and flushes (and zeroes) after kRdfFlushChunks = 65535 of them: at most 65535 x 2^16 = 2^32 - 2^16
// increments between two flushes.
//
// Contention: in water the lanes of a workgroup meet in the few bins under the first peak.  A histogram per wave (four of them,
// summed by the flush) was measured against the single one and gave nothing -- 88.6 against 88.2 us at 3072 atoms, 3.82 against
// 3.85 ms at 98 304 -- so there is one histogram per workgroup.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "rdf_plan.h"

namespace admp {

constexpr unsigned kRdfFlushChunks = 65535u;
static_assert(kRdfTile == 256 && kRdfChunk == 256, "one staged atom per lane");

extern __shared__ double rdf_lds[];      // (8-byte aligned: reals, then tags, then counters)

__device__ __forceinline__ void rdf_count(unsigned* hist, int k) {
  (void)__hip_atomic_fetch_add(&hist[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// every non-zero counter into the global histogram; rezero: the workgroup goes on counting
__device__ __forceinline__ void rdf_flush(unsigned* hist, int counters, unsigned long long* __restrict__ out, bool rezero) {
  __syncthreads();
  for (int k = threadIdx.x; k < counters; k += 256) {
    const unsigned v = hist[k];
    if (v) {
      atomicAdd(&out[k], (unsigned long long)v);
      if (rezero) hist[k] = 0u;
    }
  }
  if (rezero) __syncthreads();
}

template <class T>
__global__ __launch_bounds__(256) void k_rdf_tiles(int na, const T* __restrict__ pos, const int* __restrict__ tags, Box<T> box,
                                                   int n_types, T rmax2, T inv_dr, int n_bins, int counters, int n_tiles,
                                                   unsigned long long* __restrict__ out) {
  T* xyz = reinterpret_cast<T*>(rdf_lds);                             // [2][kRdfTile][3]
  int* tg = reinterpret_cast<int*>(xyz + 2 * kRdfTile * 3);           // [2][kRdfTile]
  unsigned* hist = reinterpret_cast<unsigned*>(tg + 2 * kRdfTile);    // [counters]
  const int tid = threadIdx.x;
  int I, J;
  rdf_tri_pair((int)blockIdx.x, n_tiles, &I, &J);
  const int i0 = I * kRdfTile, j0 = J * kRdfTile;
  const int ni = min(kRdfTile, na - i0), nj = min(kRdfTile, na - j0);
  for (int k = tid; k < counters; k += 256) hist[k] = 0u;
  for (int t = tid; t < 3 * ni; t += 256) xyz[t] = pos[3 * (long)i0 + t];
  for (int t = tid; t < 3 * nj; t += 256) xyz[3 * kRdfTile + t] = pos[3 * (long)j0 + t];
  if (tid < ni) tg[tid] = tags[i0 + tid];
  if (tid < nj) tg[kRdfTile + tid] = tags[j0 + tid];
  __syncthreads();
  if (tid < ni && rdf_tag_type(tg[tid]) < n_types) {
    const T ri[3] = {xyz[3 * tid], xyz[3 * tid + 1], xyz[3 * tid + 2]};
    const int tag_i = tg[tid];
    const T* xj = xyz + 3 * kRdfTile;
    const int* tj = tg + kRdfTile;
    for (int jj = 0; jj < nj; ++jj) {
      const int ch = rdf_pair_channel(tag_i, tj[jj], n_types);
      if (ch < 0 || (I == J && jj <= tid)) continue;
      const int b = rdf_pair_bin(box, ri, xj + 3 * jj, rmax2, inv_dr, n_bins);
      if (b >= 0) rdf_count(hist, ch * n_bins + b);
    }
  }
  rdf_flush(hist, counters, out, false);
}

template <class T>
__global__ __launch_bounds__(256) void k_rdf_cells(const CellAtom<T>* __restrict__ spos, const int* __restrict__ start,
                                                   const int* __restrict__ tags, Box<T> box, int g0, int g1, int g2, int n_types,
                                                   T rmax2, T inv_dr, int n_bins, int counters, unsigned long long* __restrict__ out) {
  T* xyz = reinterpret_cast<T*>(rdf_lds);                             // [kRdfChunk][3]
  int* tg = reinterpret_cast<int*>(xyz + kRdfChunk * 3);              // [kRdfChunk]
  unsigned* hist = reinterpret_cast<unsigned*>(tg + kRdfChunk);       // [counters]
  const int tid = threadIdx.x;
  const int home = (int)blockIdx.x;
  const int hb = start[home], he = start[home + 1], nh = he - hb;
  if (nh <= 0) return;                                                // (the whole workgroup: an empty cell has no pairs)
  for (int k = tid; k < counters; k += 256) hist[k] = 0u;
  const int c2 = home % g2, c01 = home / g2, c1 = c01 % g1, c0 = c01 / g1;
  const int n[3] = {g0, g1, g2}, c[3] = {c0, c1, c2};
  int h2 = 1, shift = 0;
  while (h2 < nh && h2 < 256) { h2 <<= 1; ++shift; }
  const int groups = 256 >> shift, grp = tid >> shift, li = tid & (h2 - 1);
  unsigned chunks = 0;
  const int cnt0 = rdf_sweep_count(g0), cnt1 = rdf_sweep_count(g1), cnt2 = rdf_sweep_count(g2);
  for (int hp = hb; hp < he; hp += h2) {                              // passes over a home cell of more than 256 atoms
    const int slot = hp + li;
    bool live = slot < he;
    T ri[3] = {T(0), T(0), T(0)};
    int tag_i = kRdfNotCounted;
    if (live) {
      const CellAtom<T> me = spos[slot];
      ri[0] = me.x; ri[1] = me.y; ri[2] = me.z;
      tag_i = tags[me.id];
      live = rdf_tag_type(tag_i) < n_types;
    }
    for (int a = 0; a < cnt0; ++a)
      for (int b = 0; b < cnt1; ++b)
        for (int e = 0; e < cnt2; ++e) {
          int t0, t1, t2;
          const int s0 = rdf_sweep_step(n[0], c[0], a, &t0), s1 = rdf_sweep_step(n[1], c[1], b, &t1),
                    s2 = rdf_sweep_step(n[2], c[2], e, &t2);
          const int take = rdf_sweep_take(s0, s1, s2);
          if (take < 0) continue;                                     // (uniform: the other cell takes this pair of cells)
          const int cid = (t0 * g1 + t1) * g2 + t2;
          const int kb = start[cid], ke = start[cid + 1];
          for (int k0 = kb; k0 < ke; k0 += kRdfChunk) {
            const int nc = min(kRdfChunk, ke - k0);
            __syncthreads();                                          // the chunk before this one has been walked
            if (tid < nc) {
              const CellAtom<T> p = spos[k0 + tid];
              xyz[3 * tid] = p.x; xyz[3 * tid + 1] = p.y; xyz[3 * tid + 2] = p.z;
              tg[tid] = tags[p.id];
            }
            __syncthreads();
            if (live)
              for (int jj = grp; jj < nc; jj += groups) {
                if (take == 0 && k0 + jj <= slot) continue;           // the home cell: every pair once
                const int ch = rdf_pair_channel(tag_i, tg[jj], n_types);
                if (ch < 0) continue;
                const int bin = rdf_pair_bin(box, ri, xyz + 3 * jj, rmax2, inv_dr, n_bins);
                if (bin >= 0) rdf_count(hist, ch * n_bins + bin);
              }
            if (++chunks == kRdfFlushChunks) {                        // (uniform) before a counter could wrap
              rdf_flush(hist, counters, out, true);
              chunks = 0;
            }
          }
        }
  }
  rdf_flush(hist, counters, out, false);
}

// One frame into `out` (channels x n_bins 64-bit counters, added to) by the plan `p` of rdf_plan.h, made for this n_atoms, this
// precision and this box; cs: the scratch of the cell form.  No host synchronisation.  Returns hipError_t as int.
template <class T>
int launch_rdf(hipStream_t st, const RdfPlan& p, int n_atoms, const T* pos, const int* tags, const Box<T>& box,
               int n_types, double r_max, int n_bins, CellScratch& cs, unsigned long long* out) {
  if (p.form == RDF_FORM_NONE) return 0;
  const T rmax2 = (T)(r_max * r_max), inv_dr = (T)((double)n_bins / r_max);
  const size_t sh = p.lds_bytes;
  if (p.form == RDF_FORM_TILES) {
    auto kern = k_rdf_tiles<T>;
    static size_t attr = 0;
    if (sh > 48 * 1024 && attr < sh) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh); attr = sh; }
    kern<<<(unsigned)p.workgroups, 256, sh, st>>>(n_atoms, pos, tags, box, n_types, rmax2, inv_dr, n_bins, p.counters, p.n_tiles, out);
    return (int)hipGetLastError();
  }
  const int rc = cell_bin_pack<T>(st, n_atoms, pos, box, p.grid, cs);
  if (rc != 0) return rc;
  auto kern = k_rdf_cells<T>;
  static size_t attr = 0;
  if (sh > 48 * 1024 && attr < sh) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh); attr = sh; }
  kern<<<(unsigned)p.workgroups, 256, sh, st>>>(reinterpret_cast<const CellAtom<T>*>(cs.spos), cs.start, tags, box, p.grid[0],
                                                p.grid[1], p.grid[2], n_types, rmax2, inv_dr, n_bins, p.counters, out);
  return (int)hipGetLastError();
}
template int launch_rdf<float>(hipStream_t, const RdfPlan&, int, const float*, const int*, const Box<float>&, int, double, int,
                               CellScratch&, unsigned long long*);
template int launch_rdf<double>(hipStream_t, const RdfPlan&, int, const double*, const int*, const Box<double>&, int, double,
                                int, CellScratch&, unsigned long long*);

}  // namespace admp
