// Kernel launchers shared between the translation units of libadmp_hip.
// Every launcher enqueues on `st` and returns immediately; T is float or double.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "env.h"
#include "frame_math.h"
#include "brick_plan.h"
#include "con_plan.h"
#include "mol_plan.h"
#include "mts_plan.h"
#include "pfa_maps.h"
#include "pme_math.h"
#include "scf_aspc.h"
#include "slab_plan.h"
#include "spline_math.h"

namespace admp {

// Per-nbonds scale tables (nbonds 0..15 -> scales[(nbonds-1) mod n], admp/pme.py:681-683) and the
// Fermi weight of the Thole-width switch at that pscale (admp/pme.py:337-348,411).
template <class T>
struct ScaleTab {
  T mm[16];   // mscale - 1
  T p[16];    // pscale
  T w0[16];
};

// i-grouped neighbour table: row i lists every partner of atom i (both directions of each i<j
// pair), entry = partner index | nbonds << 28.
struct NbrTable {
  int* rowptr = nullptr;   // na + 1
  int* col = nullptr;      // 2 * n_half
  // An evaluation's inner table (admp_set_cutoff on a multipolar handle, build_cut_table): a copy of the walked table's struct
  // whose col holds, at each row's own offset rowptr[i], the entries below the cutoff, and whose row i ends at rowend[i].
  // nullptr: row i ends at rowptr[i + 1] (every table a handle owns or borrows).  Never owned by the struct.
  int* rowend = nullptr;   // na
  int64_t n_half = 0;
  int64_t cap = 0;         // allocated entries of col
  int* order = nullptr;    // na: rows sorted by length inside windows of kRowWindow rows (launch_row_order), or nullptr
  // Site classes the table was compiled with: cls[a] = 1 for a charge-only atom (no dipole/quadrupole, not polarizable).
  // Entries whose PARTNER is charge-only carry kColMono and stand after all the others of their row, so the pair kernel
  // walks each row as two runs of uniform arithmetic.  k_prepare_sites checks cls against the sites of every call
  // (CLS_STALE / CLS_BETTER in the flag word next to E_NACT); a stale table is still a valid table of the general form.
  int* cls = nullptr;      // na
  int* order_plain = nullptr;   // na, only with cls: the row order WITHOUT the class grouping, for the kernels that have no
                                // use for classes (dispersion, Tang-Toennies: grouping costs them locality -- 0.49 -> 0.74 ms
                                // at 1M atoms on a borrowed, class-ordered table)
  // build scratch kept with the table (no allocation / synchronisation per rebuild): the second column buffer that the
  // out-of-place passes (row sort, class partition) write and swap with `col`, and the degree / cursor words
  int* col_alt = nullptr;
  int64_t cap_alt = 0;
  int* deg = nullptr;
  int deg_na = 0;
  // Slab ranks (round 4): a table built from positions holds the rows of the atoms near the rank's slab only (RowFilter);
  // built[i] = 1 for the atoms whose row exists (nullptr: every row).  The ownership pass refuses an evaluation in which an
  // atom without a row has become a home atom (the list is older than its skin allows).
  unsigned char* built = nullptr;
  void free_all() {             // the owner's buffers (a borrowed table is a copy of the lender's struct: never freed)
    for (int** p : {&rowptr, &col, &order, &cls, &order_plain, &col_alt, &deg})
      if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (built) { (void)hipFree(built); built = nullptr; }
    n_half = cap = cap_alt = 0; deg_na = 0;
  }
};
constexpr int kRowWindow = 1024;
constexpr int kColMask = 0x0fffffff;
constexpr int kColMono = (int)0x80000000u;   // partner is charge-only (NbrTable::cls)
constexpr int kNbMask = 7;                   // covalent class in bits 28..30
__host__ __device__ inline int col_nb(int c) { return (c >> 28) & kNbMask; }
enum { CLS_STALE = 1 /* an atom marked charge-only no longer is: ignore kColMono */, CLS_BETTER = 2 /* atoms became charge-only */ };

struct Topology {
  int na = 0;
  int* axis_type = nullptr;   // na
  int* axis_idx = nullptr;    // na * 3
  int* excl_ptr = nullptr;    // na + 1
  int* excl_col = nullptr;
  int* excl_nb = nullptr;
  // inverse frame map: inv_idx[inv_ptr[a] .. inv_ptr[a+1]) = sites whose local frame involves atom a
  int* inv_ptr = nullptr;     // na + 1
  int* inv_idx = nullptr;
  // frame groups: when every connected component of the "takes part in the frame of" graph is a run of <= kMaxGroup
  // consecutive atoms (molecular liquids: one group per molecule), group g = atoms grp_ptr[g] .. grp_ptr[g+1]-1 and the
  // closing kernel evaluates each frame ONCE, by one thread per group (k_finish_groups); else ngroups = 0 (pull form)
  int* grp_ptr = nullptr;     // ngroups + 1
  int ngroups = 0;
  // row form of the closing kernel (k_finish_rows, round 4): one thread per ATOM, a workgroup takes a run of whole groups of at
  // most kFinishBlock atoms -- rows_blk[b] .. rows_blk[b+1]-1 -- so that everything a frame needs of its group mates is
  // exchanged through LDS; grp_of[i] = (first atom of i's group) << 2 | (group size - 1)
  int* rows_blk = nullptr;    // nrowblk + 1
  int nrowblk = 0;
  int* grp_of = nullptr;      // na
  // the same cut into runs of at most kGatherRun atoms: one workgroup of the gather each when the closing work rides in its
  // epilogue (small systems: one dispatch fewer per step)
  int* gath_blk = nullptr;    // ngathblk + 1
  int ngathblk = 0;
};
constexpr int kFinishBlock = 256;
constexpr int kGatherRun = 32;
// closing work in the gather's epilogue (k_gather_staged<.., FIN>): what launch_finish takes besides the gather's arguments
template <class T>
struct FinishArgs {
  const T* pol = nullptr;
  T kappa = 0;
  T* dQlocal = nullptr;
  double* energies = nullptr;   // nullptr = epilogue off
  int want_grad = 1;            // 0: energies only (the frame adjoint is skipped)
};
constexpr int kMaxGroup = 4;

// energies[] slots on the device
enum { E_REAL = 0, E_RECIP = 1, E_SELF = 2, E_PEN = 3, E_NACT = 4 /* int: number of polarizable sites (k_prepare_sites) */,
       E_SCRATCH = 5 /* energy of passes whose energy nobody reads */, E_SCF_RECIP = 6, E_FMAX = 7 /* bit pattern */,
       E_FMAX1 = 8 /* bit patterns: residuals of checks 1 .. E_CHAIN of a chained SCF (engine.hip) */, E_CHAIN = 6,
       E_SLOTS = E_FMAX1 + E_CHAIN,
       E_PARTS = 64 /* partial sums of the atom-side reciprocal energy (k_gather<.., true>): 32k workgroups adding into ONE
                       word serialise at the memory side (0.2 ms at 1M atoms); 64 words take them in parallel */,
       E_RED = E_SLOTS + E_PARTS /* 4 words: (real, recip, self, penalty) packed for the SUM all-reduce of a slab evaluation */,
       E_RPARTS = E_RED + 4 /* E_PARTS partial sums of the real-space energy (k_pair_full: one word per workgroup modulo
                               E_PARTS instead of every workgroup's atomic on E_REAL); the real-space energy is E_REAL + their sum */,
       E_WORDS = E_RPARTS + E_PARTS /* one half of the double-buffered energy block */ };

// optional epilogue of the gather (small systems) or of the closing kernel (large ones), speculative first SCF cycle on
// one rank: total dE/dU and its maximum, exactly what launch_field_finish computes, without a separate dispatch
template <class T>
struct FieldFin {
  const T* pol = nullptr;
  const T* Ucart = nullptr;
  const T* fld_pair = nullptr;
  const T* fld_recip = nullptr;                // closing-kernel variant only (the gather has it in registers)
  T kappa = 0;
  T* field = nullptr;
  unsigned long long* fmax_bits = nullptr;   // nullptr = epilogue off
  const Site<T>* sites = nullptr;            // field-gather variant only: the full site rows (its own rows may be compact)
};
// ---- atom_kernels.hip
template <class T>
void launch_site_classes(hipStream_t st, int na, const Site<T>* sites, int* cls);   // NbrTable::cls <- site_is_mono
template <class T>
void launch_prepare_sites(hipStream_t st, const Topology& top, const T* pos, const T* Qlocal, const T* Ucart,
                          const T* pol, const T* thole, const Box<T>& box, Site<T>* sites,
                          double* zero_next /* E_WORDS doubles cleared for the next evaluation, or nullptr */,
                          const RecipGeom<T>& g, int4* bases /* optional: stencil base indices per atom */,
                          int* act_list = nullptr /* optional: the atoms with pol > 0 (unordered) ... */,
                          int* act_count = nullptr /* ... and their number: an int the caller has zeroed */,
                          const int* cls = nullptr /* NbrTable::cls, checked against the sites: flags OR-ed into ... */,
                          int* cls_flags = nullptr /* ... this word (CLS_STALE / CLS_BETTER) */,
                          RQ4<T>* rq = nullptr /* optional: compact copy (position, charge) of every row */,
                          T* Ucopy = nullptr /* optional: Ucart is read-only; this array receives a copy of it */,
                          const int* list = nullptr /* optional: only the rows of these atoms ... */, int nlist = 0 /* ... this many */);
template <class T>
void launch_local_frames(hipStream_t st, const Topology& top, const T* pos, const Box<T>& box, T* out /* (na,3,3) */);
// The dipole observable (dipole_kernels.hip): molecular dipoles mu_groups (n_groups,3; may be null) and the 16 words of
// admp_pme_dipoles over the groups of a CSR pair; rows: dipole_rows(n_groups) * 12 doubles of scratch.  No atomics, no read-back;
// n_groups = 0 zeroes out16 on the stream.  Returns hipError_t as int.
int dipole_rows(int n_groups);
template <class T>
int launch_dipoles(hipStream_t st, const Topology& top, const T* pos, const Box<T>& box, const T* Ql, const T* U /* may be null */,
                   const T* inv_mass, int n_groups, const int* group_start, const int* group_atoms, double* mu_groups, double* rows,
                   double* out16);
// field (Cartesian dE/dU) = pair (harmonic order) + recip (cartesian) + self + penalty; also max |field| over
// sites with pol > 0.001 (admp/pme.py:130,136) into *fmax_bits (order-preserving bit pattern of a non-negative real)
// Every per-atom / per-row launcher below takes an optional index list (`list`/`rows`, nullptr = atoms 0..n-1):
// with the x-slab decomposition a rank works on its "home" atoms only and n is the list length.
template <class T>
void launch_field_finish(hipStream_t st, int na, const Site<T>* sites, const T* pol, const T* Ucart, const T* fld_pair,
                         const T* fld_recip, T kappa, T* field, unsigned long long* fmax_bits, const int* list,
                         const int* n_dev = nullptr);
// Jacobi step over the polarizable sites (act list): dU = -field pol / D, U += dU (Cartesian array and packed harmonic
// copy), dU (harmonic order) into the pad words of the site row and into the compact row isites[slot] = {r, Q = 0, U = dU}
// that the increment's spread / gather read
template <class T>
void launch_jacobi_delta(hipStream_t st, int n_act, const int* act, const T* pol, const T* field, T* Ucart, Site<T>* sites,
                         Site<T>* isites, const unsigned long long* gate = nullptr /* device word: bit pattern of the residual */,
                         double gate_min = 0.0 /* with gate: a zero step unless residual >= gate_min */,
                         double relax = 1.0 /* factor on the step: the corrector's omega of a fixed-form call */);
// the predictor of a fixed-form call: out[i] = sum_{j < n} B[j] U[j][i] over `n_words` words, U[j] = the dipoles of j + 1
// calls ago (scf_aspc.h); accumulated in double, rounded once
template <class T>
struct AspcSets {
  int n = 0;
  const T* U[kAspcMaxSets] = {};
  double B[kAspcMaxSets] = {};
};
template <class T>
void launch_aspc_predict(hipStream_t st, long n_words, const AspcSets<T>& h, T* out);
// self term + polarization penalty energies, self potential, local-frame adjoint, dE/dQ_local
template <class T>
void launch_finish(hipStream_t st, const Topology& top, const T* pos, const Box<T>& box, const Site<T>* sites,
                   const T* pol, const T* Ucart, int lpol, T kappa, T* pot, T* grad, T* dQlocal, double* energies,
                   const int* list, int nlist,
                   const FieldFin<T>& ff = FieldFin<T>(),
                   const int* slab_bits = nullptr /* slab rank: per-atom words, kSlabHome marks the rank's own atoms (with a
                                                     home list); the frame-group kernel then serves the groups of home atoms */);
// which kernel launch_finish takes for this topology (list / slab_bits: whether the call hands one over), see atom_kernels.hip:
// out4 = {ADMP_FINISH_FORM_*, frame groups, runs of the row form, workgroups of the row form's launch}
void finish_launch_choice(const Topology& top, bool list, bool slab_bits, int out4[4]);
// dispersion: site rows carrying one scalar channel (Q[0] = vals[i*stride+chan], no dipoles/quadrupoles); also
// accumulates coef * sum_i vals^2 into energies[E_SELF] (the self term of admp/disp_pme.py:254-279)
template <class T>
void launch_scalar_sites(hipStream_t st, int na, const T* pos, const T* vals, int stride, int chan, double self_coef,
                         Site<T>* sites, double* energies);
// grad[i] += vals[i*stride+chan] * v[i]   (scalar site: dE/dr = c * Jac . F1)
// nch > 1: grad[i] += sum_b vals[i*stride+chan+b] * v[b][i] with v[b] = v + b * 3 * na
template <class T>
void launch_scale_add(hipStream_t st, int na, const T* vals, int stride, int chan, const T* v, T* grad, int nch = 1);
struct SelfCoefs {
  double c[3] = {0, 0, 0};
};
// channels 0..nch-1 of vals at once: site rows of channel b at sites + b * na
template <class T>
void launch_scalar_sites_batch(hipStream_t st, int na, const T* pos, const T* vals, int stride, int nch,
                               const double* self_coefs, Site<T>* sites, double* energies,
                               const RecipGeom<T>* g = nullptr /* with bases: the mesh the rows will be spread on */,
                               int4* bases = nullptr /* optional: stencil base indices per atom, as launch_prepare_sites */);
// ---- dft_kernels.hip: direct-DFT mesh convolution for mesh sizes rocFFT only does with Bluestein (dft_math.h)
// tw = (cos, sin)(2 pi m / K[d]) tables of the three dimensions back to back (K[0] + K[1] + K[2] complex numbers)
int dft_tile_cols(int N);
// nb independent meshes (batch) are transformed by one launch each: mesh b at mesh + b * mesh_stride, its half spectrum
// at spec + b * spec_stride (strides in reals), its G table tabs.p[b] (dispersion PME: the C6 / C8 / C10 passes)
template <class T>
struct DftTabs {
  const T* p[3] = {nullptr, nullptr, nullptr};
};
// z and y lines of every x plane in one kernel (dft_kernels.hip, round 3); dft_zy_fits: the plane and its spectrum fit the LDS
template <class T>
bool dft_zy_fits(const int K[3]);
// what the forward plane kernel needs to build its planes itself (no spread kernel, no mesh): nb channels of na site rows back to back
template <class T>
struct PlaneSpread {
  int na = 0, lpol = 0;
  const Site<T>* sites = nullptr;
  const int4* bases = nullptr;      // stencil records of the atoms (k_prepare_sites), or nullptr: from the positions
  RecipGeom<T> g;
};
template <class T>
bool dft_zy_spread_fits(const int K[3], int na);
template <class T>
bool launch_dft_zy(hipStream_t st, const int K[3], const T* tw, T* mesh, T* spec, int inverse, int nb = 1, long mesh_stride = 0,
                   long spec_stride = 0, T* accum = nullptr, const PlaneSpread<T>* sp = nullptr /* forward only */,
                   int* mfma_share = nullptr /* out: 1 where the launch carries a matrix-core share (plane_mfma_plan.h) */);
template <class T>
bool launch_dft_z(hipStream_t st, const int K[3], const T* tw, T* mesh, T* spec, int inverse, int nb = 1,
                  long mesh_stride = 0, long spec_stride = 0,                                     // r2c / c2r along z
                  T* accum = nullptr /* c2r of one mesh: accum += result as well; returns whether that was done */);
template <class T>
void launch_dft_y(hipStream_t st, const int K[3], const T* tw, T* spec, int inverse, int nb = 1,
                  long spec_stride = 0);                                                          // in place along y
// along x: forward, spec *= gtab with energies[slot] += sum w G |S|^2, inverse -- one kernel, in place
template <class T>
void launch_dft_x_conv(hipStream_t st, const int K[3], const T* tw, T* spec, const DftTabs<T>& tabs, double* energies,
                       int slot, int nb = 1, long spec_stride = 0);
// the x pass of one mesh as a real circulant product per column (dft_math.h), for a G table that is even along x:
// launch_ctab builds ctab [K1/2+1][K2][K3/2+1] from gtab and sets *uneven (device word, cleared by the caller) where a
// column of gtab is not even -- ctab must then not be used
template <class T>
void launch_dft_x_circ(hipStream_t st, const int K[3], T* spec, const T* ctab, double* energies, int slot);
template <class T>
void launch_ctab(hipStream_t st, const int K[3], const T* gtab, T* ctab, int* uneven);

// ---- pfa_kernels.hip: two-level (Good-Thomas) direct DFT for mesh dimensions N = N1 * N2 > 160 with a hard prime power N2
// (PfaAxis, the split and the index maps: pfa_maps.h)
struct PfaPlan {
  PfaAxis ax[3];
  int Khp;                                    // stored z columns: ax[2].N1 * (ax[2].N2 / 2 + 1)
  int tw_off[3];                              // twiddles of axis d at tw + tw_off[d] (complex entries): N2 entries, then N1
  const int* ptab[3];                         // device: index table of axis d (pfa_index_table)
};
bool pfa_split(int N, PfaAxis* out);          // pfa_split_at with ADMP_PFA_MIN (default 160) as plain_max; false: no usable split
// which form each pass of the plan takes for words of w bytes: out[3 * d + 0 .. 2] = columns (x, y: NC) or lines (z: NL of the
// forward pass) per workgroup, MFMA stage A or not, NL of the inverse z pass (0 on x and y) -- the launchers' own choices
void pfa_forms(const PfaPlan& p, size_t w, int out[9]);
template <class T>
void launch_pfa_z(hipStream_t st, const PfaPlan& p, const T* tw, T* mesh, T* spec, int inverse, int nb = 1, long mesh_stride = 0,
                  long spec_stride = 0);
template <class T>
void launch_pfa_y(hipStream_t st, const PfaPlan& p, const T* tw, T* spec, int inverse, int nb = 1, long spec_stride = 0);
template <class T>
void launch_pfa_x_conv(hipStream_t st, const PfaPlan& p, const T* tw, T* spec, const DftTabs<T>& tabs, double* energies, int slot,
                       int nb = 1, long spec_stride = 0);

// ---- fftx_kernels.hip: x lines forward * G (+ energy) * x lines inverse in one sweep, power-of-two K[0]
bool fftx_usable(int N);
template <class T>
void launch_fftx_conv(hipStream_t st, const int K[3], const T* tw, T* spec, const T* gtab, double* energies, int slot,
                      int khp = 0 /* row pitch of spec in complex numbers (0: K[2]/2+1) */,
                      int ny = 0 /* y rows held: spec and gtab are [K0][ny][..] (0: K[1]; a slab rank holds its own rows) */);
template <class T>
void launch_fftx_conv_batch(hipStream_t st, const int K[3], const T* tw, T* spec, const DftTabs<T>& tabs, int nb,
                            long spec_stride /* reals between the spectra of consecutive channels */, double* energies, int slot,
                            int khp = 0, int ny = 0);

// ---- pair_kernels.hip
// incremental SCF: the polarizable-polarizable sub-table (rows keyed by atom) that k_pair_field_ind walks.
// Row i holds its kept entries at col[beg[i] .. end[i]) with beg = the neighbour table's own row offsets (borrowed pointer):
// the sub-table is written in ONE pass over the neighbour table -- no count pass, no prefix sum, no host read of the total
// (round 4; the two-pass build cost 0.57 ms per list rebuild at 1M atoms plus a hipMalloc / hipFree pair).  col is as long
// as the neighbour table's column array; for water 1/9 of it is used.
struct IndTable {
  const int* beg = nullptr;   // = NbrTable::rowptr of the table it was built from (not owned)
  int* end = nullptr;         // na
  int* col = nullptr;
  int64_t cap = 0;            // entries col can hold
  int na_cap = 0;             // rows `end` can hold
};
// The argument record of the closing pair kernel, in a launch of its own (launch_pair_full) or as a rider of the x pass of a
// direct-DFT convolution (k_xconv_pair_full, through launch_dft_x_pass).  The caller fills everything but nblocks / grid,
// which the launcher sets for the lane count it picks; on == 0: absent.
template <class T>
struct PairFullArgs {
  int on = 0, na = 0;           // na: the rows of this launch
  const int* rowptr = nullptr;  // the neighbour table; rowend != nullptr: an evaluation's inner table (NbrTable::rowend)
  const int* rowend = nullptr;
  const int* col = nullptr;
  const Site<T>* sites = nullptr;
  Box<T> box;
  ScaleTab<T> tab;
  T kappa = 0;
  T* grad = nullptr;
  T* pot = nullptr;
  double* energies = nullptr;
  const int* rows = nullptr;
  T* fld = nullptr;             // optional: also write the real-space dE/dU (speculative SCF pass)
  unsigned nblocks = 0, grid = 0;
  int use_mono = 0;             // 1: charge-only sites take the reduced forms (pme_math.h): not for dE/dQ_local requests
  const int* cls_flags = nullptr;   // the flag word launch_prepare_sites wrote for THIS evaluation
  const RQ4<T>* rq = nullptr;       // compact position/charge rows of launch_prepare_sites
  const T* tholes = nullptr;        // the caller's per-atom thole array, or nullptr
};
// The argument record of the SCF field kernels, on their own or as riders of an x pass (k_xconv_pair, k_xconv_pair_full).
// kind 1 = k_pair_field: the neighbour table, cls_flags / rq / tholes as in PairFullArgs, n_dev (optional): the row count
// lives on the device and na is the bound the grid is sized for.  kind 2 = k_pair_field_ind: fld[row] += sum_j T_ij dU_j,
// dU_j in the pad words of sites[j]; rowptr / rowend / col = the IndTable's beg / end / col.  kind 0: absent.
template <class T>
struct PairFieldArgs {
  int kind = 0, na = 0;
  const int* rowptr = nullptr;
  const int* rowend = nullptr;
  const int* col = nullptr;
  const Site<T>* sites = nullptr;
  Box<T> box;
  ScaleTab<T> tab;
  T kappa = 0;
  T* fld = nullptr;
  const int* rows = nullptr;
  unsigned nblocks = 0, grid = 0;
  const int* n_dev = nullptr;
  const int* cls_flags = nullptr;
  const RQ4<T>* rq = nullptr;
  const T* tholes = nullptr;
};
template <class T>
void launch_pair_full(hipStream_t st, PairFullArgs<T> a, int lpol);
template <class T>
void launch_pair_field(hipStream_t st, PairFieldArgs<T> a);       // kind 1
template <class T>
void launch_pair_field_ind(hipStream_t st, PairFieldArgs<T> a);   // kind 2
// Can the kernel of this record ride in an x pass?  false: no rows, or another lane count (the closing kernel: another
// type, or not polarizable) than the rider kernels are compiled for -- the caller then launches it on its own.
template <class T>
bool full_rider(const PairFullArgs<T>& a, int lpol);
template <class T>
bool field_rider(const PairFieldArgs<T>& a);
// The x pass of the direct-DFT convolution of one mesh, with or without riders: k_dft_x_circ (ctab != nullptr: the circulant
// form, launch_ctab; tw and tabs are then unused) or k_dft_x_conv on their own; with a field rider k_xconv_pair; with the
// closing pair kernel k_xconv_pair_full, which takes a field rider of kind 2 along.  Absent riders: nullptr or on / kind 0.
template <class T>
void launch_dft_x_pass(hipStream_t st, const int K[3], const T* tw, T* spec, const DftTabs<T>& tabs, double* energies, int slot,
                       const T* ctab, const PairFieldArgs<T>* field, const PairFullArgs<T>* full);
// (nbr_kernels.hip) inner table of an MD loop: the entries of `full` whose minimum-image distance is below rc, rows compacted
// in the order of `full`.  hipError_t as int; one host synchronisation (the entry count).
template <class T>
int prune_table(hipStream_t st, int na, const NbrTable& full, const T* pos, const Box<T>& box, double rc, int* rowptr_out,
                int* cnt, int* col_out, void** scratch, size_t* scratch_bytes, int64_t* total);
// (nbr_kernels.hip) inner table of one evaluation with a cutoff (admp_set_cutoff on a multipolar handle): for the n rows
// `rows` (nullptr: rows 0 .. n-1) the entries of `nb` whose minimum-image distance at the site rows is below rc, written at the
// row's own offset nb.rowptr[i] in the order of nb (class runs survive): col_out[nb.rowptr[i] .. end_out[i]).  With iend /
// icol also the polarizable-polarizable part of those entries (the sub-table of build_ind_table, below rc).  col_out and icol
// hold as many entries as nb.col.  No atomics, no host synchronisation; hipError_t as int.
template <class T>
int build_cut_table(hipStream_t st, int n, const int* rows, const NbrTable& nb, const Site<T>* sites, const Box<T>& box,
                    double rc, int* end_out, int* col_out, int* iend, int* icol);
// (nbr_kernels.hip) ascending in-place sort of n ints; keys_tmp = n ints of scratch.  hipError_t as int.
int sort_ints(hipStream_t st, int* keys, int* keys_tmp, int n, void** scratch, size_t* scratch_bytes);
// (nbr_kernels.hip) it <- the polarizable-polarizable entries of nb; rows keyed by atom, empty for non-polarizable atoms.
// Returns a hipError_t as int; no host synchronisation (allocates only when the neighbour table has grown).
template <class T>
int build_ind_table(hipStream_t st, int na, const NbrTable& nb, const Site<T>* sites, IndTable& it);
int pair_lanes_per_row(int n_rows);   // 4/8/16 by row count; env ADMP_PAIR_LPR overrides
// the launchers' choices for a record of n_rows rows (kind 0: k_pair_full, 1: k_pair_field, 2: k_pair_field_ind), see pair_kernels.hip
void pair_launch_choice(int kind, int n_rows, int lpol, size_t real_bytes, int out4[4]);
// sumX[i] = sum_j dE_ij/d ln(au_ij), sumXw[i] = sum_j (same) * d ln(au_ij)/d thole_i  (pme_math.h pair_thole_logderiv)
template <class T>
void launch_thole_sums(hipStream_t st, int na, const NbrTable& nb, const Site<T>* sites, const Box<T>& box,
                       const ScaleTab<T>& tab, T* sumX, T* sumXw, const int* rows = nullptr, int n_rows = 0);
// cls16[nb] += sum over the pairs of covalent class nb of d(pair energy)/d(mscale); kind 0: multipolar PME (sites),
// 1: dispersion (pos, par = c6/c8/c10 per atom, pmax), 2: Tang-Toennies (pos, par = a/b/q/c6 per atom)
template <class T>
void launch_mscale_sums(hipStream_t st, int kind, int na, const NbrTable& nb, const Site<T>* sites, const T* pos,
                        const T* par, const Box<T>& box, int pmax, double* cls16,
                        double cutoff = 0.0 /* kinds 1, 2: listed pairs beyond it are skipped (admp_set_cutoff) */,
                        const int* rows = nullptr /* slab rank: its n_rows home rows */, int n_rows = 0);
// cls16[nb] += sum over the pairs of covalent class nb of d(pair energy)/d(pscale) (pme_math.h pair_pscale_deriv)
template <class T>
void launch_pscale_sums(hipStream_t st, int na, const NbrTable& nb, const Site<T>* sites, const Box<T>& box,
                        const ScaleTab<T>& tab, double* cls16, const int* rows = nullptr, int n_rows = 0);
// packed rows of the scalar pair kernels: position (3) + up to 4 per-atom parameters + pad, one aligned 8-real row per atom
template <class T>
struct alignas(8 * sizeof(T)) SRow {
  T v[8];
};
template <class T>
void launch_pack_scalar_rows(hipStream_t st, int na, int np /* parameters per atom: 3 (c6, c8, c10) or 4 (a, b, q, c6) */,
                             const T* pos, const T* par, SRow<T>* rows);
template <class T>
void launch_disp_pair(hipStream_t st, int na, const NbrTable& nb, const SRow<T>* srows, const Box<T>& box,
                      const ScaleTab<T>& tab, T kappa, int pmax, T* grad, double* energies,
                      const int* rows = nullptr /* the n_rows rows to evaluate (nullptr: all, in the table's order) */,
                      int n_rows = 0, double cutoff = 0.0 /* > 0: listed pairs beyond it are skipped (admp_set_cutoff) */);
template <class T>
void launch_tt_pair(hipStream_t st, int na, const NbrTable& nb, const SRow<T>* srows, const Box<T>& box,
                    const ScaleTab<T>& tab, T* grad, double* energies, const int* rows = nullptr, int n_rows = 0,
                    double cutoff = 0.0);

// ---- box gradient (dE/dbox at fixed Cartesian positions; on request only).  All sums are double device words.
// vir[9] += 1/2 sum_entries shift (x) dE_pair/dr_I over the pairs whose minimum image crosses the cell boundary
template <class T>
void launch_pair_virial(hipStream_t st, int na, const NbrTable& nb, const Site<T>* sites, const Box<T>& box,
                        const ScaleTab<T>& tab, T kappa, int lpol, double* vir,
                        const int* rows = nullptr /* slab rank: its n_rows home rows */, int n_rows = 0);
template <class T>
void launch_scalar_pair_virial(hipStream_t st, int tt, int na, const NbrTable& nb, const T* pos, const T* par,
                               const Box<T>& box, const ScaleTab<T>& tab, T kappa, int pmax, double* vir, double cutoff = 0.0,
                               const int* rows = nullptr /* slab rank: its n_rows home rows */, int n_rows = 0);
// vir[9] += shift (x) dE/d(frame vector) of the local frames whose axis vectors cross the cell boundary
template <class T>
void launch_frame_virial(hipStream_t st, const Topology& top, const T* pos, const Box<T>& box, const Site<T>* sites,
                         int lpol, T kappa, const T* pot, double* vir, const int* list = nullptr /* home sites */, int nlist = 0);
// tk[6] += sum_k w dG/dk^2 |S_k|^2 k (x) k (xx, yy, zz, xy, xz, yz), spectrum NOT yet multiplied by G (single rank)
template <class T>
void launch_kspace_virial(hipStream_t st, const int K[3], const double* box_inv, double volume, double kappa, int which,
                          int ref_order, const T* spec, double* tk,
                          int y0 = 0, int ny = 0 /* spec holds the y rows y0 .. y0+ny-1 as [K0][ny][K2/2+1] (0: all K[1] rows) */);
// xw[9] += sum_atoms x (x) dE_recip/dx ; yy[9] += sum_atoms dE_recip/dAop (recip_box_terms)
template <class T>
void launch_gather_virial(hipStream_t st, int na, const Site<T>* sites, int lpol, const RecipGeom<T>& g, const T* phi,
                          double* xw, double* yy, const int* list = nullptr /* the na atoms to gather at (nullptr: 0 .. na-1) */);

// BrickGrid, make_bricks, brick_of, brick_code: brick_plan.h
// below this atom count the spread uses global atomics (8 lanes per atom) instead of binned LDS bricks
// (default 20000; env ADMP_SPREAD_BRICK_MIN overrides, 0 forces the brick path -- used by the parity tests)
int spread_brick_min_atoms();
// launch_spread(na atoms, this mesh) takes the binned brick kernel and leaves its lists in the BinScratch
template <class T>
bool spread_uses_bricks(int na, const RecipGeom<T>& g);
// scratch for the per-call binning: brick offsets cell_start[ncell+1] (+cursor copy) and the
// (atom, brick) entry list sorted[<= 8 na] (a stencil touches at most 2 bricks per axis)
struct BinScratch {
  int* cell_start = nullptr;   // ncell + 1
  int* cursor = nullptr;       // ncell + 1: per-brick entry counts (input of the scan)
  int* fillcur = nullptr;      // ncell + 1: per-brick fill cursors of the second binning pass
  bool counters_zero = false;  // cursor / fillcur are all zero (the brick kernel clears its own words when it is done)
  int* sorted = nullptr;       // 8 * na
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
};

// ---- recip_kernels.hip
// LDS-brick spread: bins the atoms, accumulates every brick in LDS, writes each mesh point exactly once
// (no memset, no global atomics).  Returns a hipError_t as int.
template <class T>
int launch_spread(hipStream_t st, int na, const Site<T>* sites, int lpol, const RecipGeom<T>& g, BinScratch& bs,
                  T* mesh, const int* list, const int4* bases = nullptr /* from launch_prepare_sites, or recomputed */,
                  int nb = 1 /* batch (scan kernel only): site rows of b at sites + b * na, its mesh at mesh + b * mesh size */,
                  int reuse_bins = 0 /* binned kernel: positions unchanged since the previous call, keep its brick lists */,
                  int tight = 1 /* binned kernel, f32: fixed-point scale from the stencil-window bound (0: entry count; SCF increments) */);
size_t spread_scan_bytes(int ncell);
// which kernel launch_spread takes for na atoms on a mesh of these local dimensions (admp_mesh_spread reports it; the rules and
// switches stay in recip_kernels.hip): out4 = {0 scan, 1 planes, 2 bricks; bricks along x, y, z}
void spread_launch_choice(int na, const int dims[3], int out4[4]);
// k-space layout [K0][ny][K2/2+1] holding mesh rows y0 .. y0+ny-1 (ny = K1, y0 = 0 on one rank).
// which: 1 = electrostatics (Ck_1, gamma point dropped, x DIELECTRIC), 6/8/10 = dispersion kernels
template <class T>
void launch_gtab(hipStream_t st, const int K[3], int y0, int ny, const double* box_inv, double volume, double kappa,
                 int which, T* gtab, int ref_order = 0 /* the reference's k-point table, see k_gtab */,
                 const int* fmap = nullptr /* slot-ordered spectrum (pfa_kernels.hip): device table of the frequency stored
                                              at every x slot (K0), y slot (K1) and z column (nh), back to back */,
                 int nh = 0 /* with fmap: number of stored z columns */);
// spec <- spec * gtab ; energies[slot] += sum_k w_k (gtab/2) |S_k|^2
template <class T>
void launch_kspace(hipStream_t st, const int K[3], int ny, const T* gtab, T* spec /* interleaved complex */,
                   double* energies, int slot);
template <class T>
void launch_gather(hipStream_t st, int na, const Site<T>* sites, int lpol, const RecipGeom<T>& g, const T* phi, T* pot,
                   T* grad, const int* list, T* fld_recip /* optional: cartesian reciprocal dE/dU */,
                   const FieldFin<T>& ff = FieldFin<T>(),
                   double* e_recip = nullptr /* optional: += 1/2 sum_i Q_tot,i . dE_recip/dQ_i = the reciprocal energy */,
                   const Topology* top = nullptr /* with fin: the workgroups take the runs of whole frame groups top->gath_blk */,
                   const Box<T>* box = nullptr, const FinishArgs<T>& fin = FinishArgs<T>());
template <class T>
void launch_gather_field(hipStream_t st, int na, const Site<T>* sites, const RecipGeom<T>& g, const T* phi,
                         T* fld_recip, const int* list, int nb = 1 /* batch: phi of b at phi + b * mesh size, fld + b * 3 * na */,
                         const int* n_dev = nullptr /* atom count on the device (na = grid bound) */,
                         const int* add_to = nullptr /* rows are compact: ADD the result to fld_recip[3 * add_to[slot]] */,
                         const FieldFin<T>& ff = FieldFin<T>() /* small systems: total dE/dU and its maximum of the rows' atoms
                                                                 ride along (launch_field_finish's work; nb = 1) */);
// a += b over n mesh points
template <class T>
void launch_mesh_add(hipStream_t st, long n, T* a, const T* b);
// the binning passes of launch_spread on their own (count, scan, fill): leaves the brick lists of the n listed atoms in bs;
// `bases` must hold the stencil records of those atoms (sites may then be nullptr).  hipError_t as int.
template <class T>
int launch_bin_bricks(hipStream_t st, int na, const Site<T>* sites, const RecipGeom<T>& g, BinScratch& bs, const int* list,
                      const int4* bases);
// ---- disp_kernels.hip: the scalar channels of dispersion PME through ONE spread and ONE gather
template <class T>
void launch_atom_bases(hipStream_t st, int na, const T* pos, const RecipGeom<T>& g, int4* bases);
// mesh of channel c (vals[i * stride + c]) at mesh + c * mesh_stride, from the brick lists in bs.  hipError_t as int.
template <class T>
int launch_spread_scalar(hipStream_t st, int nch, const T* pos, const T* vals, int stride, const RecipGeom<T>& g,
                         const BinScratch& bs, T* mesh, long mesh_stride);
// grad[i] += sum_c vals[i][c] Jac . grad phi_c(r_i) for the n listed atoms
template <class T>
void launch_gather_scalar(hipStream_t st, int nch, int na, const T* pos, const T* vals, int stride, const RecipGeom<T>& g,
                          const T* phi, long mesh_stride, T* grad, const int* list,
                          int interleaved = 0 /* phi = [mesh point][nch]: the channels of a point side by side (launch_interleave) */,
                          const int* types = nullptr /* typed form: atom i gathers, with weight 1, from mesh types[i] */);
// typed dispersion meshes (disp_kernels.hip k_spread_bricks_typed): unit sources into mesh types[i]; nt = 1..3
template <class T>
int launch_spread_typed(hipStream_t st, int nt, const T* pos, const int* types, const RecipGeom<T>& g, const BinScratch& bs,
                        T* mesh, long mesh_stride);
// x pass of the typed form (fftx_kernels.hip k_fftx_mix): spec holds nt type meshes; at every k the channel structure
// factors S_p = sum_t ctab[p][t] S_t are formed, E += w G_p |S_p|^2, and the types get back psi_t = sum_p ctab[p][t] G_p S_p
struct MixTab { double c[3][4]; int nch, nt; };      // c[power][type]; columns of unused (padding) types are zero
// direct-DFT meshes (dft_kernels.hip k_dft_x_mix): the same combination between the forward and inverse x lines
template <class T>
void launch_dft_x_mix(hipStream_t st, const int K[3], const T* tw, T* spec, const DftTabs<T>& tabs, const MixTab& mix,
                      long spec_stride, double* energies, int slot);
// w[i][t] = (types[i] == t): the typed form through the kernels that take per-atom weights (small systems)
void launch_type_counts(hipStream_t st, int na, const int* types, int* counts4 /* zeroed by the caller */);
template <class T>
void launch_onehot(hipStream_t st, int na, int nt, const int* types, T* w);
template <class T>
void launch_types_check(hipStream_t st, int na, const T* vals, int stride, const int* types, const MixTab& mix, double* bad);
template <class T>
void launch_fftx_mix(hipStream_t st, const int K[3], const T* tw, T* spec, const DftTabs<T>& tabs, const MixTab& mix,
                     long spec_stride, double* energies, int slot, int khp);
// dst[i * nch + c] = src[c * stride + i], i < n: the nch meshes of a dispersion call side by side per mesh point, so that the
// gather fetches all channels of a stencil point with ONE load instruction
template <class T>
void launch_interleave(hipStream_t st, int nch, long n, const T* src, long stride, T* dst);
// energies[E_SELF] += sum over the n listed atoms and the nch channels of self_coefs[c] vals[i][c]^2
template <class T>
void launch_scalar_self(hipStream_t st, int nch, int na, const T* vals, int stride, const int* list, const double* self_coefs,
                        double* energies);
// out[i * stride + chan] += phi(r_i) + extra * vals[i * stride + chan]  (mesh potential at the atoms: dE_recip/dc_i)
// workgroups the dispersion launchers of disp_kernels.hip use (they call these themselves; the test entries report them):
// brick spreads of a local mesh, k_gather_scalar over na rows, k_gather_value over na rows
int disp_spread_groups(const int dims[3]);
unsigned disp_gather_groups(int na);
int disp_value_groups(int na);
template <class T>
void launch_gather_value(hipStream_t st, int na, const T* pos, const T* vals, int stride, int chan, const RecipGeom<T>& g,
                         const T* phi, double extra, T* out, const int* list = nullptr /* the na atoms (nullptr: 0 .. na-1) */);
// (pair_kernels.hip) per-atom parameter derivatives of the scalar pair terms: tt = 0 dispersion, out (na,3) = dE/dc6,c8,c10;
// tt = 1 Tang-Toennies, out (na,4) = dE/d(a, b, q, c6)
template <class T>
void launch_scalar_pair_pgrad(hipStream_t st, int tt, int na, const NbrTable& nb, const T* pos, const T* par, const Box<T>& box,
                              const ScaleTab<T>& tab, T kappa, int pmax, T* out, double cutoff = 0.0,
                              const int* rows = nullptr, int n_rows = 0);
// ---- cell_kernels.hip: positions -> half pair list (cell list), two phases so that the caller can size `pairs`
struct CellScratch {
  int n[3] = {0, 0, 0};
  int* start = nullptr; int* cursor = nullptr; int* sorted = nullptr;
  long long* count = nullptr; long long* offs = nullptr;
  void* spos = nullptr;        // cell-sorted packed records (x, y, z, atom id), 4 reals (<= 32 B) per atom
  int* deg4 = nullptr;         // partial row lengths: 4 per atom (lanes of k_cell_rows) or 16 (k_brute_rows), cap_part words
  void* scan_tmp = nullptr; size_t scan_bytes = 0;
  int cap_atoms = 0, cap_cells = 0;
  size_t cap_part = 0;         // words behind deg4 (cell_plan.h cell_partial_words: NOT monotonic in the atom count)
  int ensure(int na, int ncell);
  void release();
};
// cell-sorted record of one atom (CellScratch::spos): a sweep reads ONE 16-B (f32) / 32-B (f64) word per candidate instead of
// an index and three scattered coordinates
template <class T>
struct alignas(4 * sizeof(T)) CellAtom {
  T x, y, z;
  int id;
};
// the binning stage alone: cs.start (cell starts of the grid n, n[0] n[1] n[2] + 1 words) and cs.spos (the records; inside a
// cell in NO particular order: for sweeps that do not depend on it) from the positions; no host synchronisation.  Returns
// hipError_t as int.
template <class T>
int cell_bin_pack(hipStream_t st, int na, const T* pos, const Box<T>& box, const int n[3], CellScratch& cs);
// (rdf_kernels.hip) the typed pair-distance counts of one frame ADDED to out (channels x n_bins 64-bit counters) by the plan of
// rdf_plan.h; tags: type | group << 4 per atom (rdf_math.h); cs: the scratch of the cell form.  Integer atomics only, no host
// synchronisation.  Returns hipError_t as int.
struct RdfPlan;
template <class T>
int launch_rdf(hipStream_t st, const RdfPlan& plan, int n_atoms, const T* pos, const int* tags, const Box<T>& box, int n_types,
               double r_max, int n_bins, CellScratch& cs, unsigned long long* out);
// (tcf_kernels.hip) one frame of the time correlation functions by the plan of tcf_plan.h: the frame goes into the caller's ring
// (n_lags, 2, 3, n_slots), the sums of |d(t) - d(t - k)|^2 and v(t) . v(t - k) per type and lag are ADDED to acc (2, n_types,
// n_lags); partial: plan.scratch_bytes of scratch.  The box is double whatever T: the unwrap runs in double (tcf_math.h).  No float
// atomics, no host synchronisation.  Returns hipError_t as int.
struct TcfPlan;
template <class T>
int launch_tcf(hipStream_t st, const TcfPlan& plan, int n_atoms, const T* pos, const T* vel, const Box<double>& box, int n_slots,
               const int* slot_atom, int n_tiles, const int* tile_type, int tile_atoms, int n_types, int n_lags, int64_t frame,
               T* ring, double* unwrapped, T* last, unsigned long long* jumps, double* partial, double* acc);
template <class T>
int cell_count_pairs(hipStream_t st, int na, const T* pos, const Box<T>& box, const double* heights, double rc,
                     CellScratch& cs, long long* n_pairs);
template <class T>
int cell_fill_pairs(hipStream_t st, int na, const T* pos, const Box<T>& box, double rc, CellScratch& cs, int* pairs);
// positions -> the pair kernels' neighbour table directly (both directions, nbonds packed), no pair array in between
// rows to build (slab ranks): the atoms whose approximate stencil base plane floor(frac_x K0) - 2 lies in the periodic
// interval [lo, lo + width) of the K0 planes along x; on == 0: every row
struct RowFilter {
  int on = 0;
  int K0 = 0, lo = 0, width = 0;
};
template <class T>
int cell_build_table(hipStream_t st, const Topology& top, const T* pos, const Box<T>& box, const double* heights,
                     double rc, CellScratch& cs, NbrTable& nb, const RowFilter& rf = RowFilter());

// ---- slab_kernels.hip: x-slab decomposition (multi-GPU) ------------------------------------------------------------------
// (the plain constants and records of the decomposition -- kSlabHome, SlabCols, SlabBins, SlabSegs -- are slab_plan.h's)
// owner[na] / bits[na] of this evaluation and the compacted columns lists[c * na ..]; totals[ncols] stay on the device
// (the caller reads them once).  counts: ncols * slab_compact_blocks(max len) ints of scratch.  hipError_t as int.
// owner_prev (optional): the owners of the previous evaluation; mig[na] then receives, for the atoms that changed hands,
// 1 << previous owner (atoms this rank took over) or kSlabHome | 1 << new owner (atoms it gave away), else 0
// totals[cs.ncols] (one word past the columns' totals) comes back non-zero when a home atom has no row in a filtered table
int launch_slab_decompose(hipStream_t st, int na, const NbrTable& nb, const Topology& top, const int4* bases, const void* pol,
                          int prec, int width, int K0, int X0, int nranks, int me, int* owner, int* bits,
                          const SlabCols& cs, const SlabBins& sb, int* counts, int* totals, int* lists,
                          const int* owner_prev = nullptr, int* mig = nullptr);
int slab_compact_blocks(int maxlen);
void launch_slab_concat(hipStream_t st, const SlabSegs& segs, const int* lists, long col_stride, int* out);
template <class T>
void launch_rows_gather(hipStream_t st, int n, int w, const int* idx, const T* src, T* out);
// mode 0: dst[idx[k]] = in[k]; 1: dst[idx[k]] += in[k]; 2: dst[idx[k]] = 0 (in unused)
template <class T>
void launch_rows_scatter(hipStream_t st, int mode, int n, int w, const int* idx, const T* in, T* dst);
// what 0: Cartesian induced dipoles of the listed atoms; what 1: the last Jacobi step's change (site pad words)
template <class T>
void launch_halo_u_pack(hipStream_t st, int n, int what, const int* idx, const T* Ucart, const Site<T>* sites, T* out);
template <class T>
void launch_halo_u_unpack(hipStream_t st, int n, int what, const int* idx, const T* in, T* Ucart, Site<T>* sites);
// spec[nx][K1][pitch] complex (nh used per row) <-> all-to-all buffer (block of peer t: [nx][ny_t][nh]); dir 0 pack, 1 unpack
template <class T>
void launch_transpose_pack(hipStream_t st, int nx, int K1, int nh, int pitch, int nranks, int dir, T* spec, T* buf);
// out[4] = (real, recip, self, penalty) of the energy block e; recip_slot >= 0: that word, -1: the sum of the E_PARTS words
void launch_energy_pack(hipStream_t st, const double* e, int recip_slot, double* out);

// ---- nbr_kernels.hip
// order[] <- the rows of every window of W <= kRowWindow consecutive rows sorted by neighbour count (ties by index).  The
// pair kernels give each row a fixed group of lanes, so a wavefront runs as long as its longest row: with rows of
// equal length side by side the lanes stay busy (water, rc 4 A: 85 % -> 99 % of the lane-iterations useful), while the
// window keeps the rows' site / output accesses local.
void launch_row_order(hipStream_t st, int na, const int* rowptr, int* order, const int* cls = nullptr);
// re-parts every row of nb by nb.cls (see NbrTable); replaces nb.col.  Returns hipError_t as int.
int launch_class_partition(hipStream_t st, int na, NbrTable& nb);
// builds nb from (n_rows, 2) device pairs; scratch (deg/cursor) is managed inside. Returns hipError_t as int.
int build_neighbour_table(hipStream_t st, const Topology& top, int64_t n_rows, const int* pairs_dev, NbrTable& nb,
                          void** scratch, size_t* scratch_bytes);

// ---- md_kernels.hip: harmonic bonded terms and velocity-Verlet half steps of the MD drivers
template <class T>
void launch_md_bonded(hipStream_t st, int nb, const int* bidx, const T* bpar, int na, const int* aidx, const T* apar, const T* pos,
                      const Box<T>& box, T* grad, double* E);
template <class T>
void launch_md_kick_drift(hipStream_t st, int n, T* pos, T* vel, const T* grad, const T* inv_mass, double half_dt_acc, double dt,
                          double* ekin);
// first half of a BAOAB Langevin step (B, A, O, A; noise of md_math.h, stream 0) and the generator written to memory
// (kind 0: (n,4) uint32 words, kind 1: (n,3) T normals)
template <class T>
void launch_md_langevin(hipStream_t st, int n, T* pos, T* vel, const T* grad, const T* inv_mass, double half_dt_acc, double dt,
                        double c1, double c2sq_kT_acc, uint64_t seed, uint64_t step, double* ekin);
template <class T>
void launch_md_random(hipStream_t st, int kind, int64_t n, uint64_t seed, uint64_t step, uint32_t stream, void* out);
// isotropic barostat: S (9 doubles) += sum shift (x) dE/dd over the bond / angle vectors that cross the cell, E as
// launch_md_bonded; out[0..8] += sum m v (x) v, out[9..17] += sum r (x) g, out[18..20] = normals of (seed, step, stream 2,
// atom 0) (launched for n = 0 too); r *= mu, v *= inv_mu
template <class T>
void launch_md_bonded_box(hipStream_t st, int nb, const int* bidx, const T* bpar, int na, const int* aidx, const T* apar,
                          const T* pos, const Box<T>& box, double* E, double* S);
template <class T>
void launch_md_virial(hipStream_t st, int n, const T* pos, const T* vel, const T* grad, const T* inv_mass, uint64_t seed,
                      uint64_t step, double* out);
template <class T>
void launch_md_scale(hipStream_t st, int n, T* pos, T* vel, double mu, double inv_mu);

// ---- mts_kernels.hip: the multiple-time-step integrator, n_inner BAOAB steps on the bonded terms between the half kicks of
// the slow gradient, one workgroup per tile of whole molecules.  MtsTiles: the device copy of an MtsPlan (mts_plan.h; the
// parameters in the handle's precision).  threads = mts_threads(tile capacity), lds_bytes = mts_lds_bytes(dims, sizeof(T)).
template <class T>
struct MtsTiles {
  int n_tiles;
  MtsDims dims;
  const int *tile_atom0, *atom_id, *tile_bond0, *bond_slot, *tile_angle0, *angle_slot, *ref0, *ref;
  const T *bond_par, *angle_par;
};
template <class T>
void launch_md_mts(hipStream_t st, const MtsTiles<T>& P, int threads, size_t lds_bytes, T* pos, T* vel, const T* grad_slow,
                   const T* inv_mass, const Box<T>& box, double half_dt_acc_outer, double dt_outer, int n_inner, double c1,
                   double c2sq_kT_acc, uint64_t seed, uint64_t outer_step, double* E, T* grad_fast);

// ---- con_kernels.hip: pairwise distance constraints (SHAKE on the displacement of the first half of a BAOAB step, RATTLE on
// the velocities of the second, a position projection), one workgroup per tile of whole clusters.  ConTiles: the device copy of
// a ConPlan (con_plan.h; d^2 in the handle's precision).  threads = mts_threads(tile capacity); the launchers size the LDS
// themselves (con_lds_bytes).  counters (optional, device): [0] += clusters that stopped unconverged, [1] = max(sweeps).
template <class T>
struct ConTiles {
  int n_tiles;
  ConDims dims;
  const int *tile_atom0, *atom_id, *tile_clu0, *clu_con0, *con_slot;
  const T* con_d2;
};
template <class T>
void launch_con_step(hipStream_t st, const ConTiles<T>& P, int threads, T* pos, T* vel, const T* grad, const T* inv_mass,
                     const Box<T>& box, double half_dt_acc, double dt, double c1, double c2sq_kT_acc, uint64_t seed, uint64_t step,
                     double tol, int max_sweeps, int* counters);
template <class T>
void launch_con_kick(hipStream_t st, const ConTiles<T>& P, int threads, const T* pos, T* vel, const T* grad, const T* inv_mass,
                     const Box<T>& box, double half_dt_acc, double dt, double tol, int max_sweeps, double* ekin, int* counters);
template <class T>
void launch_con_project(hipStream_t st, const ConTiles<T>& P, int threads, T* pos, const T* ref, const T* inv_mass, const Box<T>& box,
                        double tol, int max_sweeps, int* counters);

// ---- mol_kernels.hip: molecular (centre-of-mass) cell scaling, one workgroup per tile of whole groups.  MolTiles: the device
// copy of a MolPlan (mol_plan.h).  threads = mts_threads(tile capacity); the launchers size the LDS themselves
// (mol_lds_bytes).  out (21 doubles, device): the layout of launch_md_virial with the groups' kinetic tensor and the virial of
// the centres' images; the caller zeroes the first 18 words.
struct MolTiles {
  int n_tiles;
  MolDims dims;
  const int *tile_atom0, *atom_id, *tile_grp0, *grp_atom0, *slot_grp;
};
template <class T>
void launch_md_mol_sums(hipStream_t st, const MolTiles& P, int threads, const T* pos, const T* vel, const T* grad, const T* inv_mass,
                        const Box<T>& box, uint64_t seed, uint64_t step, double* out);
template <class T>
void launch_md_mol_scale(hipStream_t st, const MolTiles& P, int threads, T* pos, T* vel, const T* inv_mass, const Box<T>& box,
                         double mu_minus_1, double inv_mu_minus_1);

// ---- fire_kernels.hip: one iteration of the FIRE minimiser (md_fire_math.h): the six reduced words as one row per workgroup in
// `rows` (>= kFireRowsBytes), then fold + control + update.  state16 (device): two slots of 8 doubles, slot call & 1 is read, the
// other written; n = 0 copies the slot forward.  par9 is read on the host.  Returns hipError_t as int.
constexpr size_t kFireRowsBytes = 256 * 6 * sizeof(double);
template <class T>
int launch_md_fire(hipStream_t st, int n, T* pos, T* vel, const T* grad, const T* inv_mass, const double* par9, double ftol,
                   uint64_t call, double* rows, double* state16);

// ---- vrescale_kernels.hip: one application of the stochastic velocity-rescaling thermostat (md_vrescale_math.h): the closing half
// kick (grad != nullptr) and the kinetic energy as one double per workgroup in `rows` (>= kVrRowsBytes), then fold + rule + scale.
// state16 (device): two slots of 8 doubles, slot call & 1 is read, the other written; n = 0 copies the slot forward.  Returns
// hipError_t as int.
constexpr size_t kVrRowsBytes = 256 * sizeof(double);
template <class T>
int launch_md_vrescale(hipStream_t st, int n, T* vel, const T* grad, const T* inv_mass, double half_dt_acc, int64_t n_dof,
                       double kT_acc, double c, uint64_t seed, uint64_t step, uint64_t call, double* rows, double* state16);

}  // namespace admp
