/* libadmp_hip -- C ABI of the MI355X-native multipolar PME path.
 *
 * The reference (Roy-Kid/ADMP) has no FFI layer: its boundary is the Python callable API of
 * admp/pme.py:30-143 (ADMPPmeForce), admp/disp_pme.py:20-77 (ADMPDispPmeForce) and
 * admp/pairwise.py:45-113 (generate_pairwise_interaction + TT kernel).  This header is the layer
 * BENEATH that API: admp_amd/{pme,disp_pme,pairwise}.py keep the reference's class / method names
 * and bind these entry points through ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 on success or a negative ADMP_E_* code; nothing throws or aborts;
 *     admp_last_error() gives the message of the last failure on that handle.
 *   - `real` arrays are float (precision 4) or double (precision 8), fixed at admp_create.
 *   - array arguments marked [dev|host] are device pointers when `on_device` is non-zero, host
 *     pointers otherwise (the library then stages them); the caller owns every buffer.
 *   - one handle = one GPU + one HIP stream; a handle is not thread-safe, distinct handles are
 *     independent.  Energies are always returned as double, in kJ/mol; lengths in Angstrom.
 */
#ifndef ADMP_HIP_H
#define ADMP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct admp_handle admp_handle;

enum {
  ADMP_OK = 0,
  ADMP_E_ARG = -1,      /* bad argument / call order */
  ADMP_E_HIP = -2,      /* HIP runtime error */
  ADMP_E_FFT = -3,      /* rocFFT error */
  ADMP_E_NOGPU = -4,    /* no usable device */
  ADMP_E_STATE = -5,    /* topology / ewald / pairs not set, or an internal precondition violated */
  ADMP_E_COMM = -6      /* a communicator callback of a slab-decomposed handle failed */
};

/* library version, and the gfx target the kernels were built for ("gfx950") */
const char* admp_version(void);

/* ---- lifetime ------------------------------------------------------------------------------ */
/* replaces: ADMPPmeForce.__init__ (admp/pme.py:37-55) -- device side of the object */
int admp_create(admp_handle** out, int device, int precision /* 4 | 8 */);
int admp_destroy(admp_handle* h);
const char* admp_last_error(const admp_handle* h);
/* run on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int admp_set_stream(admp_handle* h, void* hip_stream);
/* run on the legacy default (null) stream -- what torch.cuda.current_stream() is unless the caller switched streams */
int admp_use_default_stream(admp_handle* h);
int admp_synchronize(admp_handle* h);

/* ---- static environment -------------------------------------------------------------------- */
/* replaces: axis_type / axis_indices / covalent_map ctor arguments (admp/pme.py:37-51,
 * generate_construct_local_frames admp/spatial.py:44-74).  covalent_map is passed in CSR form
 * (row i: atoms j with covalent_map[i,j] = nbonds > 0, nbonds <= 7: ADMP_E_ARG beyond -- the reference's
 * parser marks 1..2, its scale lists have 5 entries); all pointers are HOST pointers.
 * axis_type[i] in 0..5 (ZThenX, Bisector, ZBisect, ThreeFold, Zonly, NoAxisType);
 * axis_idx[i*3 + {0,1,2}] = z, x, y atom (-1 = none). */
int admp_set_topology(admp_handle* h, int n_atoms, const int32_t* axis_type, const int32_t* axis_idx,
                      const int32_t* excl_rowptr, const int32_t* excl_col, const int32_t* excl_nbonds);

/* replaces: the kappa / K1..K3 / lmax / lpol environment (admp/pme.py:42-50, update_env :89-94).  Meshes below 6 points per
 * dimension are accepted here for admp_mesh_convolve alone: every call that spreads or gathers (order-6 splines) refuses them. */
int admp_set_ewald(admp_handle* h, double kappa, int K1, int K2, int K3, int lmax, int lpol);

/* behaviour switches that are not part of the reference's argument lists */
enum {
  ADMP_OPT_REFERENCE_KPOINTS = 1,  /* value 1: build the reciprocal-space tables with the reference's literal k-point order
                                      (meshgrid(kz, kx, ky), admp/recip.py:339-340) instead of the axis-by-axis one; the
                                      two agree iff K1 = K2 = K3 on a cubic box.  Default 0. */
  ADMP_OPT_KEEP_POL_SITES = 2,     /* value 1: the caller vouches that the SET of polarizable sites {i : pol_i > 0} of the
                                      following admp_pme_energy_grad calls is the one of the previous call (the values may
                                      change); the library then keeps its list of those sites instead of rebuilding it in
                                      every call.  Default 0 (rebuild every call).  Speed only, never results. */
  ADMP_OPT_SIDE_STREAM = 3,        /* value 0: every kernel of a call runs on the handle's stream.  Default 1: on systems up to
                                      200 000 atoms the real-space pair kernels run on a second stream next to the mesh chain
                                      of the same call.  Speed only; switched off by measurements that bracket single kernels
                                      with events (the event time of a kernel that shares the chip is not its duration). */
  ADMP_OPT_ASPC_HOLD = 4           /* value 1: while admp_scf_aspc is on, the following admp_pme_energy_grad calls are NOT time
                                      steps: they run as without the mode and leave its history alone (a wrapper that
                                      converges the dipoles ahead of a box or parameter gradient sets it around that call).
                                      Default 0. */
};
int admp_set_option(admp_handle* h, int option, int value);

/* replaces: `pairs = pairs[pairs[:,0] < pairs[:,1]]` + the per-pair gathers of pme_real
 * (admp/pme.py:671-683).  pairs is (n_rows, 2) int32 [dev|host]; rows with i >= j (padding) are
 * dropped.  The list is compiled into an i-grouped neighbour table that stays valid until the
 * next call. */
int admp_set_pairs(admp_handle* h, int64_t n_rows, const int32_t* pairs, int on_device);

/* The calculators of one system (PME, dispersion PME, pair potentials) are handed the SAME pair list by the reference's
 * drivers (examples/water_pol_1024/run_admp.py:117-136: one `pairs` array for every force object).  Instead of compiling
 * that list once per handle, `h` walks the neighbour table of `lender` (same atoms, same covalent map, same device):
 * whatever list the lender holds when `h` is next called -- also after the lender's admp_set_pairs /
 * admp_set_pairs_from_positions.  lender = NULL, or a pair list of its own, ends the loan; calling `h` after the lender
 * was destroyed is ADMP_E_ARG. */
int admp_share_neighbors(admp_handle* h, admp_handle* lender);
int64_t admp_num_pairs(const admp_handle* h);   /* pairs kept (i < j) */
/* Verlet lists with a skin (MD drivers rebuild the list every few steps with rc + skin): pairs of the list whose
 * minimum-image distance is >= rc are skipped by the pair kernels, so that the result is the one of the exact-rc list
 * whatever the skin.  rc = 0 (default): every listed pair is evaluated -- what the reference does with whatever list it is
 * handed (admp/pme.py:671-729 has no distance test).  Honoured by every pair kernel and everything derived from them: the
 * dispersion and Tang-Toennies kernels test each partner (admp_disp_energy_grad, admp_tt_energy_grad, their box gradients,
 * admp_disp_param_grad, admp_tt_param_grad, admp_mscale_grad kinds 1 and 2); a multipolar PME evaluation with rc > 0 first
 * writes the inner table of the table it walks (owned, borrowed or pruned) at its own sites -- the entries below rc, rows in
 * place order, no host synchronisation -- and every pair pass of the call walks that (admp_pme_energy_grad with all its SCF
 * forms, admp_pme_energy_fixed_dipoles, admp_pme_box_grad, admp_thole_sums, admp_pscale_grad; admp_mscale_grad kind 0 tests
 * each partner).  The derivatives are those of the energy the calculator returns. */
int admp_set_cutoff(admp_handle* h, double rc);
/* MD loops with a Verlet skin (no counterpart in the reference, which evaluates whatever list it is given): until the next
 * list build the calculators of `h` -- and of every handle that borrows its table -- walk an INNER table: the entries of the
 * current one whose minimum-image distance at `positions` (DEVICE pointer, (Na,3) real) is below rc, rows compacted in place
 * order.  A driver that rebuilds the outer list (rc + skin) every n steps prunes it to rc + skin_inner every m < n steps,
 * skin_inner = twice what an atom can move in m steps: the multipolar kernels then do (rc + skin_inner)^3 / (rc + skin)^3 of
 * the work, and so do the cutoff-testing dispersion / pair-potential kernels.  Without admp_set_cutoff the multipolar kernels
 * evaluate every entry of the inner table (pairs between rc and rc + skin_inner included); with it they walk the entries below
 * rc of the inner table, and pruning only saves the per-call pass that finds them.  Pruning
 * always starts from the table as built; rc <= 0 goes back to it.  Single-rank handles that own their table.  One host
 * synchronisation. */
int admp_prune_pairs(admp_handle* h, const void* positions, const double* box, double rc);
/* One shot, device pointers only: the NEXT admp_pme_energy_grad reads its initial dipoles from U_init ((Na,3), read-only) and
 * uses U_inout purely as output (it starts as a copy made by the first kernel of the evaluation).  The reference's callers
 * pass `U_init=pme.U_ind` and get a new array back (admp/pme.py:104-109: jnp arrays are immutable): with this entry the
 * wrapper hands over a fresh output array without a device copy of its own.  NULL clears it. */
int admp_set_dipole_source(admp_handle* h, const void* U_init);

/* ---- the hot path -------------------------------------------------------------------------- */
/* replaces: ADMPPmeForce.get_energy / get_forces (admp/pme.py:58-86, 108) including the induced
 * dipole SCF optimize_Uind (admp/pme.py:111-143) when the handle is polarizable.
 *   positions  (Na,3) real [dev|host]         box        9 doubles, lattice vectors in rows (host)
 *   Q_local    (Na,9) real [dev|host]         harmonics [00,10,11c,11s,20,21c,21s,22c,22s], zero-padded above lmax
 *   pol,tholes (Na) real [dev|host]           NULL unless polarizable
 *   mScales/pScales/dScales                   n_scales doubles each (host); index (nbonds-1) wraps like the reference
 *   U_inout    (Na,3) real [dev|host]         in: SCF start (global Cartesian), out: converged dipoles; NULL unless polarizable
 *   max_cycle, thresh                         MAX_N_POL / POL_CONV of admp/settings.py:29-30
 *   E_out[4]                                  real-space, reciprocal, self, polarization penalty
 *   dE_dpos    (Na,3) real [dev|host]         +dE/dpositions (the reference returns the gradient, not the force); may be NULL (energy only)
 *   dE_dQlocal (Na,9) real [dev|host]         optional (NULL to skip)
 *   n_cycle, converged                        loop index at exit and `i != max_cycle-1` (admp/pme.py:139-143) */
int admp_pme_energy_grad(admp_handle* h, const void* positions, const double* box, const void* Q_local,
                         const void* pol, const void* tholes, int n_scales, const double* mScales,
                         const double* pScales, const double* dScales, void* U_inout, int max_cycle, double thresh,
                         double* E_out, void* dE_dpos, void* dE_dQlocal, int* n_cycle, int* converged,
                         int on_device);

/* replaces: ADMPPmeForce.energy_fn / grad_U_fn / grad_pos_fn (admp/pme.py:69-78): the bare polarizable energy with the
 * induced dipoles as an explicit input (no SCF), and its derivatives with respect to positions, dipoles and Q_local.
 * All array arguments are DEVICE pointers; U (Na,3) global Cartesian; dE_dpos / dE_dU / dE_dQlocal may each be NULL.
 * dE_dU is the "field" of optimize_Uind (admp/pme.py:133): real + reciprocal + self + polarization-penalty terms.
 * On a slab-decomposed handle (round 4): U must be valid on the rank's home rows (the rows it reads of other ranks are fetched
 * from their owners into a copy); dE_dpos / dE_dU / dE_dQlocal hold the home rows, E_out the global energies. */
int admp_pme_energy_fixed_dipoles(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                         const void* tholes, int n_scales, const double* mScales, const double* pScales, const void* U,
                         double* E_out, void* dE_dpos, void* dE_dU, void* dE_dQlocal);

/* replaces: jax.value_and_grad(get_energy, argnums=1) -- the gradient of the energy with respect to the cell matrix at FIXED
 * Cartesian positions, from which callers of the reference form the virial (README.md:7; admp/pme.py:108 and
 * admp/disp_pme.py:76 with argnums).  dE_dbox is 9 doubles (host), row-major like `box` (lattice vectors in rows).
 * Positions / parameters are DEVICE pointers.  For a polarizable handle U holds the induced dipoles to evaluate at (the
 * converged ones: the reference differentiates energy_fn at stop_gradient(U_ind), admp/pme.py:81-85).
 * E_out as in the corresponding energy_grad call.  All three also run on a slab-decomposed handle (round 4: every rank returns
 * the full gradient; the device sums are added over the ranks). */
int admp_pme_box_grad(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                      const void* tholes, int n_scales, const double* mScales, const double* pScales, const void* U,
                      double* E_out, double* dE_dbox);
int admp_disp_box_grad(admp_handle* h, const void* positions, const double* box, const void* c_list, int pmax, int n_scales,
                       const double* mScales, double* E_out, double* dE_dbox);
int admp_tt_box_grad(admp_handle* h, const void* positions, const double* box, const void* abqc, int n_scales,
                     const double* mScales, double* E_out, double* dE_dbox);

/* replaces: the `construct_local_frames(positions, box)` attribute (generate_construct_local_frames,
 * admp/spatial.py:44-142): frames_out (Na,3,3) real, rows = local x, y, z axes in the global frame.  DEVICE pointers.
 * Diagnostic only -- the hot path builds the frames inside its first kernel and never materialises them. */
int admp_local_frames(admp_handle* h, const void* positions, const double* box, void* frames_out);

/* No counterpart in the reference: the dipole observable of a multipolar, polarizable model -- molecular (per-group) dipoles and
 * the cell dipole M, split into their charge, permanent-dipole and induced parts (admp_amd/csrc/dipole_math.h, dipole_kernels.hip).
 * Groups are sets of atoms narrower than half the cell (the labels of admp_amd.md.groups_of); the anchor a of a group is its
 * lowest-numbered atom, and atoms may be wrapped into the cell independently.  For atom i of group c:
 *   d_i  = minimum image of r_i - r_a (exactly r_i - r_a when no translation was applied),  D_c = sum m_i d_i / M_c
 *   p_i  = x_loc X_i + y_loc Y_i + z_loc Z_i with (z_loc, x_loc, y_loc) = Q_local[i, 1:4] (harmonics 10, 11c, 11s) and X_i, Y_i,
 *          Z_i the rows of the atom's local frame (what admp_local_frames returns)
 *   U_i  = the induced dipole (global Cartesian); zero when U is NULL
 *   mu_c = sum_i [ q_i (d_i - D_c) + p_i + U_i ],  q_i = Q_local[i, 0];   M = sum_c mu_c
 * A neutral group's mu_c does not depend on the origin, a charged group's is taken about its centre of mass, a single atom gives
 * p_i + U_i.  The itinerant term q_c R_c of charged groups is NOT part of M: it is not defined under periodic boundaries.
 * Unit: that of Q_local -- e A for positions in A (1 e A = 4.80320471 D).
 *   positions (Na,3), Q_local (Na,9), U (Na,3; may be NULL), inv_mass (Na) 1/m_i: real of the handle's precision, DEVICE pointers
 *   box               9 HOST doubles, lattice vectors in rows
 *   group_start_dev   (n_groups + 1) int32, group_atoms_dev (Na) int32, DEVICE pointers: group c is the atoms
 *                     group_atoms[group_start[c] .. group_start[c + 1]), ascending, so that the anchor comes first; a group has no
 *                     size cap.  An index outside 0 .. Na - 1 is passed over, a range outside 0 .. Na makes an empty group.
 *   mu_groups_dev     (n_groups,3) doubles, DEVICE pointer, may be NULL: mu_c
 *   out16_dev         16 doubles, DEVICE pointer: [0..2] charge part of M, [3..5] permanent part, [6..8] induced part,
 *                     [9] sum_c |mu_c|, [10] sum_c |mu_c|^2, [11] max_c |mu_c|, [12] n_groups, [13..15] 0
 * The frames and d_i are formed in the handle's precision; every product and sum runs in double.  Two kernels on the handle's
 * stream, no atomics (the 16 words and mu_c are the same bit for bit from run to run), no host synchronisation: an MD loop can
 * record a row per step and read them when the run ends.  n_groups = 0 launches nothing and zeroes out16_dev on the stream.
 * ADMP_E_ARG, before anything is launched, for a NULL required pointer, n_groups < 0, or a singular or non-finite box;
 * ADMP_E_STATE without a topology (admp_set_topology) or on a slab-decomposed handle. */
int admp_pme_dipoles(admp_handle* h, const void* positions, const double* box, const void* Q_local,
                     const void* U /* may be NULL */, const void* inv_mass, int n_groups, const int32_t* group_start_dev,
                     const int32_t* group_atoms_dev, double* mu_groups_dev /* (n_groups,3), may be NULL */, double* out16_dev);

/* replaces: ADMPDispPmeForce.get_energy / get_forces (admp/disp_pme.py:44-77, 80-279).
 *   c_list (Na,3) real: C6, C8, C10 per atom (columns above pmax ignored); E_out[3] = real, recip, self */
int admp_disp_energy_grad(admp_handle* h, const void* positions, const double* box, const void* c_list, int pmax,
                          int n_scales, const double* mScales, double* E_out, void* dE_dpos, int on_device);

/* Optional hint for admp_disp_energy_grad (no counterpart in the reference, which spreads every channel's coefficients,
 * admp/disp_pme.py:80-123): the rows of c_list take only n_types <= 3 distinct values (atom types: water has two).
 *   type_of_atom  (Na) int32, DEVICE pointer owned by the caller (must stay valid until replaced): row index of every atom
 *   coefficients  (n_types,3) host doubles: the distinct rows (C6, C8, C10)
 * A single-rank handle on a power-of-two mesh in single precision then keeps one mesh per TYPE instead of one per channel
 * (S_p(k) = sum_t c_p,t S_t(k): one spread and one gather per atom, n_types transforms each way, the channels combined per k
 * point) -- the same sums regrouped.  Every call that uses the table checks it against c_list and fails with ADMP_E_ARG on a
 * mismatch.  n_types = 0 (or NULL): forget the table.  Other handles ignore it. */
int admp_disp_set_types(admp_handle* h, int n_types, const void* type_of_atom, const double* coefficients);

/* replaces: generate_pairwise_interaction(TT_damping_qq_c6_kernel, ...) (admp/pairwise.py:45-113).
 *   abqc (Na,4) real: a, b, q, c6 per atom */
int admp_tt_energy_grad(admp_handle* h, const void* positions, const double* box, const void* abqc, int n_scales,
                        const double* mScales, double* E_out, void* dE_dpos, int on_device);

/* replaces: generate_pairwise_interaction(pair_int_kernel, covalent_map, static_args) for an ARBITRARY kernel
 * (admp/pairwise.py:45-91): the Python layer traces `pair_int_kernel(dr, m, p1i, p1j, ...)` once into HIP source
 * (admp_amd/xp.py: one statement per arithmetic operation, d/d(dr) by forward-mode dual numbers) and this call compiles
 * it for gfx950 with hiprtc and loads it.  The source must define
 *   extern "C" __global__ void admp_pair_custom(int na, const int* rowptr, const int* col, const int* order,
 *       const REAL_T* pos, const REAL_T* par, const REAL_T* box18, const REAL_T* mscale16, REAL_T* grad, double* energy)
 * (REAL_T is defined on the command line as the handle's precision).  program_id receives a handle-local id. */
int admp_pair_program_build(admp_handle* h, const char* hip_source, int n_params, int* program_id);
/* energy and +dE/dpositions of a built program on the current pair list; params (Na, n_params) real [dev|host],
 * other arguments as admp_tt_energy_grad; E_out[1] */
int admp_pair_program_energy_grad(admp_handle* h, int program_id, const void* positions, const double* box,
                                  const void* params, int n_scales, const double* mScales, double* E_out, void* dE_dpos,
                                  int on_device);

/* replaces: jax.grad(potential, argnums=3)(...)['mScales'] of the reference's parameter-gradient example
 * (examples/openmm_api/run.py:41-46): dE/dmScales[k], k = 0..n_scales-1, of one calculator on the current pair list.
 *   kind 0  multipolar PME         params = Q_local (Na,9) real   (admp/pme.py:681-683: mscales = mScales[nbonds-1])
 *   kind 1  dispersion PME         params = c_list  (Na,3) real, pmax as in admp_disp_energy_grad
 *   kind 2  Tang-Toennies damping  params = abqc    (Na,4) real
 * The pair energy is linear in the scale factor, so the result does not depend on the current mScales values (nor, for a
 * polarizable handle, on the induced dipoles: the induced terms carry pScales).  positions / params [dev|host]. */
int admp_mscale_grad(admp_handle* h, int kind, const void* positions, const double* box, const void* params, int pmax,
                     int n_scales, double* dE_dmScales, int on_device);

/* replaces: the 'C6' / 'C8' / 'C10' and 'A' / 'B' / 'Q' entries of jax.grad(pot_disp, argnums=3) of the reference's
 * dispersion front-end (examples/openmm_api/run.py:41-43 through admp/api.py:183-199), at the level of the per-ATOM lists the
 * calculators take (the caller chains them to its per-type tables and unit conversions, admp_amd/api.py):
 *   admp_disp_param_grad   dE_dc (Na,3) real = d(E_real + E_recip + E_self)/dc_list of admp_disp_energy_grad
 *   admp_tt_param_grad     dE_dabqc (Na,4) real = dE/d(a, b, q, c6) of admp_tt_energy_grad; an atom whose a or b is zero gets 0
 *                          for that entry (the geometric mean sqrt(a_i a_j) has no finite derivative there: NaN in autodiff)
 * All array arguments are DEVICE pointers.  On a slab-decomposed handle (round 4) the rows of the rank's home atoms are filled
 * (per-atom outputs, like the gradient); the class sums of admp_mscale_grad / admp_pscale_grad are added over the ranks. */
int admp_disp_param_grad(admp_handle* h, const void* positions, const double* box, const void* c_list, int pmax, int n_scales,
                         const double* mScales, void* dE_dc);
int admp_tt_param_grad(admp_handle* h, const void* positions, const double* box, const void* abqc, int n_scales,
                       const double* mScales, void* dE_dabqc);

/* replaces: the 'pol' / 'tholes' entries of jax.grad(pot_pme, argnums=3) (parameter gradients of the polarizable model).
 * The polarizabilities and Thole parameters enter the pair energy only through the Thole argument
 * au = a_w r / (alpha_i alpha_j)^(1/6) (admp/pme.py:408-414).  This call returns, for the induced dipoles U given
 * (normally the converged ones), the per-atom sums
 *   sumX[i]  = sum_j dE_ij / d ln(au_ij)            -> dE/dalpha_i = -sumX[i] / (6 alpha_i) - D |U_i|^2 / (2 alpha_i^2)
 *   sumXw[i] = sum_j dE_ij / d ln(au_ij) (1 - w0_ij) / a_w,ij   -> dE/dthole_i = sumXw[i]
 * (the closing formulas are applied by the caller, admp_amd/pme.py).  All array arguments are DEVICE pointers. */
int admp_thole_sums(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                    const void* tholes, int n_scales, const double* mScales, const double* pScales, const void* U,
                    void* sumX, void* sumXw);

/* replaces: the 'pScales' entry of jax.grad(pot_pme, argnums=3): dE/dpScales[k], k = 0..n_scales-1, at the induced dipoles U
 * given (DEVICE pointers).  pscale multiplies the Thole factor of the permanent-induced coefficients (admp/pme.py:455-470);
 * its second role, the Fermi switch of the Thole width (pme.py:411), has a derivative below 1e-38 wherever it is finite
 * and is NaN in the reference's autodiff for pscale > ~0.008 (exp overflow): the analytic limit 0 is used.  The 'dScales'
 * entry is identically zero (the reference ignores dScales, uscales = 1, pme.py:472). */
int admp_pscale_grad(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                     const void* tholes, int n_scales, const double* mScales, const double* pScales, const void* U,
                     double* dE_dpScales);

/* ---- neighbour search ("next" row of SURVEY.md 8f) --------------------------------------------------------
 * replaces: jax_md.partition.neighbor_list(displacement_fn, box, rc, 0, format=OrderedSparse).allocate(positions)
 * of the reference's drivers (examples/water_1024/run_admp.py:109-112): the producer of `pairs`.
 * Cell list on the GPU, any lattice with rc <= half of every box height.  Two phases so the caller can size
 * the output: count -> allocate (n_pairs, 2) int32 on the device -> fill (rows i < j, grouped by i, j ascending
 * within a cell sweep).  positions is a DEVICE pointer to (n_atoms, 3) reals and must stay valid until fill.
 *   Empty list: no pair within rc (one atom, a dilute gas) is a valid answer.  count then reports 0, and fill accepts a
 *   NULL pairs_out (a zero-row device array has no address), writes nothing and ends the pending count like any fill;
 *   NULL after a non-zero count is ADMP_E_ARG.  A handle may be given a new topology of any size afterwards (the search's
 *   scratch is sized per call, tests/test_gpu_neighbour.py).
 *   Covalent classes: the table entries built by admp_set_pairs / admp_set_pairs_from_positions carry the class of
 *   admp_set_topology in three bits, so classes are 0..7 (admp_amd._device.covalent_to_csr refuses more).
 *   Precision: a pair is listed when the minimum-image distance EVALUATED IN THE HANDLE'S PRECISION (min_image: d = r_i - r_j,
 *   s = d box^-1, d = (s - floor(s + 1/2)) box) is below rc.  In double this is the float64 reference's set exactly.  In
 *   single a pair may be classified differently only within band = 8 * 2^-24 * (max |position component| + largest column
 *   sum of |box|) of rc (inputs rounded to f32, one subtraction, two 3-term products); measured margins: profiles/README.md. */
int admp_neighbor_count(admp_handle* h, int n_atoms, const void* positions, const double* box, double rc,
                        int64_t* n_pairs);
int admp_neighbor_fill(admp_handle* h, int32_t* pairs_out);
/* search + admp_set_pairs fused: builds the handle's neighbour table (all pairs with minimum-image r < rc) straight
 * from DEVICE positions (n_atoms of admp_set_topology), without materialising the pair array. */
int admp_set_pairs_from_positions(admp_handle* h, const void* positions, const double* box, double rc);

/* ---- MD-driver helpers ("next" row f2 of SURVEY.md 8f; the reference has no integrator) -------------------
 * replaces: nothing in the reference -- its drivers stop at get_forces.  What an MD loop around the hot path needs besides
 * it, as device kernels so that a step does not pay dozens of framework launches: the harmonic bonded terms of the drivers'
 * force field (examples/water_1024/mpidwater.xml:16-21: HarmonicBondForce E = k/2 (r - r0)^2, HarmonicAngleForce E = k/2
 * (theta - theta0)^2) over explicit lists, and the half steps of velocity Verlet.  All pointers are DEVICE pointers
 * (box: host); nothing is read back -- energies accumulate into device words the caller reads when it logs.
 *   admp_md_bonded      bond_idx (n_bonds,2) int32, bond_par (n_bonds,2) real = (k, r0); angle_idx (n_angles,3) int32 = (i,
 *                       centre, k), angle_par (n_angles,2) real = (k, theta0 in rad); minimum-image vectors;
 *                       E_dev[0] += bond energy, E_dev[1] += angle energy (doubles); grad_inout (Na,3) real += dE/dr
 *   admp_md_kick_drift  v -= half_dt_acc * grad / m (grad = +dE/dr, inv_mass (Na) real); then, if dt != 0, r += dt * v;
 *                       ekin_dev (optional) += sum m v^2 / 2 after the kick, in the caller's units
 *   admp_md_langevin    first half of a BAOAB Langevin step in one pass: v -= half_dt_acc * grad / m; r += dt/2 * v;
 *                       v = c1 * v + sqrt(c2sq_kT_acc / m) * xi; r += dt/2 * v, with c1 = exp(-gamma dt) in [0, 1] and
 *                       c2sq_kT_acc = (1 - c1^2) kB T in the units of v^2 m (>= 0), both from the host in double; xi: three
 *                       standard normals per atom, a function of (seed, step, stream 0, atom index) alone (Philox-4x32-10,
 *                       Box-Muller in double: csrc/md_math.h), so a restart at `step` draws the same noise.  ekin_dev
 *                       (optional) += sum m v^2 / 2 after the friction step.  The second half of the step is
 *                       admp_md_kick_drift with dt = 0.
 *   admp_md_random      the same generator written to memory: kind 0: out (n,4) uint32, the raw words; kind 1: out (n,3)
 *                       real, the normals; counter = (atom, step low, step high, stream), key = (seed low, seed high)
 *   admp_md_bonded_box  the box-gradient pass of admp_md_bonded (same lists): for every bond and angle vector the lattice
 *                       translation of the minimum image, shift = d_min - d_raw; S_dev (9 doubles, row-major) +=
 *                       sum shift^T (x) dE/dd; E_dev[0..1] += the energies as above; no gradient is written.  The caller
 *                       forms dE/dbox = box^-T S (fixed Cartesian positions).  ADMP_E_ARG for a singular or non-finite box.
 *   admp_md_virial      one pass over the atoms for what a pressure needs: out_dev (21 doubles, zeroed by the call):
 *                       [0..8] = sum_i v_i (x) v_i / inv_mass_i, [9..17] = sum_i r_i (x) grad_i, [18..20] = the three normals
 *                       of (seed, step, stream 2, atom 0) in double.  Products and sums in double on both precisions.
 *                       n_atoms = 0 writes zeros and the normals.
 *   admp_md_scale       r *= mu, v *= 1 / mu in place (isotropic cell rescaling; the caller scales its box); mu from the
 *                       host in double, rounded to the handle's precision once.  ADMP_E_ARG unless mu is finite and > 0.
 *   admp_md_mts_plan    the plan of the multiple-time-step integrator (csrc/mts_plan.h) from HOST lists in the layout of
 *                       admp_md_bonded with HOST double parameters: the connected components of the bond and angle lists
 *                       (an atom in no item is one of its own) packed whole into tiles of at most tile_atoms atoms, one
 *                       workgroup each; tile_atoms 0 selects the library's default, which is also the maximum: 256.  The plan's
 *                       device arrays live on the handle and replace an earlier plan (the call waits for the handle's
 *                       stream).  ADMP_E_ARG, with admp_last_error naming the size and the smallest atom, for a component
 *                       larger than tile_atoms; also for an index out of range or a tile whose items exceed 64 KiB of LDS.
 *                       Duplicate items and items in any order are legal.
 *   admp_md_mts_step    one outer step of impulse multiple time stepping (two-level r-RESPA, as OpenMM's
 *                       MTSLangevinIntegrator) up to the calculators, in ONE launch: v -= half_dt_acc_outer * grad_slow / m;
 *                       then n_inner BAOAB steps of length dt_outer / n_inner on the planned bonded terms, each
 *                       v -= (half_dt_acc_outer / n_inner) f / m; r += half v; v = c1 v + sqrt(c2sq_kT_acc / m) xi;
 *                       r += half v; f = bonded gradient at r; v -= ... f / m, with c1 = exp(-gamma dt_outer / n_inner) and
 *                       c2sq_kT_acc as in admp_md_langevin.  xi of inner step k of outer step s: the normals of (seed,
 *                       s * n_inner + k modulo 2^64, stream 0, atom) -- with n_inner = 1 the noise of admp_md_langevin; c1 = 1
 *                       draws nothing.  The closing half kick is admp_md_kick_drift with dt = 0 and the gradient of the
 *                       calculators at the new positions.  Forces are summed in the order of the caller's lists, bonds before
 *                       angles, without float atomics: r and v are bit-identical from run to run and for every tile_atoms.
 *                       Optional, from the bonded evaluation at the returned positions: E_dev[0] += bond energy, E_dev[1] +=
 *                       angle energy (doubles); grad_fast_out (Na,3) real = the bonded gradient.  box: host, 9 doubles.
 *                       ADMP_E_ARG for n_inner < 1, a step without a plan, or n_atoms other than the plan's.
 *   admp_md_mts_info    out8: tiles, tile capacity, largest component, atoms, bonds, angles, LDS bytes per workgroup, launches
 *                       so far (zeros but for the launches on a handle without a plan)
 *   admp_md_con_plan    the plan of the distance constraints (csrc/con_plan.h) from HOST lists: pairs (n, 2) int32, lengths (n)
 *                       double in A.  The connected components of the list ("clusters"; an atom in no constraint is one of its
 *                       own) are packed whole into tiles of at most tile_atoms atoms, one workgroup each; tile_atoms 0 selects
 *                       the library's default, which is also the maximum: 256.  A cluster's constraints are swept in the
 *                       caller's order by one lane, without float atomics: results are bit-identical from run to run and for
 *                       every tile_atoms.  The plan lives on the handle and replaces an earlier one (the call waits for the
 *                       handle's stream).  ADMP_E_ARG, with admp_last_error naming the offender, for an index out of range,
 *                       i == j, a length that is not positive and finite, a cluster larger than tile_atoms (size and smallest
 *                       atom named) or a tile that needs more than 64 KiB of LDS.  Duplicates are kept.
 *   admp_md_con_step    first half of a constrained BAOAB step (the splitting of OpenMM's LangevinMiddleIntegrator) in ONE
 *                       launch: v -= half_dt_acc grad / m; delta = (dt/2) v; v = c1 v + sqrt(c2sq_kT_acc / m) xi (the normals of
 *                       (seed, step, stream 0, atom); c1 = 1 draws nothing); delta += (dt/2) v; SHAKE on delta with the
 *                       directions s_ij of the old positions: sweeps of g = (d^2 - |p|^2) / (2 (1/m_i + 1/m_j) s.p),
 *                       p = s + delta_j - delta_i, delta_i -= (g/m_i) s, delta_j += (g/m_j) s until every |d^2 - |p|^2| <=
 *                       2 tolerance d^2; v += (delta - delta_unconstrained) / dt; r += delta.  box: host, 9 doubles.
 *   admp_md_con_kick    second half: v -= half_dt_acc grad / m at the new positions, then RATTLE: sweeps of k = s.(v_j - v_i) /
 *                       (|s|^2 (1/m_i + 1/m_j)), v_i += (k/m_i) s, v_j -= (k/m_j) s until every |s.(v_j - v_i)| dt <=
 *                       tolerance d^2.  half_dt_acc = 0 with grad NULL is a pure velocity projection.  ekin_dev (optional) +=
 *                       sum m v^2 / 2 of the result, as admp_md_kick_drift.
 *   admp_md_con_project positions moved onto the constraints by the SHAKE sweeps along the directions s_ij of `reference`
 *                       (which may be `positions` itself); no velocities.
 *                       All three stop after max_sweeps sweeps whatever happens; a cluster that stops unconverged, or whose
 *                       SHAKE update meets s.p <= 0 (skipped), adds 1 to counters_dev[0]; counters_dev[1] = max(itself, the
 *                       sweeps of any cluster) (two int32 device words, optional).  ADMP_E_ARG for a call without a plan,
 *                       n_atoms other than the plan's, tolerance < 0, max_sweeps < 1 or dt <= 0.
 *   admp_md_con_info    out8: tiles, tile capacity, largest cluster, atoms, constraints, clusters, LDS bytes per workgroup (of
 *                       the projection, the largest), launches so far (zeros but for the launches without a plan)
 *   admp_md_mol_plan    the plan of the molecular (centre-of-mass) cell scaling (csrc/mol_plan.h) from a HOST array:
 *                       group_of (n_atoms) int32 labels >= 0, every atom in exactly one group ("molecule"; a singleton is a
 *                       group); the labels need not be dense or ordered.  Groups are taken in the order of their smallest
 *                       atom -- the group's anchor a -- and packed whole into tiles of at most tile_atoms atoms, one workgroup
 *                       each; tile_atoms 0 selects the library's default, which is also the maximum: 256.  The plan has a slot
 *                       of its own on the handle, next to those of admp_md_mts_plan and admp_md_con_plan, and replaces an
 *                       earlier one (the call waits for the handle's stream).  ADMP_E_ARG, with admp_last_error naming the
 *                       offender, for a negative label, a group larger than tile_atoms (size and smallest atom named) or
 *                       tile_atoms outside 0..256.
 *                       With d_i = minimum image of r_i - r_a and s_i = (r_i - r_a) - d_i (the lattice translation the image
 *                       applied, exactly zero when none was; groups are smaller than half the cell, atoms may be wrapped one
 *                       by one): R_c = r_a + sum m_i d_i / M, V_c = sum m_i v_i / M, R_c(i) = R_c + s_i.  M, sum m d and
 *                       sum m v are summed in double by one lane per group in the plan's order, without float atomics.
 *   admp_md_mol_sums    what the molecular pressure needs, in the layout and units of admp_md_virial: out21_dev (21 doubles,
 *                       zeroed by the call): [0..8] = sum over groups M_c V_c (x) V_c, [9..17] = sum_i R_c(i) (x) grad_i,
 *                       [18..20] = the three normals of (seed, step, stream 2, atom 0).  box: host, 9 doubles.
 *   admp_md_mol_scale   one application with factor mu (the caller scales its box): r_i += (mu - 1) R_c(i), v_i += (1/mu - 1)
 *                       V_c in place -- a group moves rigidly.  mu_minus_1 and inv_mu_minus_1 from the host in double (expm1);
 *                       the products are rounded to the handle's precision once, so atoms of a group in the same image receive
 *                       bitwise the same displacement.  No atomics: r and v are bit-identical from run to run and for every
 *                       tile_atoms.  ADMP_E_ARG unless both are finite and > -1 and belong to one mu.
 *                       Both: ADMP_E_ARG for a call without a plan, n_atoms other than the plan's, a singular or non-finite box.
 *   admp_md_mol_info    out8: tiles, tile capacity, largest group, atoms, groups, LDS bytes per workgroup, lanes of a
 *                       workgroup, launches so far (zeros but for the launches without a plan)
 *   admp_md_fire_step   one iteration of the FIRE energy minimiser (Bitzek et al. 2006, with the half step back of FIRE 2.0,
 *                       Guenole et al. 2020; semi-implicit Euler; hard displacement cap; the rule is csrc/md_fire_math.h) in two
 *                       launches, its decision logic on the device, nothing read back.  With F = -grad and w_i = 1e-4 inv_mass_i
 *                       six words are reduced in double on both precisions, without atomics (one row per workgroup, folded in a
 *                       fixed order): Fv = sum F.v, FF = sum |F|^2, vv = sum |v|^2, vmax = max |v|, fmax = max |F|, amax =
 *                       max w |F|.  A word that is not finite sets flag 2 (failed): nothing moves, in this call or any later one,
 *                       until the caller writes a fresh state.  fmax <= ftol sets flag 1 (done): nothing moves; a later call with
 *                       a larger fmax resumes.  Fv > 0: a = 1 - alpha, b = alpha sqrt(vv / FF), back = 0, n_pos += 1, and if
 *                       n_pos > n_delay: dt = min(dt f_inc, dt_max), alpha *= f_alpha (a and b keep the old alpha); vb = a vmax +
 *                       b fmax.  Otherwise: a = b = 0, back = dtv_last / 2, n_pos = 0, dt *= f_dec if that stays >= dt_min, alpha
 *                       = alpha_start, vb = 0, uphill steps += 1.  dtv = min(dt, 2 max_step / (vb + sqrt(vb^2 + 4 amax
 *                       max_step))), the largest step with dtv vb + dtv^2 amax <= max_step; dtv_last = dtv; iterations += 1.
 *                       Per atom, the four coefficients rounded to the handle's precision once: x -= back v; v = a v + b F;
 *                       v += dtv w F; x += dtv v -- no atom's forward move exceeds max_step.
 *                       params9 (HOST) = dt_start (not read by the step), dt_max, dt_min, max_step, n_delay, f_inc, f_dec,
 *                       alpha_start, f_alpha.  state16_dev (DEVICE, the caller's): two slots of 8 doubles = dt, alpha, n_pos,
 *                       dtv_last, fmax, iterations, uphill steps, flags; the call reads slot call & 1 and writes slot
 *                       (call + 1) & 1 in full (a frozen call copies it forward), `call` being the caller's call counter.  For a
 *                       given n positions, velocities and state are functions of the inputs alone, bit for bit.  n_atoms = 0
 *                       launches nothing and copies the slot forward on the stream.  ADMP_E_ARG for a null pointer, n_atoms < 0,
 *                       dt_min, dt_max or max_step not finite and positive, dt_min > dt_max, f_inc < 1, f_dec, alpha_start or
 *                       f_alpha outside (0, 1], n_delay < 0, ftol negative or not finite -- and for a slab-decomposed handle.
 *   admp_md_vrescale    one application of the stochastic velocity-rescaling thermostat (Bussi, Donadio, Parrinello 2007; the rule
 *                       is csrc/md_vrescale_math.h) in two launches, its draw and its decision on the device, nothing read back.
 *                       With grad != NULL the first launch makes the closing half kick of a step, v -= half_dt_acc grad inv_mass
 *                       -- admp_md_kick_drift with dt = 0, bit for bit -- before it sums; grad = NULL is the thermostat alone.
 *                       K = sum v^2 / inv_mass / 2 of those velocities is reduced in double on both precisions, without atomics
 *                       (one double per workgroup, folded in a fixed order).  With c = exp(-dt / tau) and kT_acc = 1e-4 kB T:
 *                       K' = (sqrt(c K) + sqrt((1 - c) kT_acc / 2) R1)^2 + (1 - c) (kT_acc / 2) S, R1 ~ N(0, 1), S ~ chi^2(n_dof
 *                       - 1), both functions of (seed, step) alone on stream 3 of the generator (S through a gamma deviate by
 *                       rejection, at most 64 tries); alpha = sqrt(K' / K), rounded to the handle's precision once; v *= alpha.
 *                       K = 0 and c = 1 draw nothing: alpha = 1 exactly.  state16_dev (DEVICE, the caller's): two slots of 8
 *                       doubles = K before, K after (= alpha^2 K with the rounded alpha), alpha, heat = the accumulated sum of
 *                       (K after - K before), applications, tries of the last draw, 0, flags; the call reads slot call & 1 and
 *                       writes slot (call + 1) & 1 in full, `call` being the caller's call counter.  A K or a factor that is not
 *                       finite, or a draw out of tries, sets flag 1 (failed): nothing is scaled, in this call or any later one,
 *                       and words 0-6 are carried over, until the caller writes a fresh state.  Energies in the internal unit
 *                       (kJ/mol times 1e-4).  For a given n velocities and state are functions of the inputs alone, bit for bit.
 *                       n_atoms = 0 launches nothing and copies the slot forward on the stream.  ADMP_E_ARG for a null
 *                       state pointer, a null velocities or inv_mass pointer (unless n_atoms = 0: an empty device array has no
 *                       address), n_atoms < 0, n_dof < 1, c outside [0, 1] or not finite, kT_acc negative or not finite,
 *                       half_dt_acc not finite.
 * All but the first two set the handle's device, check their launch, and refuse slab-decomposed handles (ADMP_E_STATE;
 * admp_md_fire_step: ADMP_E_ARG); admp_md_bonded_box and all after it check every argument (n < 0 included) before anything is
 * launched. */
int admp_md_bonded(admp_handle* h, const void* positions, const double* box, int n_bonds, const int32_t* bond_idx,
                   const void* bond_par, int n_angles, const int32_t* angle_idx, const void* angle_par, double* E_dev,
                   void* grad_inout);
int admp_md_kick_drift(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* grad, const void* inv_mass,
                       double half_dt_acc, double dt, double* ekin_dev);
int admp_md_langevin(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* grad, const void* inv_mass,
                     double half_dt_acc, double dt, double c1, double c2sq_kT_acc, uint64_t seed, uint64_t step,
                     double* ekin_dev);
int admp_md_random(admp_handle* h, int kind, int64_t n, uint64_t seed, uint64_t step, uint32_t stream, void* out);
int admp_md_bonded_box(admp_handle* h, const void* positions, const double* box, int n_bonds, const int32_t* bond_idx,
                       const void* bond_par, int n_angles, const int32_t* angle_idx, const void* angle_par, double* E_dev,
                       double* S_dev);
int admp_md_virial(admp_handle* h, int n_atoms, const void* positions, const void* velocities, const void* grad,
                   const void* inv_mass, uint64_t seed, uint64_t step, double* out_dev);
int admp_md_scale(admp_handle* h, int n_atoms, void* positions, void* velocities, double mu);
int admp_md_mts_plan(admp_handle* h, int n_atoms, int n_bonds, const int32_t* bond_idx, const double* bond_par, int n_angles,
                     const int32_t* angle_idx, const double* angle_par, int tile_atoms);
int admp_md_mts_step(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* grad_slow, const void* inv_mass,
                     const double* box, double half_dt_acc_outer, double dt_outer, int n_inner, double c1, double c2sq_kT_acc,
                     uint64_t seed, uint64_t outer_step, double* E_dev, void* grad_fast_out);
int admp_md_mts_info(admp_handle* h, int64_t* out8);
int admp_md_con_plan(admp_handle* h, int n_atoms, int n_constraints, const int32_t* pairs, const double* lengths, int tile_atoms);
int admp_md_con_step(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* grad, const void* inv_mass,
                     const double* box, double half_dt_acc, double dt, double c1, double c2sq_kT_acc, uint64_t seed, uint64_t step,
                     double tolerance, int max_sweeps, int32_t* counters_dev);
int admp_md_con_kick(admp_handle* h, int n_atoms, const void* positions, void* velocities, const void* grad, const void* inv_mass,
                     const double* box, double half_dt_acc, double dt, double tolerance, int max_sweeps, double* ekin_dev,
                     int32_t* counters_dev);
int admp_md_con_project(admp_handle* h, int n_atoms, void* positions, const void* reference, const void* inv_mass, const double* box,
                        double tolerance, int max_sweeps, int32_t* counters_dev);
int admp_md_con_info(admp_handle* h, int64_t* out8);
int admp_md_mol_plan(admp_handle* h, int n_atoms, const int32_t* group_of, int tile_atoms);
int admp_md_mol_sums(admp_handle* h, int n_atoms, const void* positions, const void* velocities, const void* grad, const void* inv_mass,
                     const double* box, uint64_t seed, uint64_t step, double* out21_dev);
int admp_md_mol_scale(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* inv_mass, const double* box,
                      double mu_minus_1, double inv_mu_minus_1);
int admp_md_mol_info(admp_handle* h, int64_t* out8);
int admp_md_fire_step(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* grad, const void* inv_mass,
                      const double* params9, double ftol, uint64_t call, double* state16_dev);
int admp_md_vrescale(admp_handle* h, int n_atoms, void* velocities, const void* grad /* may be NULL: thermostat only */,
                     const void* inv_mass, double half_dt_acc, int64_t n_dof, double kT_acc, double c, uint64_t seed, uint64_t step,
                     uint64_t call, double* state16_dev);

/* No counterpart in the reference: radial distribution functions -- the typed pair-distance counts of one frame, ADDED to a
 * caller-owned device histogram (admp_amd/csrc/rdf_math.h, rdf_plan.h, rdf_kernels.hip).  Needs no topology and no pair list:
 * the neighbour tables of the calculators stop at their cutoff, a g(r) runs to 8-12 A.
 *   positions_dev  (n_atoms,3) real of the handle's precision, DEVICE pointer; atoms may lie outside the cell
 *   box            9 HOST doubles, lattice vectors in rows
 *   tags_dev       (n_atoms) int32, DEVICE pointer: type | group << 4.  type 0 .. n_types - 1 is a counted type, 15 means "not
 *                  counted", and so does every other value (8 .. 14, and a type >= n_types); group is 0 .. 2^27 - 1.  A pair is
 *                  counted when both types are counted and the groups differ (groups = molecules excludes the intramolecular
 *                  pairs; "no exclusions" is every atom its own group).
 *   n_types        1 .. 8; the unordered type pair (a <= b) is channel a n_types - a (a - 1) / 2 + (b - a), of
 *                  n_types (n_types + 1) / 2 channels
 *   r_max, n_bins  bin k of a channel counts the pairs with k r_max / n_bins <= r < (k + 1) r_max / n_bins, r the length of the
 *                  minimum image of r_i - r_j in the handle's precision (the arithmetic of the pair kernels); pairs with
 *                  r >= r_max are not counted.  channels * n_bins <= 16384 (the histogram of a workgroup is 64 KB of LDS).
 *   hist_dev       (channels, n_bins) uint64, DEVICE pointer: the counts are ADDED; the caller zeroes it and reads it
 *   force          0: the library chooses (up to 4096 atoms the tile form: one workgroup per pair of 256-atom tiles; above, the
 *                  cell form: atoms binned at cell width >= r_max, one workgroup per home cell, half sweep); 1: tiles; 2: cells
 *   info4          HOST, may be NULL: form (0 nothing launched, 1 tiles, 2 cells), workgroups, tiles or cells, LDS bytes of a
 *                  workgroup
 * Counters are integers and only integer atomics add to them (32-bit in LDS, flushed before one could wrap, 64-bit in hist_dev):
 * the result does not depend on the order of anything and is the same bit for bit from run to run.  Runs on the handle's stream
 * and makes no host synchronisation (the first call of the cell form, and one that needs more scratch, allocate): an MD loop
 * records a frame every few steps and reads the histogram when the run ends.  n_atoms = 0 launches nothing.
 * ADMP_E_STATE on a slab-decomposed handle.  ADMP_E_ARG, before anything is launched, for a NULL box or hist_dev, NULL positions
 * or tags (unless n_atoms = 0: an empty device array has no address), n_atoms < 0, n_types outside 1 .. 8, n_bins < 1,
 * channels * n_bins > 16384, r_max not finite, <= 0 or above half of any perpendicular height of the cell, a singular or
 * non-finite box, force outside 0 .. 2. */
int admp_md_rdf(admp_handle* h, int n_atoms, const void* positions_dev, const double* box /* 9 host */, const int32_t* tags_dev,
                int n_types, double r_max, int n_bins, uint64_t* hist_dev /* channels * n_bins, ADDED to */,
                int force /* 0 auto, 1 tiles, 2 cells */, int64_t* info4 /* host, may be NULL */);

/* No counterpart in the reference: time correlation functions -- one recorded frame correlated with the last n_lags - 1 frames
 * of a caller-owned device ring (admp_amd/csrc/tcf_math.h, tcf_plan.h, tcf_kernels.hip).  For every counted type a and every lag
 * k = 0 .. min(frame, n_lags - 1) the call ADDS
 *     acc[0][a][k] += sum_{i of type a} |d_i(t) - d_i(t - k)|^2        (A^2;      mean-square displacement x N_a x origins)
 *     acc[1][a][k] += sum_{i of type a} v_i(t) . v_i(t - k)            (A^2/fs^2; velocity autocorrelation x N_a x origins)
 * where t is this frame and t - k the frame recorded k calls earlier; lag 0 is included (acc[0][a][0] stays 0, acc[1][a][0] sums
 * v^2).  The number of time origins behind lag k after `frames` calls is max(0, frames - k); the caller keeps it.
 *   positions_dev, velocities_dev  (n_atoms,3) real of the handle's precision, DEVICE pointers; atoms may lie outside the cell
 *   box            9 HOST doubles, lattice vectors in rows
 *   slot_atom_dev  (n_slots) int32, DEVICE pointer: the atom of a slot, or anything outside 0 .. n_atoms - 1 for padding.  The
 *                  counted atoms sorted by type, every type's run padded to a whole number of tiles of tile_atoms slots, so
 *                  that a tile holds one type (admp_amd/md.py tcf_layout).  n_slots = n_tiles * tile_atoms.
 *   tile_type_dev  (n_tiles) int32, DEVICE pointer: the type 0 .. n_types - 1 of a tile; anything else: the tile is not counted
 *   tile_atoms     a multiple of 64 in 64 .. 1024;  n_types 1 .. 8;  n_lags >= 1
 *   frame          the index of this frame, 0, 1, 2, ...: 0 initialises the state (d = 0, last = positions) and counts no jump;
 *                  frame f is stored in ring slot f mod n_lags and reaches the lags 0 .. min(f, n_lags - 1)
 *   ring_dev       (n_lags, 2, 3, n_slots) real of the handle's precision, DEVICE pointer: d and v of the last n_lags frames, one
 *                  component per row.  d is rounded once from the double accumulator, v is copied unchanged.
 *   unwrapped_dev  (n_slots,3) double: d_i, the unwrapped displacement since frame 0.  Every call adds the minimum image of
 *                  positions - last, taken in THIS call's cell, in double whatever the handle's precision: the result is the
 *                  same whether or not the caller wraps atoms into the cell, on a triclinic cell too.  Under a changing cell
 *                  (NPT) the displacement between two frames is therefore the minimum image in the newer cell.
 *   last_dev       (n_slots,3) real of the handle's precision: the position of the slot's atom at the previous call
 *   jumps_dev      one uint64 word, integer atomicAdd: the number of (slot, call) whose minimum-image move had a fractional
 *                  component |s| >= 0.25 (whole lattice vectors, which a caller who wraps atoms adds, are removed first) -- a
 *                  quarter of a cell height or more between two frames cannot be unwrapped safely.  The move is applied all the
 *                  same and nothing is refused.
 *   acc_dev        (2, n_types, n_lags) double, DEVICE pointer: ADDED to; the caller zeroes it and reads it
 *   info4          HOST, may be NULL: workgroups of the lag kernel, lags per workgroup, lags correlated in this call, scratch bytes
 * The sums are in double (the conversion of a float is exact) without float atomics: a lane sums its slots, a wave its lanes, a
 * workgroup its waves and one lane per (quantity, type, lag) the tiles of its type, all in an order that is a function of the
 * layout alone, so a run repeats bit for bit.  A call reads every ring word of the lags it reaches once: lags * n_slots * 6
 * words.  Runs on the handle's stream and makes no host synchronisation (growing the driver's scratch, 2 n_tiles n_lags doubles,
 * excepted).  n_slots = 0 launches nothing.
 * ADMP_E_STATE on a slab-decomposed handle.  ADMP_E_ARG, before anything is launched or written, for a NULL box, acc, ring,
 * unwrapped, last or jumps pointer, NULL positions, velocities, slot_atom or tile_type (unless n_slots = 0), a negative count,
 * n_slots != n_tiles * tile_atoms, tile_atoms not a multiple of 64 in 64 .. 1024, n_types outside 1 .. 8, n_lags < 1, frame < 0, a
 * singular or non-finite box. */
int admp_md_tcf(admp_handle* h, int n_atoms, const void* positions_dev, const void* velocities_dev, const double* box /* 9 host */,
                int n_slots, const int32_t* slot_atom_dev, int n_tiles, const int32_t* tile_type_dev, int tile_atoms,
                int n_types, int n_lags, int64_t frame /* 0: first frame, initialises the state */,
                void* ring_dev, double* unwrapped_dev, void* last_dev, uint64_t* jumps_dev,
                double* acc_dev /* (2, n_types, n_lags), ADDED to */, int64_t* info4 /* host, may be NULL */);

/* ---- multi-GPU: x-slab decomposition ---------------------------------------------------------------------
 * (no counterpart in the reference, which is single-device)  One process per GPU, SPMD: every rank makes
 * the same admp_pme_energy_grad / admp_disp_energy_grad / admp_tt_energy_grad call with the same full input arrays.  Rank s
 * owns the mesh planes [X0,X1) along x and works on its "home" atoms (lowest stencil plane inside the slab); the library
 * runs the whole evaluation -- the same kernels and the same SCF forms as on one GPU -- and calls back into the caller's
 * communicator where ranks exchange data: ghost planes after the spread / before the gather (shift), the two transposes
 * of the distributed 3-D transform (all_to_all_v), the dipoles / gradient contributions of the halo atoms (all_to_all_v
 * over index lists both ends derive by themselves), the SCF residual (all_reduce MAX of one word) and the energies
 * (all_reduce SUM of four words).  The host side binds the callbacks to RCCL (torch.distributed backend "nccl" in
 * admp_amd/parallel.py); nothing proportional to the number of atoms is ever exchanged by the library itself.
 *
 * Callback contract: buffers are DEVICE pointers owned by the library; counts are in elements of `dtype`; a callback is
 * entered on the thread that made the library call, with the handle's stream being the caller's current stream, and must
 * enqueue its communication ordered after the work already on that stream and before whatever is enqueued on it later
 * (torch.distributed collectives on the current stream do exactly that).  Return 0, or non-zero to abort the call with
 * ADMP_E_COMM.  `tag` says what travels (accounting only). */
enum { ADMP_T_I32 = 0, ADMP_T_F32 = 1, ADMP_T_F64 = 2 };
enum { ADMP_OP_SUM = 0, ADMP_OP_MAX = 1 };
enum { ADMP_TAG_GHOST = 1, ADMP_TAG_TRANSPOSE = 2, ADMP_TAG_HALO_DIPOLES = 3, ADMP_TAG_HALO_GRADIENT = 4, ADMP_TAG_SCF_MAX = 5,
       ADMP_TAG_ENERGIES = 6 };
typedef struct admp_comm {
  void* ctx;
  /* in place over `count` elements of every rank */
  int (*all_reduce)(void* ctx, void* buf, int64_t count, int dtype, int op, int tag);
  /* segment t of `send` (send_counts[t] elements, segments back to back in rank order) goes to rank t; segment s of `recv`
   * (recv_counts[s] elements) comes from rank s */
  int (*all_to_all_v)(void* ctx, const void* send, const int64_t* send_counts, void* recv, const int64_t* recv_counts,
                      int dtype, int tag);
  /* ring shift: send `count` elements to rank+1 (to_next != 0) or rank-1, receive as many from the opposite neighbour */
  int (*shift)(void* ctx, const void* send, void* recv, int64_t count, int dtype, int to_next, int tag);
} admp_comm;
/* rank / nranks of this handle (nranks = 1: not decomposed; at most 28 ranks).  Call before the first evaluation. */
int admp_slab_configure(admp_handle* h, int rank, int nranks);
/* the communicator of a decomposed handle (copied; ctx must outlive the handle).  NULL detaches. */
int admp_set_comm(admp_handle* h, const admp_comm* comm);
/* out11 = {X0, X1, Y0, Y1, local planes (X1-X0+ghost), ghost, K1, K2, K3/2+1, rank, nranks} */
int admp_slab_info(admp_handle* h, int64_t* out11);
/* ---- native RCCL communicator (round 4) ---------------------------------------------------------------------
 * The collectives of a decomposed handle issued by the library itself, on the handle's stream: ncclAllReduce, and
 * ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd for the all-to-all-v and the ring shifts -- no callback, no host
 * language in the step.  RCCL is bound at run time (dlopen of librccl.so.1; inside a PyTorch process that is the copy
 * PyTorch already holds), so single-GPU users never load it.
 *   admp_rccl_unique_id   rank 0 creates the 128-byte id (ncclGetUniqueId); the caller distributes it to the other ranks by
 *                         whatever means it has (torch.distributed broadcast in admp_amd/parallel.py, MPI, a file ...)
 *   admp_rccl_create      every rank: ncclCommInitRank on `device` (blocks until all ranks have joined)
 *   admp_set_comm_rccl    binds the communicator to a handle: sets rank / nranks (as admp_slab_configure) and replaces the
 *                         callbacks of admp_set_comm.  One communicator serves any number of handles of the process (PME,
 *                         dispersion PME, pair potentials); it must outlive them.  NULL detaches.
 *   admp_rccl_stats       bytes sent to other ranks / calls per ADMP_TAG_* (arrays of ADMP_RCCL_NTAGS), optionally cleared
 *   admp_rccl_abort       ncclCommAbort: releases peers blocked in a collective of this communicator (error paths)
 *   admp_rccl_all_reduce  in-place SUM / MAX over `count` elements of a caller-owned DEVICE buffer on `hip_stream` (what a
 *                         driver that wants the reference's replicated outputs does once per output array; tag 7)
 *   admp_rccl_all_to_all_v, admp_rccl_shift   the other two collectives of the decomposed evaluation on caller-owned DEVICE
 *                         buffers, with the semantics of the admp_comm callbacks above (for drivers that move their own
 *                         per-atom data between slab ranks, and for tests) */
typedef struct admp_rccl admp_rccl;
enum { ADMP_RCCL_ID_BYTES = 128, ADMP_RCCL_NTAGS = 8 };
int admp_rccl_unique_id(void* out128);
int admp_rccl_create(admp_rccl** out, int device, const void* id128, int rank, int nranks);
int admp_rccl_destroy(admp_rccl* c);
int admp_rccl_abort(admp_rccl* c);
int admp_rccl_stats(admp_rccl* c, int64_t* bytes_out, int64_t* calls_out, int reset);
int admp_rccl_all_reduce(admp_rccl* c, void* buf, int64_t count, int dtype /* ADMP_T_* */, int op /* ADMP_OP_* */, void* hip_stream);
int admp_rccl_all_to_all_v(admp_rccl* c, const void* send, const int64_t* send_counts, void* recv, const int64_t* recv_counts,
                           int dtype, void* hip_stream);
int admp_rccl_shift(admp_rccl* c, const void* send, void* recv, int64_t count, int dtype, int to_next, void* hip_stream);
int admp_rccl_version(int* version);
const char* admp_rccl_last_error(void);
int admp_set_comm_rccl(admp_handle* h, admp_rccl* c);
/* Outputs of a decomposed evaluation: dE_dpos / U_inout / dE_dQlocal hold this rank's HOME rows (the other rows are
 * unspecified); E_out, n_cycle and converged are the global values on every rank.  home_out (device, room for n_atoms
 * int32) receives the home atoms of the last evaluation in ascending order, *n_home their number; n_import (optional) the
 * number of atoms the rank read without owning them. */
int admp_slab_home(admp_handle* h, int32_t* home_out, int* n_home, int* n_import);
/* The lists of the last decomposed evaluation of a handle, copied to HOST arrays as they stand on the device (test entry: no
 * kernel runs; ADMP_E_ARG on a single-rank handle, on a handle without a decomposed evaluation, and when n_atoms / nranks are
 * not the handle's).  owner, bits: n_atoms words (owner of every atom; kSlabHome / kSlabPolar / reader bits of slab_kernels.hip).
 * home (ascending), rows (the home rows in the pair kernels' order), act (polarizable home atoms), imp (atoms read from every
 * other rank, rank after rank), mig_in, mig_out (atoms that changed hands since the handle's previous evaluation): room for
 * n_atoms words each.  exp (atoms sent to every other rank, rank after rank; an atom may go to several): room for n_atoms *
 * nranks words.  counts (8 + 4 nranks words): {n_home, n_act, n_import, n_export, 1 if the evaluation tracked migrants,
 * n_mig_in, n_mig_out, 0}, then per rank the lengths of its segment of imp, exp, mig_in, mig_out. */
int admp_slab_lists(admp_handle* h, int n_atoms, int nranks, int32_t* owner, int32_t* bits, int32_t* home, int32_t* rows,
                    int32_t* act, int32_t* imp, int32_t* exp, int32_t* mig_in, int32_t* mig_out, int64_t* counts);

/* How the polarizable evaluations of this handle were enqueued (the residual history of the previous calls decides between
 * the plain loop, a speculative first cycle and a chain of device-gated Jacobi steps: engine.hip pme()) and what the guesses
 * cost.  out8 = {plain calls, speculative calls, speculative calls whose first check failed, chained calls, chained calls
 * that needed more steps than enqueued, chained calls that enqueued more than needed, field increments that ran for nothing
 * in those, Jacobi steps in total}; reset != 0 clears the counters.  The results never depend on the form. */
int admp_scf_stats(admp_handle* h, int64_t* out8, int reset);

/* Always-stable predictor-corrector dipoles (J. Kolafa, J. Comput. Chem. 25, 335, 2004) for molecular dynamics: while the
 * mode is on, EVERY polarizable admp_pme_energy_grad of this handle counts as one time step.  With order k the handle keeps
 * the dipoles U(n-1) .. U(n-k-2) that its last k + 2 such calls used for their forces (a ring of device arrays of the
 * handle's precision) and a call runs the fixed form:
 *     U_p = sum_{j=1..k+2} B_j U(n-j),   B_j = (-1)^(j+1) j C(2k+4, k+2-j) / C(2k+2, k+1)
 *     n_corrector times:  U <- U - omega pol (dE/dU at U) / DIELECTRIC          (first from U = U_p)
 *     energies, gradient and dE/dQ_local at U; U joins the history and is returned in U_inout
 * That is 1 + n_corrector field evaluations (the later ones incremental), no residual read and one host synchronisation.
 * The call ignores U_inout's initial values, admp_set_dipole_source, thresh and max_cycle (max_cycle >= 1 is still asked
 * for) and reports n_cycle = n_corrector, converged = 1.
 *   order        -1 turns the mode off (the default) and drops the history; 0..4 turns it on
 *   n_corrector  1 .. 6
 *   omega        <= 0: Kolafa's (k + 2) / (2k + 3); otherwise 0 < omega <= 1.  n_corrector > 1 with omega = 1 is n plain
 *                Jacobi steps from U_p.
 * Anything else (a NaN included) is ADMP_E_ARG; a non-polarizable or slab-decomposed handle ADMP_E_STATE.  Every accepted
 * call drops the history and clears the counters; configuring the handle as a slab afterwards turns the mode off.
 * While fewer than k + 2 sets are stored a call runs exactly as without the mode and its final dipoles are stored (warm-up).
 * A call whose polarizable rows the host does not know yet starts from U_p and runs the ordinary SCF to the caller's
 * threshold (fallback); its result is stored as well.  admp_set_topology and admp_set_ewald drop the history; a failed call
 * leaves it unadvanced or drops it.  Only admp_pme_energy_grad advances it: the fixed-dipole, box-gradient, parameter-gradient
 * and diagnostic entries do not touch it.
 * admp_scf_aspc_reset keeps the mode and drops the history: for a driver whose positions have just jumped.
 * admp_scf_aspc_info: out8 = {order, n_corrector, stored sets, fixed-form calls, warm-up calls, fallback calls, 0, 0},
 * out2 = {omega in effect, max|dE/dU| at the predicted dipoles of the last fixed-form call (it comes back with the energies)}. */
int admp_scf_aspc(admp_handle* h, int order, int n_corrector, double omega);
int admp_scf_aspc_reset(admp_handle* h);
int admp_scf_aspc_info(admp_handle* h, int64_t* out8, double* out2);
/* Which form the x passes of the direct-DFT mesh convolution took: out2 = {one real circulant product per line (G table
 * even along x: orthorhombic cells; ADMP_DFT_XCIRC=0 turns it off), forward transform * G * inverse transform}. */
int admp_xpass_stats(admp_handle* h, int64_t* out2, int reset);
/* Launches of the plane kernels of the direct-DFT mesh convolution: out2 = {FORWARD launches with a matrix-core share of their
 * line products (double precision, lines of 33 points and more; ADMP_DFT_PLANE_MFMA=0 turns it off), every other plane launch:
 * forward ones in the vector form and inverse ones of EITHER form}. */
int admp_plane_mfma_stats(admp_handle* h, int64_t* out2, int reset);
/* The same launches by direction: out4 = {forward with a share, forward in the vector form, inverse with a share (double
 * precision, a y or z line of 33 points and more; ADMP_DFT_PLANE_MFMA_INV=0 turns that one off alone), inverse in the vector
 * form}.  The two sets of counters are reset separately. */
int admp_plane_mfma_stats4(admp_handle* h, int64_t* out4, int reset);
/* The k-space leg of a reciprocal pass alone, on a mesh of the caller's (admp/recip.py:400-426):
 *     mesh <- IFFT( G * FFT(mesh) ) (unnormalised: N times numpy's ifftn),   *E_out = 1/2 sum_k G(k) |FFT(mesh)(k)|^2
 * with G the handle's own table for `box`: which = 1: 2 DIELECTRIC Ck_1 / theta_k^2, gamma point zero; which = 6, 8, 10:
 * 2 Ck_n / theta_k^2 with the gamma point.  It runs what an evaluation runs between its spread and its gather -- the same
 * transform path (rocFFT, fused x, direct-DFT lines or planes, two-level), the same G table, the same kernels -- in place on
 * K1 K2 K3 words of the handle's type, on the device (on_device != 0) or on the host.  Needs admp_set_ewald only (no
 * topology, no pairs; meshes down to 2 points per dimension); single rank: a slab-decomposed handle returns ADMP_E_ARG.
 * info16 says which form ran:
 *   [0] path (ADMP_MESH_PATH_*)       [1] direct paths: x pass as 1 = one circulant product, 2 = two transforms (else 0)
 *   two-level path, per axis d = x, y, z:  [2+d] N1   [5+d] N2   [12+d] MFMA stage A (z: bit 0 forward, bit 1 inverse pass)
 *   [8] [9] columns per workgroup (NC) of the x and y passes   [10] [11] lines per workgroup (NL) of the forward / inverse z pass
 *   [15] 0 */
#define ADMP_MESH_INFO_WORDS 16
#define ADMP_MESH_PATH_ROCFFT 0        /* rocFFT 3-D r2c, G kernel, c2r */
#define ADMP_MESH_PATH_FUSED_X 1       /* rocFFT y-z planes around the fused x pass (fftx_kernels.hip) */
#define ADMP_MESH_PATH_DIRECT_LINES 2  /* direct DFT, z, y and x lines as separate passes (dft_kernels.hip) */
#define ADMP_MESH_PATH_DIRECT_PLANES 3 /* direct DFT, plane kernels for z and y */
#define ADMP_MESH_PATH_TWO_LEVEL 4     /* Good-Thomas split (pfa_kernels.hip) */
int admp_mesh_convolve(admp_handle* h, const double* box, int which, void* mesh_inout, int on_device, double* E_out,
                       int32_t* info16);
/* The same leg on the ranks of a slab-decomposed handle (test entry; a single-rank handle returns ADMP_E_ARG).  Needs
 * admp_set_ewald, admp_slab_configure or admp_set_comm_rccl, and a communicator (no topology, no pairs); every rank makes the
 * call, as with an evaluation.  mesh_inout is the rank's LOCAL mesh exactly as an evaluation holds it between spread and
 * gather: (X1-X0) + 5 planes of K2 K3 words of the handle's type, on the device or on the host -- the rank's own planes, then
 * the 5 overhang planes meant for the next rank.  The call runs the distributed convolution of an evaluation and nothing else
 * (ghost planes sent on and added, y-z transforms, transpose, the x pass the handle would choose with the rank's rows of the G
 * table, and back).  It returns phi on the own planes and, in the 5 ghost planes, what the closing shift delivered: the next
 * rank's first 5 planes of phi.  *E_out is this rank's share of 1/2 sum_k G |S|^2 (its rows Y0 <= ky < Y1 of the transposed
 * spectrum); the sum over the ranks is the energy.
 * info16: [0] the x pass: ADMP_MESH_PATH_FUSED_X = the fused x kernel on the transposed layout, ADMP_MESH_PATH_ROCFFT = rocFFT
 * 1-D lines around the G kernel; [2] X0 [3] X1 [4] Y0 [5] Y1; [6] row pitch of the y-z spectrum (complex numbers); [7] K3/2+1;
 * every other word 0. */
int admp_slab_mesh_convolve(admp_handle* h, const double* box, int which, void* mesh_inout, int on_device, double* E_out,
                            int32_t* info16);
/* One real-space pair kernel alone, and its raw per-atom rows (test entry; single rank: a slab-decomposed handle returns
 * ADMP_E_ARG).  The call does what an evaluation does up to that kernel -- sites prepared at the dipoles U as given (no SCF),
 * site classes compiled into the neighbour table, the inner table of admp_set_cutoff -- and launches it through the
 * evaluation's own launcher; nothing of the mesh chain runs.
 *   which = 0: the closing kernel k_pair_full.  flags bit 0 set: the charge-only pair forms are allowed, as in a call
 *              without dE_dQlocal; clear: general arithmetic on every row.
 *   which = 1: the SCF field kernel k_pair_field over the polarizable rows (polarizable handle; `flags` unused).
 *   which = 2: the incremental field kernel k_pair_field_ind.  `F` (Na,3, like U) is the total field of the Jacobi step the
 *              kernel follows: the step forms dU = -pol F / DIELECTRIC on the polarizable sites exactly as in the SCF (in a
 *              copy of U), the kernel walks the SCF's own polarizable-polarizable sub-table and sorted site list, and fld
 *              returns the increment alone, sum_j T_ij dU_j.  `F` is ignored (may be NULL) for which = 0 and 1.
 * Outputs, words of the handle's type on the device (on_device != 0) or on the host, like the inputs:
 *   *E_out (host)  the real-space energy (which = 0; else 0)
 *   grad (Na,3)    dE/dr of the pair terms at fixed global multipoles          (which = 0)
 *   pot  (Na,9)    dE/dQ_global; on a charge-only row walked in the reduced forms only slot 0 is formed   (which = 0)
 *   fld  (Na,3)    dE/dU in harmonic order (z, x, y); polarizable handles; which >= 1: zero on rows that are not polarizable
 * info4 = {lanes per row of the launch, 1 if the rows ended at the cutoff's inner table, 1 if the charge-only forms were in
 * effect (allowed, compiled in and the table's classes not stale; 0 for which = 2, which has none), minimum-waves instance
 * of k_pair_full (0 for which >= 1)}.
 * The class bookkeeping is an evaluation's: a first call compiles the classes, a call after the sites changed class sees a
 * stale table (general forms) and the call after that a recompiled one. */
int admp_pair_real(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                   const void* tholes, int n_scales, const double* mScales, const double* pScales, const void* U,
                   const void* F, int which, int flags, int on_device, double* E_out, void* grad, void* pot, void* fld,
                   int32_t* info4);
/* The B-spline spread of the multipoles alone, and the mesh it leaves (test entry; single rank: a slab-decomposed handle
 * returns ADMP_E_ARG).  Needs topology, Ewald parameters and pairs (an empty pair list will do).  The call prepares the
 * sites at the dipoles U as given (no SCF), as an evaluation does, and spreads through the evaluation's own launchers.
 *   which = 0: launch_spread, the spread that opens an evaluation; mesh_out receives the K1 K2 K3 words of the mesh.
 *              flags bit 0 set: the fixed-point scale of the f32 brick kernel comes from the stencil-window bound (an
 *              evaluation's form); clear: from the entry count (the form of the SCF increments).
 *              flags bit 1 set: no stencil records are handed over, the kernels recompute them (the increments' form).
 *   which = 1: the forward plane kernel of the direct-DFT convolution builds its planes from the sites (no spread kernel, no
 *              mesh) and the convolution runs on; mesh_out receives phi = IFFT(G FFT(mesh)), unnormalised, for the handle's
 *              own G table.  Only where an evaluation would do the same (double precision, at most 8192 atoms, a mesh on
 *              the plane kernels): ADMP_E_ARG otherwise, never another path.  flags bit 1 as above.
 * Words of the handle's type on the device (on_device != 0) or on the host, inputs and mesh_out alike.
 * info8 = {form that ran (ADMP_SPREAD_FORM_*), bricks along x, y, z, 1 if the stencil-window scale was in effect (brick form,
 * single precision, flags bit 0), which = 1: the ADMP_MESH_PATH_* of the convolution (else -1), 1 if stencil records were
 * handed to the kernels, 0}. */
#define ADMP_SPREAD_FORM_SCAN 0          /* k_spread_scan: every brick's workgroup scans all atoms */
#define ADMP_SPREAD_FORM_PLANES 1        /* k_spread_planes: global float atomics, 8 lanes per atom */
#define ADMP_SPREAD_FORM_BRICKS 2        /* k_bin + k_spread_bricks: binned, fixed-point LDS tiles */
#define ADMP_SPREAD_FORM_PLANE_KERNEL 3  /* zy_plane_spread inside the forward plane kernel of the direct DFT */
int admp_mesh_spread(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                     const void* tholes, const void* U, int which, int flags, int on_device, void* mesh_out, int32_t* info8);
/* The gather alone, on a phi of the caller's (K1 K2 K3 words; test entry, single rank, prerequisites and site preparation as
 * admp_mesh_spread).  The output rows are zeroed by the call.
 *   which = 0: k_gather_staged with the atom-side energy: pot (Na,9) = the reciprocal dE/dQ_global, grad (Na,3) = dE/dr at
 *              fixed global multipoles, fld (Na,3) = the Cartesian reciprocal dE/dU (slots 11c, 11s, 10 of pot) on polarizable
 *              handles (else ignored), *E_out = 1/2 sum_i Q_i . pot_i summed from the partial words.
 *   which = 1: k_gather_field_staged over the handle's own list of polarizable sites (polarizable handle): fld (Na,3) = the
 *              Cartesian reciprocal dE/dU of the listed atoms, zero on every other row; pot, grad unused, *E_out = 0.
 * info4 = {kernel (0: k_gather_staged, 1: k_gather_field_staged), rows gathered, workgroups that have rows, workgroups
 * launched}.  Not reached from here: the closing epilogue of the gather, compact rows added to a field, batches. */
int admp_mesh_gather(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                     const void* tholes, const void* U, const void* phi_in, int which, int on_device, double* E_out, void* pot,
                     void* grad, void* fld, int32_t* info4);
/* One leg of the reciprocal part of a dispersion PME call alone (test entries; single rank: a slab-decomposed handle returns
 * ADMP_E_ARG).  Needs topology, Ewald parameters and pairs (an empty pair list will do).  Both choose the path exactly as
 * admp_disp_energy_grad does (the handle's mesh plans, the brick rule of the spread, the precision, pmax, the type table of
 * admp_disp_set_types) and run that path's own part functions; nothing of the real-space chain runs.  c_list (Na,3).
 * A path keeps nmesh meshes of K1 K2 K3 words: one per power (C6, C8, C10 up to pmax), or one per type on the typed paths.
 *   admp_disp_mesh_spread: what the path launches between the pair kernel and the convolution (brick paths: stencil bases,
 *     binning, brick spread; site-row paths: scalar site rows, spread; typed paths: the type check and the one-hot weights as
 *     well).  mesh_out receives the nmesh meshes, the powers of a per-power loop in consecutive meshes.  *E_self_out: what the
 *     leg added to the self word (the site-row paths sum the self term with their rows; the brick paths add nothing here).
 *   admp_disp_mesh_gather, which = 0: phi_in holds nmesh meshes as the path's convolution leaves them (phi_p per power, or
 *     psi_t = sum_p c_p,t phi_p per type on the typed paths); out (Na,3) = the path's gather into a gradient that starts from
 *     zero; *E_self_out: the self term where the path forms it after the convolution (the brick paths' sum on the device, the
 *     typed paths' sum over the type counts), else 0.
 *   which = 1: the value gather of admp_disp_param_grad's mesh part: out (Na,3)[:, p] = phi_p(r_i) + 2 kp_p c_p,i, phi_in one
 *     mesh per power; *E_self_out = 0.
 * On a typed path a type table that does not describe c_list is refused as by admp_disp_energy_grad.
 * Words of the handle's type on the device (on_device != 0) or on the host, inputs and outputs alike.
 * info8 = {path (index of DispPath in csrc/disp_plan.h: 0 BricksTyped, 1 BricksBatched, 2 BricksPerPower, 3 DftTyped,
 * 4 DftBatched, 5 PerPower), nmesh, 1 if the meshes are per type, bricks along x, y, z, workgroups the launcher of the leg's main
 * kernel used, as that launcher reports them, for the kernels of disp_kernels.hip (brick spread, k_gather_scalar,
 * k_gather_value); -1 on the site-row paths, whose legs run the electrostatics launchers, the site-row paths' spread form
 * (ADMP_SPREAD_FORM_*; -1 on the brick paths)}. */
int admp_disp_mesh_spread(admp_handle* h, const void* positions, const double* box, const void* c_list, int pmax, int on_device,
                          void* mesh_out, double* E_self_out, int32_t* info8);
int admp_disp_mesh_gather(admp_handle* h, const void* positions, const double* box, const void* c_list, int pmax,
                          const void* phi_in, int which, int on_device, double* E_self_out, void* out, int32_t* info8);
/* The site table alone (test entry, single rank, prerequisites as admp_mesh_spread): what an evaluation does up to the end of
 * its site pass (k_prepare_sites), at the dipoles U as given.
 *   sites_out (Na,20)  the site rows as the handle's type lays them out: r (3), Q global (9), U in harmonic order z, x, y (3),
 *                      pol^(1/6), thole, 3 pad words (pad[0] = 1 marks a charge-only site)
 *   act_out (Na int32) the list of polarizable sites (pol > 0) as the device wrote it, before the host sorts it: the first
 *                      info4[0] words; polarizable handles (else untouched, may be NULL)
 * Words of the handle's type (act_out: int32) on the device (on_device != 0) or on the host, like the inputs.
 * info4 = {number of polarizable sites (0 on a handle that is not polarizable), the class flags word of the call (bit 0: the
 * neighbour table's charge-only classes are stale, bit 1: they could be better), 1 if stencil records were written, the number
 * of energy words of this call's half of the energy block, other than the count, that did not read zero (the site pass of
 * the call before clears them: always 0)}. */
int admp_site_table(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                    const void* tholes, const void* U, int on_device, void* sites_out, int32_t* act_out, int32_t* info4);
/* The closing kernels alone (test entry, single rank, prerequisites and site preparation as admp_mesh_spread), on a
 * dE/dQ_global of the caller's, through the evaluation's own launchers.
 *   which = 0: launch_finish on pot_in (Na,9): the self term is added to the potential, and the call returns E_out = {self
 *              energy, polarization penalty}, grad_out (Na,3) = the local-frame adjoint alone (what the closing kernel adds to
 *              a zeroed gradient) and, if want_dQ, dQ_out (Na,9) = dE/dQ_local.
 *              info4 = {ADMP_FINISH_FORM_* of the launch, frame groups, runs of the row form, workgroups of the row form}.
 *   which = 1: the same work in the closing epilogue of the gather on phi_in (K1 K2 K3 words, required): pot_in is the pair part,
 *              the gather adds the reciprocal part to it and to the gradient.  ADMP_E_ARG where an evaluation would not take
 *              this form (no frame groups, more atoms than ADMP_FUSE_FIN_MAX).
 *              info4 = {ADMP_FINISH_FORM_GATHER_EPILOGUE, runs of the gather, 0, 0}.
 *   which = 2: k_frame_virial on pot_in: vir_out (9 doubles, host) = sum over the frames' used axis vectors of (minimum-image
 *              shift) (x) dE/d(vector); E_out, grad_out, dQ_out unused.  info4 = {-1, 0, 0, 0}.
 * Words of the handle's type on the device (on_device != 0) or on the host, inputs and outputs alike; E_out, vir_out: host. */
#define ADMP_FINISH_FORM_PULL4 0            /* k_finish_pull<4>: four lanes per atom over its inverse frame map */
#define ADMP_FINISH_FORM_PULL1 1            /* k_finish_pull<1> */
#define ADMP_FINISH_FORM_GROUPS 2           /* k_finish_groups: one lane per frame group */
#define ADMP_FINISH_FORM_ROWS 3             /* k_finish_rows: one lane per atom, runs of whole frame groups through LDS */
#define ADMP_FINISH_FORM_GATHER_EPILOGUE 4  /* k_gather_staged<.., FIN> */
#define ADMP_FINISH_FORM_LIST 5             /* k_finish over a list of atoms (slab ranks without frame groups) */
int admp_site_close(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                    const void* tholes, const void* U, const void* pot_in, const void* phi_in, int which, int want_dQ,
                    int on_device, double* E_out2, void* grad_out, void* dQ_out, double* vir_out9, int32_t* info4);
/* Where the closing pair kernel of the polarizable calls ran: out2 = {inside the x pass of a mesh convolution (small
 * double-precision systems on the direct-DFT mesh, one stream; ADMP_PAIR_RIDER=0 turns it off), in a launch of its own}. */
int admp_pair_rider_stats(admp_handle* h, int64_t* out2, int reset);

/* ---- measurement ---------------------------------------------------------------------------- */
/* When enabled every kernel launch is bracketed by HIP events on the handle's stream. */
int admp_profile_enable(admp_handle* h, int on);
/* restrict the bracketing to one kernel label (e.g. "pair_full"); NULL or "" = every kernel */
int admp_profile_filter(admp_handle* h, const char* label);
int admp_profile_reset(admp_handle* h);
/* number of distinct kernel labels seen; label / accumulated ms / launch count of entry idx */
int admp_profile_count(admp_handle* h);
int admp_profile_entry(admp_handle* h, int idx, const char** label, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* ADMP_HIP_H */
