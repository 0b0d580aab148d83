// The MD-driver helpers behind the admp_md_* entries of include/admp_hip.h (md_kernels.hip, mts_kernels.hip, con_kernels.hip,
// mol_kernels.hip, fire_kernels.hip, vrescale_kernels.hip, rdf_kernels.hip, tcf_kernels.hip): device pointers in, nothing read back.  Of a handle they use its device, its stream, its
// profiler and its rank count (handle.h HandleCtx), nothing of the engine.  The driver of a handle is created by its first
// admp_md_* call, in the handle's precision, and dies with the handle.
//
// Behaviour that looks like an accident and is kept as it was found, for the next change to decide about deliberately:
//   * admp_md_bonded and admp_md_kick_drift have no single-rank refusal and accept a slab-decomposed handle.
//   * Every other entry refuses a slab-decomposed handle with ADMP_E_STATE and "the MD helpers serve single-rank handles only",
//     before it looks at any other argument ...
//   * ... but admp_md_fire_step refuses it with ADMP_E_ARG and "... single-rank handles only (slab-decomposed handle)".
//   * admp_md_vrescale refuses it like the older entries: ADMP_E_STATE, their text, before any other argument.
//   * A missing plan gives ADMP_E_ARG with "<plan entry> must precede <this entry>".
//   * admp_md_virial and admp_md_mol_sums clear the 21 doubles of their output before the launch.
//   * admp_md_fire_step maps a non-zero return of launch_md_fire to ADMP_E_HIP with the prefix "FIRE step: ".
//   * admp_md_mts_step checks n_inner before it looks for null pointers; the launches of the other two plans look for null
//     inv_mass / box first (MdDriver::planned).
//   * The profiler labels: md_bonded, md_kick_drift, md_langevin, md_random, md_bonded_box, md_virial, md_scale, md_mts,
//     md_con_step, md_con_kick, md_con_project, md_mol_sums, md_mol_scale, md_fire, md_vrescale, md_rdf, md_tcf.
//   * The three *_info layouts differ (see the three functions); in each, words 0-6 are zero while no plan is held and word 7,
//     the launch count, is always reported.
//   * Tests match on the error texts: they stay byte for byte.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/admp_hip.h"
#include "dev_buf.h"
#include "handle.h"
#include "launch.h"
#include "md_fire_math.h"
#include "rdf_plan.h"
#include "tcf_plan.h"

using namespace admp;

namespace {

// A plan made on the host (mts_plan.h, con_plan.h, mol_plan.h) and kept on the handle until the next one replaces it: one block
// of ints, one of reals (rounded to the handle's precision once), and the record of pointers into them that the kernels take.
template <class Tiles>
struct PlanSlot {
  bool have = false;
  int n_atoms = 0, tile_atoms = 0, threads = 0;
  size_t lds_bytes = 0;
  int64_t launches = 0;
  Tiles tiles{};
  DevBuf ints, reals;
  // The int vectors one after the other into `ints`; returns where each starts.  The slot holds no plan from here until the
  // caller has pointed `tiles` at the new arrays and set `have`.
  std::vector<size_t> upload(hipStream_t stream, std::initializer_list<const std::vector<int>*> iv) {
    std::vector<int> hi;
    std::vector<size_t> off;
    for (const std::vector<int>* v : iv) { off.push_back(hi.size()); hi.insert(hi.end(), v->begin(), v->end()); }
    HIP_TRY(hipStreamSynchronize(stream));      // a launch of the plan being replaced may still read the old arrays
    have = false;
    ints.need(hi.size() * sizeof(int));
    HIP_TRY(hipMemcpy(ints.p, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice));
    return off;
  }
  // ... and the reals into `reals` (one element to spare, so that an empty list still has an address)
  template <class T>
  std::vector<size_t> upload(hipStream_t stream, std::initializer_list<const std::vector<int>*> iv, const std::vector<T>& hr) {
    const std::vector<size_t> off = upload(stream, iv);
    reals.need((hr.size() + 1) * sizeof(T));
    if (!hr.empty()) HIP_TRY(hipMemcpy(reals.p, hr.data(), hr.size() * sizeof(T), hipMemcpyHostToDevice));
    return off;
  }
  // the eight words of an *_info entry: all but the launch count are zero while no plan is held
  void info(int64_t* out, std::initializer_list<int64_t> v) const {
    ARG_CHECK(out, "bad argument");
    int k = 0;
    for (int64_t w : v) { out[k] = have || k == 7 ? w : 0; ++k; }
  }
};

template <class T>
struct MdDriver : HandleExt {
  HandleCtx& ctx;
  hipStream_t& stream;             // the handle's stream of the moment (admp_set_stream may change it between calls), and
  Profiler& prof;                  // its profiler: what TIMED names
  explicit MdDriver(HandleCtx& c) : ctx(c), stream(c.stream), prof(c.prof) {}

  void single_rank() {
    HIP_TRY(hipSetDevice(ctx.device));
    if (ctx.snranks > 1) throw Err{ADMP_E_STATE, "the MD helpers serve single-rank handles only"};
  }
  Box<T> finite_box(const double* box) {
    for (int k = 0; k < 9; ++k) ARG_CHECK(std::isfinite(box[k]), "box must be finite");
    double inv[9], vol;
    return make_box<T>(box, inv, &vol);
  }
  // what the launches of a plan share: every argument is checked before anything is launched (finite_box closes the checks)
  template <class Slot>
  void planned(const Slot& s, const char* plan_entry, const char* what, int n, const void* inv_mass, const double* box) {
    single_rank();
    if (!s.have) throw Err{ADMP_E_ARG, std::string(plan_entry) + " must precede " + what};
    ARG_CHECK(n >= 0 && n == s.n_atoms, "n_atoms differs from the plan's");
    ARG_CHECK(inv_mass && box, "bad argument");
  }

  void bonded(const void* pos, const double* box, int nb, const int32_t* bidx, const void* bpar, int na, const int32_t* aidx,
              const void* apar, double* E_dev, void* grad_) {
    ARG_CHECK(pos && box && E_dev && grad_ && nb >= 0 && na >= 0, "bad argument");
    ARG_CHECK((nb == 0 || (bidx && bpar)) && (na == 0 || (aidx && apar)), "bond / angle lists missing");
    double inv[9], vol;
    Box<T> bx = make_box<T>(box, inv, &vol);
    TIMED("md_bonded");
    launch_md_bonded<T>(stream, nb, bidx, reinterpret_cast<const T*>(bpar), na, aidx, reinterpret_cast<const T*>(apar),
                        reinterpret_cast<const T*>(pos), bx, reinterpret_cast<T*>(grad_), E_dev);
  }
  void kick_drift(int n, void* pos, void* vel, const void* grad_, const void* inv_mass, double half_dt_acc, double dt,
                  double* ekin_dev) {
    ARG_CHECK(n >= 0 && vel && grad_ && inv_mass && (dt == 0.0 || pos), "bad argument");
    TIMED("md_kick_drift");
    launch_md_kick_drift<T>(stream, n, reinterpret_cast<T*>(pos), reinterpret_cast<T*>(vel), reinterpret_cast<const T*>(grad_),
                            reinterpret_cast<const T*>(inv_mass), half_dt_acc, dt, ekin_dev);
  }
  void langevin(int n, void* pos, void* vel, const void* grad_, const void* inv_mass, double half_dt_acc, double dt, double c1,
                double c2sq_kT_acc, uint64_t seed, uint64_t step, double* ekin_dev) {
    single_rank();
    ARG_CHECK(n >= 0 && n <= INT_MAX / 4 && pos && vel && grad_ && inv_mass, "bad argument");
    ARG_CHECK(c1 >= 0.0 && c1 <= 1.0 && c2sq_kT_acc >= 0.0, "c1 must lie in [0, 1] and c2sq_kT_acc must not be negative");
    TIMED("md_langevin");
    launch_md_langevin<T>(stream, n, reinterpret_cast<T*>(pos), reinterpret_cast<T*>(vel), reinterpret_cast<const T*>(grad_),
                          reinterpret_cast<const T*>(inv_mass), half_dt_acc, dt, c1, c2sq_kT_acc, seed, step, ekin_dev);
    HIP_TRY(hipGetLastError());
  }
  void random(int kind, int64_t n, uint64_t seed, uint64_t step, uint32_t stream_id, void* out) {
    single_rank();
    ARG_CHECK(kind == 0 || kind == 1, "kind must be 0 (words) or 1 (normals)");
    ARG_CHECK(n >= 0 && n <= (int64_t)1 << 32 && (n == 0 || out), "bad argument (the atom index is a 32-bit counter word)");
    TIMED("md_random");
    launch_md_random<T>(stream, kind, n, seed, step, stream_id, out);
    HIP_TRY(hipGetLastError());
  }
  // the isotropic barostat's three (admp_amd/md.py CRescaleBarostat): every argument is checked before the first launch
  void bonded_box(const void* pos, const double* box, int nb, const int32_t* bidx, const void* bpar, int na, const int32_t* aidx,
                  const void* apar, double* E_dev, double* S_dev) {
    single_rank();
    ARG_CHECK(box && E_dev && S_dev && nb >= 0 && na >= 0 && nb <= INT_MAX / 4 - na, "bad argument");
    ARG_CHECK(nb + na == 0 || pos, "positions missing");
    ARG_CHECK((nb == 0 || (bidx && bpar)) && (na == 0 || (aidx && apar)), "bond / angle lists missing");
    Box<T> bx = finite_box(box);
    TIMED("md_bonded_box");
    launch_md_bonded_box<T>(stream, nb, bidx, reinterpret_cast<const T*>(bpar), na, aidx, reinterpret_cast<const T*>(apar),
                            reinterpret_cast<const T*>(pos), bx, E_dev, S_dev);
    HIP_TRY(hipGetLastError());
  }
  void virial(int n, const void* pos, const void* vel, const void* grad_, const void* inv_mass, uint64_t seed, uint64_t step,
              double* out_dev) {
    single_rank();
    ARG_CHECK(n >= 0 && n <= INT_MAX / 4 && out_dev && (n == 0 || (pos && vel && grad_ && inv_mass)), "bad argument");
    TIMED("md_virial");
    HIP_TRY(hipMemsetAsync(out_dev, 0, 21 * sizeof(double), stream));
    launch_md_virial<T>(stream, n, reinterpret_cast<const T*>(pos), reinterpret_cast<const T*>(vel),
                        reinterpret_cast<const T*>(grad_), reinterpret_cast<const T*>(inv_mass), seed, step, out_dev);
    HIP_TRY(hipGetLastError());
  }
  void scale(int n, void* pos, void* vel, double mu) {
    single_rank();
    ARG_CHECK(n >= 0 && n <= INT_MAX / 4 && (n == 0 || (pos && vel)), "bad argument");
    ARG_CHECK(std::isfinite(mu) && mu > 0.0 && std::isfinite(1.0 / mu), "the scale factor must be finite and positive");
    TIMED("md_scale");
    launch_md_scale<T>(stream, n, reinterpret_cast<T*>(pos), reinterpret_cast<T*>(vel), mu, 1.0 / mu);
    HIP_TRY(hipGetLastError());
  }

  // the multiple-time-step integrator (mts_kernels.hip; admp_amd/md.py MTSLangevin)
  struct : PlanSlot<MtsTiles<T>> { int max_component = 0, n_bonds = 0, n_angles = 0; } mts;
  void mts_plan(int n_atoms, int nb, const int32_t* bidx, const double* bpar, int na, const int32_t* aidx, const double* apar,
                int tile_atoms) {
    single_rank();
    ARG_CHECK(n_atoms > 0 && n_atoms <= INT_MAX / 4 && nb >= 0 && na >= 0, "bad argument");
    ARG_CHECK((nb == 0 || (bidx && bpar)) && (na == 0 || (aidx && apar)), "bond / angle lists missing");
    const MtsPlan p = mts_make_plan(n_atoms, nb, bidx, bpar, na, aidx, apar, tile_atoms == 0 ? kMtsDefaultTileAtoms : tile_atoms);
    if (!p.error.empty()) throw Err{ADMP_E_ARG, p.error};
    std::vector<T> hr(p.bond_par.begin(), p.bond_par.end());
    hr.insert(hr.end(), p.angle_par.begin(), p.angle_par.end());
    const std::vector<size_t> off = mts.upload(stream, {&p.tile_atom0, &p.atom_id, &p.tile_bond0, &p.bond_slot, &p.tile_angle0,
                                                            &p.angle_slot, &p.ref0, &p.ref}, hr);
    const int* di = mts.ints.template as<int>();
    MtsTiles<T>& m = mts.tiles;
    m.n_tiles = p.n_tiles; m.dims = p.dims;
    m.tile_atom0 = di + off[0]; m.atom_id = di + off[1]; m.tile_bond0 = di + off[2]; m.bond_slot = di + off[3];
    m.tile_angle0 = di + off[4]; m.angle_slot = di + off[5]; m.ref0 = di + off[6]; m.ref = di + off[7];
    m.bond_par = mts.reals.template as<T>(); m.angle_par = m.bond_par + p.bond_par.size();
    mts.n_atoms = n_atoms; mts.tile_atoms = p.tile_atoms; mts.max_component = p.max_component; mts.n_bonds = nb; mts.n_angles = na;
    mts.threads = mts_threads(p.tile_atoms);
    mts.lds_bytes = mts_lds_bytes(p.dims, sizeof(T));
    mts.have = true;
  }
  void mts_step(int n, void* pos, void* vel, const void* grad_slow, const void* inv_mass, const double* box,
                double half_dt_acc_outer, double dt_outer, int n_inner, double c1, double c2sq_kT_acc, uint64_t seed,
                uint64_t outer_step, double* E_dev, void* grad_fast) {
    single_rank();
    ARG_CHECK(mts.have, "admp_md_mts_plan must precede admp_md_mts_step");
    ARG_CHECK(n == mts.n_atoms, "n_atoms differs from the plan's");
    ARG_CHECK(n_inner >= 1, "n_inner must be at least 1");
    ARG_CHECK(pos && vel && grad_slow && inv_mass && box, "bad argument");
    ARG_CHECK(c1 >= 0.0 && c1 <= 1.0 && c2sq_kT_acc >= 0.0, "c1 must lie in [0, 1] and c2sq_kT_acc must not be negative");
    Box<T> bx = finite_box(box);
    TIMED("md_mts");
    launch_md_mts<T>(stream, mts.tiles, mts.threads, mts.lds_bytes, reinterpret_cast<T*>(pos), reinterpret_cast<T*>(vel),
                     reinterpret_cast<const T*>(grad_slow), reinterpret_cast<const T*>(inv_mass), bx, half_dt_acc_outer, dt_outer,
                     n_inner, c1, c2sq_kT_acc, seed, outer_step, E_dev, reinterpret_cast<T*>(grad_fast));
    HIP_TRY(hipGetLastError());
    mts.launches += 1;
  }
  void mts_info(int64_t* out) {
    mts.info(out, {mts.tiles.n_tiles, mts.tile_atoms, mts.max_component, mts.n_atoms, mts.n_bonds, mts.n_angles,
                   (int64_t)mts.lds_bytes, mts.launches});
  }

  // distance constraints (con_kernels.hip; admp_amd/md.py Constraints, ConstrainedLangevin); lds_bytes is that of
  // k_con_project, the largest of the three
  struct : PlanSlot<ConTiles<T>> { int max_cluster = 0, n_cons = 0, n_clusters = 0; } con;
  void con_plan(int n_atoms, int n_cons, const int32_t* pairs, const double* lengths, int tile_atoms) {
    single_rank();
    ARG_CHECK(n_atoms > 0 && n_atoms <= INT_MAX / 4 && n_cons >= 0, "bad argument");
    ARG_CHECK(n_cons == 0 || (pairs && lengths), "constraint lists missing");
    const ConPlan p = con_make_plan(n_atoms, n_cons, pairs, lengths, tile_atoms == 0 ? kConDefaultTileAtoms : tile_atoms);
    if (!p.error.empty()) throw Err{ADMP_E_ARG, p.error};
    const std::vector<T> hr(p.con_d2.begin(), p.con_d2.end());      // d^2 rounded to the handle's precision once
    const std::vector<size_t> off = con.upload(stream, {&p.tile_atom0, &p.atom_id, &p.tile_clu0, &p.clu_con0, &p.con_slot}, hr);
    const int* di = con.ints.template as<int>();
    ConTiles<T>& m = con.tiles;
    m.n_tiles = p.n_tiles; m.dims = p.dims;
    m.tile_atom0 = di + off[0]; m.atom_id = di + off[1]; m.tile_clu0 = di + off[2]; m.clu_con0 = di + off[3]; m.con_slot = di + off[4];
    m.con_d2 = con.reals.template as<T>();
    con.n_atoms = n_atoms; con.tile_atoms = p.tile_atoms; con.max_cluster = p.max_cluster; con.n_cons = n_cons;
    con.n_clusters = p.n_clusters;
    con.threads = mts_threads(p.tile_atoms);
    con.lds_bytes = con_lds_bytes(p.dims, sizeof(T), true);
    con.have = true;
  }
  Box<T> con_checked(const char* what, int n, const void* inv_mass, const double* box, double tol, int max_sweeps) {
    planned(con, "admp_md_con_plan", what, n, inv_mass, box);
    ARG_CHECK(tol >= 0.0 && std::isfinite(tol), "the tolerance must be finite and not negative");
    ARG_CHECK(max_sweeps >= 1, "max_sweeps must be at least 1");
    return finite_box(box);
  }
  void con_step(int n, void* pos, void* vel, const void* grad_, const void* inv_mass, const double* box, double half_dt_acc,
                double dt, double c1, double c2sq_kT_acc, uint64_t seed, uint64_t step, double tol, int max_sweeps,
                int32_t* counters_dev) {
    const Box<T> bx = con_checked("admp_md_con_step", n, inv_mass, box, tol, max_sweeps);
    ARG_CHECK(pos && vel && grad_, "bad argument");
    ARG_CHECK(dt > 0.0 && std::isfinite(dt) && std::isfinite(half_dt_acc), "dt must be positive and finite");
    ARG_CHECK(c1 >= 0.0 && c1 <= 1.0 && c2sq_kT_acc >= 0.0, "c1 must lie in [0, 1] and c2sq_kT_acc must not be negative");
    TIMED("md_con_step");
    launch_con_step<T>(stream, con.tiles, con.threads, reinterpret_cast<T*>(pos), reinterpret_cast<T*>(vel),
                       reinterpret_cast<const T*>(grad_), reinterpret_cast<const T*>(inv_mass), bx, half_dt_acc, dt, c1, c2sq_kT_acc, seed,
                       step, tol, max_sweeps, counters_dev);
    HIP_TRY(hipGetLastError());
    con.launches += 1;
  }
  void con_kick(int n, const void* pos, void* vel, const void* grad_, const void* inv_mass, const double* box, double half_dt_acc,
                double dt, double tol, int max_sweeps, double* ekin_dev, int32_t* counters_dev) {
    const Box<T> bx = con_checked("admp_md_con_kick", n, inv_mass, box, tol, max_sweeps);
    ARG_CHECK(pos && vel, "bad argument");
    ARG_CHECK(grad_ || half_dt_acc == 0.0, "a kick needs a gradient (half_dt_acc 0 with a NULL gradient is a pure projection)");
    ARG_CHECK(dt > 0.0 && std::isfinite(dt) && std::isfinite(half_dt_acc), "dt must be positive and finite");
    TIMED("md_con_kick");
    launch_con_kick<T>(stream, con.tiles, con.threads, reinterpret_cast<const T*>(pos), reinterpret_cast<T*>(vel),
                       reinterpret_cast<const T*>(grad_), reinterpret_cast<const T*>(inv_mass), bx, half_dt_acc, dt, tol, max_sweeps,
                       ekin_dev, counters_dev);
    HIP_TRY(hipGetLastError());
    con.launches += 1;
  }
  void con_project(int n, void* pos, const void* ref, const void* inv_mass, const double* box, double tol, int max_sweeps,
                   int32_t* counters_dev) {
    const Box<T> bx = con_checked("admp_md_con_project", n, inv_mass, box, tol, max_sweeps);
    ARG_CHECK(pos && ref, "bad argument");
    TIMED("md_con_project");
    launch_con_project<T>(stream, con.tiles, con.threads, reinterpret_cast<T*>(pos), reinterpret_cast<const T*>(ref),
                          reinterpret_cast<const T*>(inv_mass), bx, tol, max_sweeps, counters_dev);
    HIP_TRY(hipGetLastError());
    con.launches += 1;
  }
  void con_info(int64_t* out) {
    con.info(out, {con.tiles.n_tiles, con.tile_atoms, con.max_cluster, con.n_atoms, con.n_cons, con.n_clusters,
                   (int64_t)con.lds_bytes, con.launches});
  }

  // molecular cell scaling (mol_kernels.hip; admp_amd/md.py MolecularCRescaleBarostat): a plan of ints only
  struct : PlanSlot<MolTiles> { int max_group = 0, n_groups = 0; } mol;
  void mol_plan(int n_atoms, const int32_t* group_of, int tile_atoms) {
    single_rank();
    ARG_CHECK(n_atoms > 0 && n_atoms <= INT_MAX / 4 && group_of, "bad argument");
    const MolPlan p = mol_make_plan(n_atoms, group_of, tile_atoms == 0 ? kMolDefaultTileAtoms : tile_atoms);
    if (!p.error.empty()) throw Err{ADMP_E_ARG, p.error};
    const std::vector<size_t> off = mol.upload(stream, {&p.tile_atom0, &p.atom_id, &p.tile_grp0, &p.grp_atom0, &p.slot_grp});
    const int* di = mol.ints.template as<int>();
    MolTiles& m = mol.tiles;
    m.n_tiles = p.n_tiles; m.dims = p.dims;
    m.tile_atom0 = di + off[0]; m.atom_id = di + off[1]; m.tile_grp0 = di + off[2]; m.grp_atom0 = di + off[3]; m.slot_grp = di + off[4];
    mol.n_atoms = n_atoms; mol.tile_atoms = p.tile_atoms; mol.max_group = p.max_group; mol.n_groups = p.n_groups;
    mol.threads = mts_threads(p.tile_atoms);
    mol.lds_bytes = mol_lds_bytes(p.dims, sizeof(T));
    mol.have = true;
  }
  Box<T> mol_checked(const char* what, int n, const void* inv_mass, const double* box) {
    planned(mol, "admp_md_mol_plan", what, n, inv_mass, box);
    return finite_box(box);
  }
  void mol_sums(int n, const void* pos, const void* vel, const void* grad_, const void* inv_mass, const double* box, uint64_t seed,
                uint64_t step, double* out_dev) {
    const Box<T> bx = mol_checked("admp_md_mol_sums", n, inv_mass, box);
    ARG_CHECK(pos && vel && grad_ && out_dev, "bad argument");
    TIMED("md_mol_sums");
    HIP_TRY(hipMemsetAsync(out_dev, 0, 21 * sizeof(double), stream));
    launch_md_mol_sums<T>(stream, mol.tiles, mol.threads, reinterpret_cast<const T*>(pos), reinterpret_cast<const T*>(vel),
                          reinterpret_cast<const T*>(grad_), reinterpret_cast<const T*>(inv_mass), bx, seed, step, out_dev);
    HIP_TRY(hipGetLastError());
    mol.launches += 1;
  }
  void mol_scale(int n, void* pos, void* vel, const void* inv_mass, const double* box, double mu_minus_1, double inv_mu_minus_1) {
    const Box<T> bx = mol_checked("admp_md_mol_scale", n, inv_mass, box);
    ARG_CHECK(pos && vel, "bad argument");
    // mu > 0 and finite, and the two factors belong to one mu: (1 + (mu - 1)) (1 + (1/mu - 1)) = 1
    ARG_CHECK(std::isfinite(mu_minus_1) && std::isfinite(inv_mu_minus_1) && mu_minus_1 > -1.0 && inv_mu_minus_1 > -1.0,
              "the scale factor must be finite and positive");
    ARG_CHECK(std::fabs((1.0 + mu_minus_1) * (1.0 + inv_mu_minus_1) - 1.0) <= 1e-12, "mu_minus_1 and inv_mu_minus_1 are not those of one factor");
    TIMED("md_mol_scale");
    launch_md_mol_scale<T>(stream, mol.tiles, mol.threads, reinterpret_cast<T*>(pos), reinterpret_cast<T*>(vel),
                           reinterpret_cast<const T*>(inv_mass), bx, mu_minus_1, inv_mu_minus_1);
    HIP_TRY(hipGetLastError());
    mol.launches += 1;
  }
  void mol_info(int64_t* out) {
    mol.info(out, {mol.tiles.n_tiles, mol.tile_atoms, mol.max_group, mol.n_atoms, mol.n_groups, (int64_t)mol.lds_bytes, mol.threads,
                   mol.launches});
  }

  // the FIRE minimiser (fire_kernels.hip, md_fire_math.h; admp_amd/md.py FireMinimizer): the driver owns the rows of partial
  // sums, the caller the state; every argument is checked before the first launch
  DevBuf fire_rows;
  void fire_step(int n, void* pos, void* vel, const void* grad_, const void* inv_mass, const double* par9, double ftol,
                 uint64_t call, double* state16_dev) {
    HIP_TRY(hipSetDevice(ctx.device));
    ARG_CHECK(ctx.snranks == 1, "the MD helpers serve single-rank handles only (slab-decomposed handle)");
    ARG_CHECK(n >= 0 && n <= INT_MAX / 4 && par9 && state16_dev && (n == 0 || (pos && vel && grad_ && inv_mass)), "bad argument");
    const double dt_max = par9[FIRE_P_DT_MAX], dt_min = par9[FIRE_P_DT_MIN], max_step = par9[FIRE_P_MAX_STEP];
    ARG_CHECK(std::isfinite(dt_max) && std::isfinite(dt_min) && std::isfinite(max_step) && dt_max > 0.0 && dt_min > 0.0 &&
              max_step > 0.0 && dt_min <= dt_max, "dt_min, dt_max and max_step must be finite and positive, dt_min <= dt_max");
    ARG_CHECK(par9[FIRE_P_N_DELAY] >= 0.0, "n_delay must not be negative");
    ARG_CHECK(std::isfinite(par9[FIRE_P_F_INC]) && par9[FIRE_P_F_INC] >= 1.0, "f_inc must be finite and at least 1");
    for (int w : {(int)FIRE_P_F_DEC, (int)FIRE_P_ALPHA_START, (int)FIRE_P_F_ALPHA})
      ARG_CHECK(par9[w] > 0.0 && par9[w] <= 1.0, "f_dec, alpha_start and f_alpha must lie in (0, 1]");
    ARG_CHECK(std::isfinite(ftol) && ftol >= 0.0, "ftol must be finite and not negative");
    fire_rows.need(kFireRowsBytes);
    TIMED("md_fire");
    const int rc = launch_md_fire<T>(stream, n, reinterpret_cast<T*>(pos), reinterpret_cast<T*>(vel),
                                     reinterpret_cast<const T*>(grad_), reinterpret_cast<const T*>(inv_mass), par9, ftol, call,
                                     fire_rows.as<double>(), state16_dev);
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("FIRE step: ") + hipGetErrorString((hipError_t)rc)};
  }

  // the velocity-rescaling thermostat (vrescale_kernels.hip, md_vrescale_math.h; admp_amd/md.py VRescale): the driver owns the
  // rows of partial sums, the caller the state; every argument is checked before the first launch
  DevBuf vr_rows;
  void vrescale(int n, void* vel, const void* grad_, const void* inv_mass, double half_dt_acc, int64_t n_dof, double kT_acc,
                double c, uint64_t seed, uint64_t step, uint64_t call, double* state16_dev) {
    single_rank();
    ARG_CHECK(n >= 0 && n <= INT_MAX / 4 && state16_dev && (n == 0 || (vel && inv_mass)), "bad argument");
    ARG_CHECK(n_dof >= 1, "n_dof must be at least 1");
    ARG_CHECK(c >= 0.0 && c <= 1.0, "c must lie in [0, 1]");
    ARG_CHECK(std::isfinite(kT_acc) && kT_acc >= 0.0, "kT_acc must be finite and not negative");
    ARG_CHECK(std::isfinite(half_dt_acc), "half_dt_acc must be finite");
    vr_rows.need(kVrRowsBytes);
    TIMED("md_vrescale");
    const int rc = launch_md_vrescale<T>(stream, n, reinterpret_cast<T*>(vel), reinterpret_cast<const T*>(grad_),
                                         reinterpret_cast<const T*>(inv_mass), half_dt_acc, n_dof, kT_acc, c, seed, step, call,
                                         vr_rows.as<double>(), state16_dev);
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("velocity rescaling: ") + hipGetErrorString((hipError_t)rc)};
  }

  // radial distribution functions (rdf_kernels.hip, rdf_math.h, rdf_plan.h; admp_amd/md.py RdfRecorder): needs no topology.  The
  // driver owns the scratch of the cell form; every argument is checked before anything is launched, the slab refusal first.
  CellScratch rdf_cells;
  ~MdDriver() override {
    (void)hipSetDevice(ctx.device);
    rdf_cells.release();
  }
  void rdf(int n, const void* pos, const double* box, const int32_t* tags, int n_types, double r_max, int n_bins, uint64_t* hist_dev,
           int force, int64_t* info4) {
    single_rank();
    ARG_CHECK(box && hist_dev && (n <= 0 || (pos && tags)), "bad argument (null pointer)");
    ARG_CHECK(n <= INT_MAX / 4, "bad argument");
    ARG_CHECK(std::isfinite(r_max), "r_max must be finite");
    const Box<T> bx = finite_box(box);
    double inv[9], vol, heights[3];
    invert3(box, inv, &vol);
    cell_heights(inv, heights);
    const RdfPlan p = rdf_make_plan(n, heights, r_max, n_types, n_bins, sizeof(T), force);
    if (p.error) throw Err{ADMP_E_ARG, p.error};
    if (info4) {
      info4[0] = p.form; info4[1] = p.workgroups; info4[2] = p.form == RDF_FORM_TILES ? p.n_tiles : p.n_cells;
      info4[3] = (int64_t)p.lds_bytes;
    }
    if (p.form == RDF_FORM_NONE) return;
    TIMED("md_rdf");
    const int rc = launch_rdf<T>(stream, p, n, reinterpret_cast<const T*>(pos), tags, bx, n_types, r_max, n_bins, rdf_cells,
                                 reinterpret_cast<unsigned long long*>(hist_dev));
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("radial distribution: ") + hipGetErrorString((hipError_t)rc)};
  }

  // time correlation functions (tcf_kernels.hip, tcf_math.h, tcf_plan.h; admp_amd/md.py CorrelationRecorder): the caller owns the
  // ring, the state and the accumulators, the driver the partial sums of one call; every argument is checked before anything is
  // launched or written, the slab refusal first.  Growing tcf_rows is the one host synchronisation.
  DevBuf tcf_rows;
  void tcf(int n, const void* pos, const void* vel, const double* box, int n_slots, const int32_t* slot_atom, int n_tiles,
           const int32_t* tile_type, int tile_atoms, int n_types, int n_lags, int64_t frame, void* ring, double* unwrapped, void* last,
           uint64_t* jumps, double* acc, int64_t* info4) {
    single_rank();
    ARG_CHECK(box && acc && ring && unwrapped && last && jumps, "bad argument (null pointer)");
    ARG_CHECK(n_slots <= 0 || (pos && vel && slot_atom && tile_type), "bad argument (null pointer)");
    const TcfPlan p = tcf_make_plan(n, n_slots, n_tiles, tile_atoms, n_types, n_lags, frame);
    if (p.error) throw Err{ADMP_E_ARG, p.error};
    (void)finite_box(box);
    double inv[9], vol;
    const Box<double> bx = make_box<double>(box, inv, &vol);
    const bool launch = n_slots > 0 && p.workgroups > 0;
    if (info4) {
      info4[0] = launch ? p.workgroups : 0; info4[1] = kTcfLagsPerWg; info4[2] = launch ? p.lags_now : 0;
      info4[3] = launch ? (int64_t)p.scratch_bytes : 0;
    }
    if (!launch) return;
    tcf_rows.need(p.scratch_bytes);
    TIMED("md_tcf");
    const int rc = launch_tcf<T>(stream, p, n, reinterpret_cast<const T*>(pos), reinterpret_cast<const T*>(vel), bx, n_slots, slot_atom,
                                 n_tiles, tile_type, tile_atoms, n_types, n_lags, frame, reinterpret_cast<T*>(ring), unwrapped,
                                 reinterpret_cast<T*>(last), reinterpret_cast<unsigned long long*>(jumps), tcf_rows.as<double>(), acc);
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("time correlation functions: ") + hipGetErrorString((hipError_t)rc)};
  }
};

template <class T>
MdDriver<T>& driver_of(HandleCtx& c) {
  if (!c.md) c.md.reset(new MdDriver<T>(c));
  return static_cast<MdDriver<T>&>(*c.md);
}

// f(driver) inside handle_call, on the driver of the handle's precision
template <class F>
int md_call(admp_handle* h, F&& f) {
  return handle_call(h, [&](HandleCtx& c) {
    if (c.prec == 4) f(driver_of<float>(c));
    else f(driver_of<double>(c));
  });
}

}  // namespace

extern "C" {

int admp_md_bonded(admp_handle* h, const void* positions, const double* box, int n_bonds, const int32_t* bond_idx,
                   const void* bond_par, int n_angles, const int32_t* angle_idx, const void* angle_par, double* E_dev,
                   void* grad_inout) {
  return md_call(h, [&](auto& md) {
    md.bonded(positions, box, n_bonds, bond_idx, bond_par, n_angles, angle_idx, angle_par, E_dev, grad_inout);
  });
}
int admp_md_kick_drift(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* grad, const void* inv_mass,
                       double half_dt_acc, double dt, double* ekin_dev) {
  return md_call(h, [&](auto& md) { md.kick_drift(n_atoms, positions, velocities, grad, inv_mass, half_dt_acc, dt, ekin_dev); });
}
int admp_md_langevin(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* grad, const void* inv_mass,
                     double half_dt_acc, double dt, double c1, double c2sq_kT_acc, uint64_t seed, uint64_t step,
                     double* ekin_dev) {
  return md_call(h, [&](auto& md) {
    md.langevin(n_atoms, positions, velocities, grad, inv_mass, half_dt_acc, dt, c1, c2sq_kT_acc, seed, step, ekin_dev);
  });
}
int admp_md_random(admp_handle* h, int kind, int64_t n, uint64_t seed, uint64_t step, uint32_t stream, void* out) {
  return md_call(h, [&](auto& md) { md.random(kind, n, seed, step, stream, out); });
}
int admp_md_bonded_box(admp_handle* h, const void* positions, const double* box, int n_bonds, const int32_t* bond_idx,
                       const void* bond_par, int n_angles, const int32_t* angle_idx, const void* angle_par, double* E_dev,
                       double* S_dev) {
  return md_call(h, [&](auto& md) {
    md.bonded_box(positions, box, n_bonds, bond_idx, bond_par, n_angles, angle_idx, angle_par, E_dev, S_dev);
  });
}
int admp_md_virial(admp_handle* h, int n_atoms, const void* positions, const void* velocities, const void* grad,
                   const void* inv_mass, uint64_t seed, uint64_t step, double* out_dev) {
  return md_call(h, [&](auto& md) { md.virial(n_atoms, positions, velocities, grad, inv_mass, seed, step, out_dev); });
}
int admp_md_scale(admp_handle* h, int n_atoms, void* positions, void* velocities, double mu) {
  return md_call(h, [&](auto& md) { md.scale(n_atoms, positions, velocities, mu); });
}
int admp_md_mts_plan(admp_handle* h, int n_atoms, int n_bonds, const int32_t* bond_idx, const double* bond_par, int n_angles,
                     const int32_t* angle_idx, const double* angle_par, int tile_atoms) {
  return md_call(h, [&](auto& md) { md.mts_plan(n_atoms, n_bonds, bond_idx, bond_par, n_angles, angle_idx, angle_par, tile_atoms); });
}
int admp_md_mts_step(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* grad_slow, const void* inv_mass,
                     const double* box, double half_dt_acc_outer, double dt_outer, int n_inner, double c1, double c2sq_kT_acc,
                     uint64_t seed, uint64_t outer_step, double* E_dev, void* grad_fast_out) {
  return md_call(h, [&](auto& md) {
    md.mts_step(n_atoms, positions, velocities, grad_slow, inv_mass, box, half_dt_acc_outer, dt_outer, n_inner, c1, c2sq_kT_acc,
                seed, outer_step, E_dev, grad_fast_out);
  });
}
int admp_md_mts_info(admp_handle* h, int64_t* out8) {
  return md_call(h, [&](auto& md) { md.mts_info(out8); });
}
int admp_md_con_plan(admp_handle* h, int n_atoms, int n_constraints, const int32_t* pairs, const double* lengths, int tile_atoms) {
  return md_call(h, [&](auto& md) { md.con_plan(n_atoms, n_constraints, pairs, lengths, tile_atoms); });
}
int admp_md_con_step(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* grad, const void* inv_mass,
                     const double* box, double half_dt_acc, double dt, double c1, double c2sq_kT_acc, uint64_t seed, uint64_t step,
                     double tolerance, int max_sweeps, int32_t* counters_dev) {
  return md_call(h, [&](auto& md) {
    md.con_step(n_atoms, positions, velocities, grad, inv_mass, box, half_dt_acc, dt, c1, c2sq_kT_acc, seed, step, tolerance,
                max_sweeps, counters_dev);
  });
}
int admp_md_con_kick(admp_handle* h, int n_atoms, const void* positions, void* velocities, const void* grad, const void* inv_mass,
                     const double* box, double half_dt_acc, double dt, double tolerance, int max_sweeps, double* ekin_dev,
                     int32_t* counters_dev) {
  return md_call(h, [&](auto& md) {
    md.con_kick(n_atoms, positions, velocities, grad, inv_mass, box, half_dt_acc, dt, tolerance, max_sweeps, ekin_dev, counters_dev);
  });
}
int admp_md_con_project(admp_handle* h, int n_atoms, void* positions, const void* reference, const void* inv_mass, const double* box,
                        double tolerance, int max_sweeps, int32_t* counters_dev) {
  return md_call(h, [&](auto& md) { md.con_project(n_atoms, positions, reference, inv_mass, box, tolerance, max_sweeps, counters_dev); });
}
int admp_md_con_info(admp_handle* h, int64_t* out8) {
  return md_call(h, [&](auto& md) { md.con_info(out8); });
}
int admp_md_mol_plan(admp_handle* h, int n_atoms, const int32_t* group_of, int tile_atoms) {
  return md_call(h, [&](auto& md) { md.mol_plan(n_atoms, group_of, tile_atoms); });
}
int admp_md_mol_sums(admp_handle* h, int n_atoms, const void* positions, const void* velocities, const void* grad, const void* inv_mass,
                     const double* box, uint64_t seed, uint64_t step, double* out21_dev) {
  return md_call(h, [&](auto& md) { md.mol_sums(n_atoms, positions, velocities, grad, inv_mass, box, seed, step, out21_dev); });
}
int admp_md_mol_scale(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* inv_mass, const double* box,
                      double mu_minus_1, double inv_mu_minus_1) {
  return md_call(h, [&](auto& md) { md.mol_scale(n_atoms, positions, velocities, inv_mass, box, mu_minus_1, inv_mu_minus_1); });
}
int admp_md_mol_info(admp_handle* h, int64_t* out8) {
  return md_call(h, [&](auto& md) { md.mol_info(out8); });
}
int admp_md_fire_step(admp_handle* h, int n_atoms, void* positions, void* velocities, const void* grad, const void* inv_mass,
                      const double* params9, double ftol, uint64_t call, double* state16_dev) {
  return md_call(h, [&](auto& md) { md.fire_step(n_atoms, positions, velocities, grad, inv_mass, params9, ftol, call, state16_dev); });
}
int admp_md_vrescale(admp_handle* h, int n_atoms, void* velocities, const void* grad, const void* inv_mass, double half_dt_acc,
                     int64_t n_dof, double kT_acc, double c, uint64_t seed, uint64_t step, uint64_t call, double* state16_dev) {
  return md_call(h, [&](auto& md) {
    md.vrescale(n_atoms, velocities, grad, inv_mass, half_dt_acc, n_dof, kT_acc, c, seed, step, call, state16_dev);
  });
}
int admp_md_rdf(admp_handle* h, int n_atoms, const void* positions_dev, const double* box, const int32_t* tags_dev, int n_types,
                double r_max, int n_bins, uint64_t* hist_dev, int force, int64_t* info4) {
  return md_call(h, [&](auto& md) { md.rdf(n_atoms, positions_dev, box, tags_dev, n_types, r_max, n_bins, hist_dev, force, info4); });
}
int admp_md_tcf(admp_handle* h, int n_atoms, const void* positions_dev, const void* velocities_dev, const double* box, int n_slots,
                const int32_t* slot_atom_dev, int n_tiles, const int32_t* tile_type_dev, int tile_atoms, int n_types, int n_lags,
                int64_t frame, void* ring_dev, double* unwrapped_dev, void* last_dev, uint64_t* jumps_dev, double* acc_dev,
                int64_t* info4) {
  return md_call(h, [&](auto& md) {
    md.tcf(n_atoms, positions_dev, velocities_dev, box, n_slots, slot_atom_dev, n_tiles, tile_type_dev, tile_atoms, n_types, n_lags,
           frame, ring_dev, unwrapped_dev, last_dev, jumps_dev, acc_dev, info4);
  });
}

}  // extern "C"
