// libadmp_hip: handle, device buffers, and the orchestration of one get_energy / get_forces evaluation behind the C ABI of
// include/admp_hip.h.  The k-space leg between spread and gather (rocFFT plans, tables, every transform path) is MeshConv,
// mesh_conv.hip; the neighbour table between two evaluations (builds, site classes, inner lists, loans) and the cell-list search
// are PairList, pair_list.hip; what a topology implies for the closing kernels is topology_plan.h; the decomposition of a slab
// rank and its halo exchanges are SlabDecomp, slab_decomp.hip; the MD entries are md_driver.hip.
//
// Flow of admp_pme_energy_grad (reference call stack: admp/pme.py:58-86 get_energy ->
// :111-143 optimize_Uind -> :176-254 energy_pme, gradient by jax.value_and_grad :108):
//   prepare_sites   local frames, Q_local -> Q_global, packed site rows           [atom_kernels.hip]
//   (polarizable)   Jacobi SCF: pair_field + spread/r2c/kspace/c2r/gather_field + field_finish,
//                   one host read of max|field| per cycle (the reference syncs there too, pme.py:136)
//   pair_full       real-space energy, dE/dr, dE/dQ                                 [pair_kernels.hip]
//   spread, r2c, kspace (energy + G multiply), c2r, gather                          [recip_kernels.hip; mesh_conv.hip]
//   finish          self + penalty, frame adjoint, dE/dQ_local                      [atom_kernels.hip]
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <functional>
#include <vector>

#include "../../include/admp_hip.h"
#include "comm.h"
#include "dev_buf.h"
#include "dft_math.h"
#include "dipole_math.h"
#include "disp_plan.h"
#include "handle.h"
#include "launch.h"
#include "mesh_conv.h"
#include "pair_list.h"
#include "rccl_comm.h"
#include "scf_policy.h"
#include "scf_aspc.h"
#include "slab_decomp.h"
#include "topology_plan.h"

using namespace admp;

namespace {

static_assert(kTopoZBisect == ZBisect && kTopoThreeFold == ThreeFold && kTopoZonly == Zonly && kTopoNoAxis == NoAxisType,
              "topology_plan.h restates the axis rules of frame_math.h");

// the device arrays behind the Topology view the kernels take
struct TopologyStore {
  DevBuf axis_type, axis_idx, excl_ptr, excl_col, excl_nb, inv_ptr, inv_idx, grp_ptr, rows_blk, grp_of, gath_blk;
  // n words of src in b (at least one word is allocated, so that an empty array has an address too)
  static int* put(DevBuf& b, const int32_t* src, size_t n) {
    b.need(sizeof(int) * std::max<size_t>(n, 1));
    if (n > 0) HIP_TRY(hipMemcpy(b.p, src, sizeof(int) * n, hipMemcpyHostToDevice));
    return b.as<int>();
  }
  void release() {
    for (DevBuf* b : {&axis_type, &axis_idx, &excl_ptr, &excl_col, &excl_nb, &inv_ptr, &inv_idx, &grp_ptr, &rows_blk, &grp_of, &gath_blk})
      b->release();
  }
};

struct EngineBase : HandleCtx {      // device, prec, stream, own_stream, prof, srank, snranks, md (handle.h)
  virtual ~EngineBase() {}
  Topology top;                 // a view of top_d
  TopologyStore top_d;
  PairList pl{this};            // the neighbour table and all that happens to it between evaluations (pair_list.h)
  bool have_top = false, have_ewald = false;
  double kappa = 0;
  int K[3] = {0, 0, 0};
  int lmax = 2, lpol = 0;
  Comm comm;                    // the collectives of a decomposed evaluation (comm.h)
  // how the polarizable calls of this handle were enqueued and how the guesses behind it turned out (admp_scf_stats):
  // [0] plain calls, [1] speculative calls, [2] ... whose first check failed (closing pass wasted), [3] chained calls,
  // [4] ... that needed more steps than enqueued (closing pass wasted), [5] ... that enqueued more steps than needed,
  // [6] increments that ran for nothing in those, [7] Jacobi steps in total
  int64_t scf_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  MeshStats mesh_stats;         // counters of the direct-DFT convolution (admp_xpass_stats, admp_plane_mfma_stats[4]); mesh_conv.h
  // closing pair kernels of polarizable calls (admp_pair_rider_stats): [0] rode in an x pass, [1] launched on their own
  int64_t pair_rider_stats[2] = {0, 0};
  // admp_scf_aspc: predictor-corrector dipoles for consecutive polarizable calls (scf_aspc.h).  The ring arithmetic lives
  // here, the dipole sets themselves in the engine's device buffers.  aspc_calls: [0] calls that ran the fixed form,
  // [1] warm-up calls, [2] fallback calls; aspc_resid: max|dE/dU| at the predicted dipoles of the last fixed-form call
  AspcRing aspc;
  int64_t aspc_calls[3] = {0, 0, 0};
  double aspc_resid = 0.0;
  int aspc_hold = 0;            // ADMP_OPT_ASPC_HOLD: the calls are not time steps, the history stays as it is
  bool aspc_dirty = false;      // a copy into the ring's next slot has been enqueued and not yet counted
  void aspc_off() { aspc.configure(-1, 1, 0.0); aspc_dirty = false; }
  const void* U_src = nullptr;  // admp_set_dipole_source: read-only initial dipoles of the NEXT polarizable evaluation
  const void* U_src_now = nullptr;   // ... taken over by that evaluation (Engine::pme), consumed by its site pass
  double cutoff = 0.0;          // admp_set_cutoff: listed pairs beyond it are skipped (0: every listed pair, as the reference)
  int ref_korder = 0;           // ADMP_OPT_REFERENCE_KPOINTS: the reference's k-point table (k_gtab)
  int keep_pol_sites = 0;       // ADMP_OPT_KEEP_POL_SITES: the caller vouches that the set {i : pol_i > 0} has not changed
  int side_stream_on = 1;       // ADMP_OPT_SIDE_STREAM: 0 keeps every kernel on the handle's stream (clean per-kernel event times)
  // a call that failed half way: whatever it left on a helper stream is waited for before the error is reported
  virtual void after_error() {}
  // the topology is being replaced or freed: whatever the engine remembers of the atoms it described goes too
  virtual void topology_gone() {}
  // admp_share_neighbors: the calculators of one system walk ONE compiled table instead of compiling the same pair list once each
  void share_neighbors(EngineBase* src) {
    ARG_CHECK(have_top, "admp_set_topology must precede admp_share_neighbors");
    if (!src) { pl.end_loan(); return; }
    ARG_CHECK(src != this && src->pl.owned(), "the lender must own its neighbour table");
    ARG_CHECK(src->have_top && src->top.na == top.na && src->device == device, "handles of different systems / devices");
    pl.borrow(&src->pl, top.na);
  }

  virtual void set_ewald(double kappa_, int K1, int K2, int K3, int lmax_, int lpol_) = 0;
  virtual void pme(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, int ns,
                   const double* mS, const double* pS, void* U, int max_cycle, double thresh, double* E, void* dpos,
                   void* dQl, int* ncyc, int* conv, int on_device) = 0;
  virtual void pme_at_U(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, int ns,
                        const double* mS, const double* pS, const void* U, double* E, void* dpos, void* dU, void* dQl) = 0;
  virtual void local_frames(const void* pos, const double* box, void* out) = 0;
  virtual void dipoles(const void* pos, const double* box, const void* Ql, const void* U, const void* inv_mass, int n_groups,
                       const int32_t* group_start, const int32_t* group_atoms, double* mu_groups, double* out16) = 0;
  virtual void mesh_convolve(const double* box, int which, void* data, int on_device, double* E_out, int32_t* info) = 0;
  virtual void slab_mesh_convolve(const double* box, int which, void* data, int on_device, double* E_out, int32_t* info) = 0;
  virtual void pair_program_eval(int id, const void* pos, const double* box, const void* par, int ns, const double* mS,
                                 double* E, void* dpos, int on_device) = 0;

  // ---- user-defined pair kernels (admp_amd/xp.py traces a Python kernel into HIP source; compiled here with hiprtc) ----
  struct PairProgram { hipModule_t mod = nullptr; hipFunction_t fn = nullptr; int n_params = 0; };
  std::vector<PairProgram> programs;
  int pair_program_build(const char* source, int n_params) {
    ARG_CHECK(source && n_params >= 0 && n_params <= 16, "bad pair program");
    hiprtcProgram prog = nullptr;
    auto rtc = [&](hiprtcResult r, const char* what) {
      if (r != HIPRTC_SUCCESS) throw Err{ADMP_E_HIP, std::string(what) + ": " + hiprtcGetErrorString(r)};
    };
    rtc(hiprtcCreateProgram(&prog, source, "admp_pair_custom.hip", 0, nullptr, nullptr), "hiprtcCreateProgram");
    const char* opts[] = {"--offload-arch=gfx950", "-O3", prec == 4 ? "-DREAL_T=float" : "-DREAL_T=double"};
    const hiprtcResult cr = hiprtcCompileProgram(prog, 3, opts);
    if (cr != HIPRTC_SUCCESS) {
      size_t n = 0;
      std::string log;
      if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) { log.resize(n); (void)hiprtcGetProgramLog(prog, &log[0]); }
      (void)hiprtcDestroyProgram(&prog);
      throw Err{ADMP_E_HIP, std::string("hiprtc could not compile the traced pair kernel: ") + log.substr(0, 1500)};
    }
    size_t sz = 0;
    rtc(hiprtcGetCodeSize(prog, &sz), "hiprtcGetCodeSize");
    std::vector<char> code(sz);
    rtc(hiprtcGetCode(prog, code.data()), "hiprtcGetCode");
    (void)hiprtcDestroyProgram(&prog);
    PairProgram p;
    p.n_params = n_params;
    HIP_TRY(hipModuleLoadData(&p.mod, code.data()));
    HIP_TRY(hipModuleGetFunction(&p.fn, p.mod, "admp_pair_custom"));
    programs.push_back(p);
    return (int)programs.size() - 1;
  }
  void free_programs() {
    for (auto& p : programs) if (p.mod) (void)hipModuleUnload(p.mod);
    programs.clear();
  }
  virtual void pme_box_grad(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, int ns,
                            const double* mS, const double* pS, const void* U, double* E, double* dbox) = 0;
  virtual void disp_box_grad(const void* pos, const double* box, const void* clist, int pmax, int ns, const double* mS,
                             double* E, double* dbox) = 0;
  virtual void tt_box_grad(const void* pos, const double* box, const void* abqc, int ns, const double* mS, double* E,
                           double* dbox) = 0;
  virtual void disp_set_types(int nt, const void* types, const double* ctab) = 0;
  virtual void disp(const void* pos, const double* box, const void* clist, int pmax, int ns, const double* mS, double* E,
                    void* dpos, int on_device) = 0;
  virtual void tt(const void* pos, const double* box, const void* abqc, int ns, const double* mS, double* E, void* dpos,
                  int on_device) = 0;
  virtual void disp_mesh_spread(const void* pos, const double* box, const void* clist, int pmax, int on_device, void* mesh_out,
                                double* E_self_out, int32_t* info8) = 0;
  virtual void disp_mesh_gather(const void* pos, const double* box, const void* clist, int pmax, const void* phi, int which,
                                int on_device, double* E_self_out, void* out, int32_t* info8) = 0;
  virtual void disp_param_grad(const void* pos, const double* box, const void* clist, int pmax, int ns, const double* mS,
                               void* out) = 0;
  virtual void tt_param_grad(const void* pos, const double* box, const void* abqc, int ns, const double* mS, void* out) = 0;
  virtual void thole_sums(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, int ns,
                          const double* mS, const double* pS, const void* U, void* sumX, void* sumXw) = 0;
  virtual void pscale_grad(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, int ns,
                           const double* mS, const double* pS, const void* U, double* out) = 0;
  virtual void pair_real(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, int ns,
                         const double* mS, const double* pS, const void* U, const void* F, int which, int flags, int on_device,
                         double* E_out, void* grad, void* pot, void* fld, int32_t* info) = 0;
  virtual void mesh_spread(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, const void* U,
                           int which, int flags, int on_device, void* mesh_out, int32_t* info) = 0;
  virtual void mesh_gather(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, const void* U,
                           const void* phi, int which, int on_device, double* E_out, void* pot, void* grad, void* fld,
                           int32_t* info) = 0;
  virtual void site_table(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, const void* U,
                          int on_device, void* sites_out, int32_t* act_out, int32_t* info) = 0;
  virtual void site_close(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, const void* U,
                          const void* pot_in, const void* phi_in, int which, int want_dQ, int on_device, double* E_out,
                          void* grad_out, void* dQ_out, double* vir_out, int32_t* info) = 0;
  virtual void mscale_grad(int kind, const void* pos, const double* box, const void* par, int pmax, int ns, double* out,
                           int on_device) = 0;
  virtual void nbr_count(int na, const void* pos, const double* box, double rc, int64_t* n_pairs) = 0;
  virtual void nbr_fill(int32_t* pairs) = 0;
  virtual void nbr_table(const void* pos, const double* box, double rc) = 0;
  virtual void prune_pairs(const void* pos, const double* box, double rc) = 0;
  virtual void slab_info(int64_t* out) = 0;
  virtual void slab_home(int32_t* out, int* n_home, int* n_import) = 0;
  virtual void slab_lists(int na, int nranks, int32_t* owner, int32_t* bits, int32_t* home, int32_t* rows, int32_t* act,
                          int32_t* imp, int32_t* exp, int32_t* mig_in, int32_t* mig_out, int64_t* counts) = 0;

  void free_topology() {
    top_d.release();
    top = Topology();
    pl.drop();
    topology_gone();
    slab_sites_na = -1;
    have_top = false;
  }
  int slab_sites_na = -1;       // slab rank: every row of the site table (at slab_sites_ptr) has been prepared at least once
  const void* slab_sites_ptr = nullptr;   //     for a system of this many atoms (Engine::stage_begin)

  void set_topology(int na, const int32_t* atype, const int32_t* aidx, const int32_t* eptr, const int32_t* ecol,
                    const int32_t* enb) {
    ARG_CHECK(na > 0 && na <= kColMask, "n_atoms out of range");
    aspc.drop();                // dipoles of another system
    free_topology();
    top.na = na;
    std::vector<int32_t> t5(na, NoAxisType), idx(3 * (size_t)na, -1);
    const int32_t* at = atype ? atype : t5.data();
    const int32_t* ai = aidx ? aidx : idx.data();
    for (int i = 0; i < na; ++i) {
      ARG_CHECK(at[i] >= 0 && at[i] <= 5, "axis_type outside 0..5");
      for (int k = 0; k < 3; ++k) ARG_CHECK(ai[3 * i + k] >= -1 && ai[3 * i + k] < na, "axis index out of range");
    }
    top.axis_type = TopologyStore::put(top_d.axis_type, at, (size_t)na);
    top.axis_idx = TopologyStore::put(top_d.axis_idx, ai, 3 * (size_t)na);
    if (eptr) {
      int nnz = eptr[na];
      ARG_CHECK(nnz >= 0, "bad exclusion rowptr");
      for (int k = 0; k < nnz; ++k) ARG_CHECK(ecol[k] >= 0 && ecol[k] < na && enb[k] >= 0 && enb[k] <= kNbMask,
                                                "bad exclusion entry (atom index out of range, or nbonds outside 0..7)");
      top.excl_ptr = TopologyStore::put(top_d.excl_ptr, eptr, (size_t)na + 1);
      top.excl_col = TopologyStore::put(top_d.excl_col, ecol, (size_t)nnz);
      top.excl_nb = TopologyStore::put(top_d.excl_nb, enb, (size_t)nnz);
    }
    // the inverse frame map for the atomics-free closing kernel and, where the frames allow them, the frame groups (topology_plan.h)
    static const bool groups_on = env_flag("ADMP_FINISH_GROUPS", true);
    const TopologyPlan p = topology_plan(na, at, ai, kMaxGroup, kFinishBlock, kGatherRun, groups_on);
    top.inv_ptr = TopologyStore::put(top_d.inv_ptr, p.inv_ptr.data(), p.inv_ptr.size());
    top.inv_idx = TopologyStore::put(top_d.inv_idx, p.inv_idx.data(), p.inv_idx.size());
    if (!p.grp_ptr.empty()) {
      top.grp_ptr = TopologyStore::put(top_d.grp_ptr, p.grp_ptr.data(), p.grp_ptr.size());
      top.ngroups = (int)p.grp_ptr.size() - 1;
      top.gath_blk = TopologyStore::put(top_d.gath_blk, p.gath_blk.data(), p.gath_blk.size());
      top.ngathblk = (int)p.gath_blk.size() - 1;
      top.rows_blk = TopologyStore::put(top_d.rows_blk, p.rows_blk.data(), p.rows_blk.size());
      top.nrowblk = (int)p.rows_blk.size() - 1;
      top.grp_of = TopologyStore::put(top_d.grp_of, p.grp_of.data(), p.grp_of.size());
    }
    have_top = true;
  }

  void set_pairs(int64_t n_rows, const int32_t* pairs, int on_device) {
    ARG_CHECK(have_top, "admp_set_topology must precede admp_set_pairs");
    pl.set_pairs(top, n_rows, pairs, on_device);
  }
};

template <class T>
struct Engine : EngineBase {
  // per-atom
  DevBuf sites, grad, pot, fld_pair, fld_recip, field, energies_d;
  bool fmax_clean = false, slot_clean[E_SLOTS] = {false};
  // The energy words are double-buffered: the evaluation of step n accumulates into half (n & 1) while its first
  // kernel zeroes the other half for step n+1 -- no memset dispatch per step.  Eh is pinned host memory for the
  // one device-to-host copy of a step.
  int ehalf = 0;
  bool other_clean = false;
  void* energies_seen = nullptr;
  double* Eh = nullptr;
  double* Ed_cur() { return energies_d.as<double>() + (size_t)ehalf * E_WORDS; }
  // staging for host-pointer calls
  DevBuf s_pos, s_Q, s_pol, s_thole, s_U, s_out, s_dQ, s_par;
  // mesh: the real meshes belong to spread and gather as much as to the transform; everything of the k-space leg between
  // them (plans, spectrum, G tables, slab bounds and transposes) is mc's (mesh_conv.h)
  DevBuf mesh, bin_cells, bin_sorted, bin_scan, bin_cells_ind, bin_sorted_ind;
  MeshConv<T> mc{this, &comm, &mesh_stats};
  BinScratch bins, bins_ind;   // brick lists of the site rows / of the compact rows of the SCF increments
  DevBuf home_list;
  DevBuf act_tmp, sort_scratch;  // sort_scratch: hipcub's, grown by sort_ints (sort_bytes)
  size_t sort_bytes = 0;
  DevBuf onehot_d, tcount_d;     // typed dispersion of small systems: (Na, n_types) one-hot weights; scratch of the type counts
  void* onehot_for = nullptr;    // ... built in this allocation
  DevBuf act_d, isites, mesh2;   // incremental SCF: polarizable-site list, their compact delta rows, the increment's mesh
  IndTable ind;                  // ... and the polarizable-polarizable part of the neighbour table
  // admp_set_cutoff (a Verlet list with a skin): each evaluation with a cutoff first writes the inner table of the table it walks
  // (pl.table(), whichever it is) at its own site rows, and all its multipolar pair passes walk that copy (build_cut_table).
  // Allocated on the first such evaluation; cutoff 0 walks pl.table() / ind as before.
  DevBuf cut_end, cut_col, cut_iend, cut_icol;
  NbrTable cut_nbr;
  IndTable cut_ind;
  bool cut_on = false;           // this evaluation walks cut_nbr / cut_ind
  const NbrTable& wnbr() const { return cut_on ? cut_nbr : pl.table(); }
  const IndTable& wind() const { return cut_on ? cut_ind : ind; }
  long act_gen = 0, act_top_na = -1;   // act_gen: bumped when the list is rebuilt; the list belongs to a topology of act_top_na atoms
  int act_n = -1;                // its length once the host has seen it (-1: not yet)
  bool act_fresh = false;        // this evaluation rebuilt the list (count still on the device)
  long ind_nbr_gen = -1, ind_act_gen = -1;
  long eval_seq = 0, ind_bins_eval = -1, ind_bins_gen = -1;   // evaluation counter; the evaluation / active set bins_ind was built for
  int ind_bins_n = -1;
  const int* ind_bins_at = nullptr;
  DevBuf bases_d;         // int4 per atom: lowest stencil index on each mesh axis
  static_assert(kScfChainSteps == E_CHAIN, "one residual word per chained Jacobi step");
  ScfHistory scf;             // residual history of the polarizable calls of this handle: picks the form of the next one
  bool mono_ok = false;       // this evaluation may use the charge-only pair forms (no dE/dQ_local requested)

  // Every DevBuf member frees itself after this body, so after the stream is gone: hipFree needs no stream, and admp_destroy
  // has set the device and synchronised the stream before it deletes the handle.  The rocFFT plans are mc's, but they go here,
  // by a call at the head of this body, so that they are destroyed before the stream as they always were; mc's own
  // destructor then finds none left.
  ~Engine() override {
    mc.destroy_plans();
    free_topology();
    if (ind.end) (void)hipFree(ind.end);      // (grown by build_ind_table with hipMalloc into the plain struct the kernels take)
    if (ind.col) (void)hipFree(ind.col);
    free_programs();
    if (Eh) (void)hipHostFree(Eh);
    prof.destroy();
    if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }

  void set_ewald(double kappa_, int K1, int K2, int K3, int lmax_, int lpol_) override {
    ARG_CHECK(kappa_ > 0, "kappa must be positive");
    ARG_CHECK(K1 >= 2 && K2 >= 2 && K3 >= 2, "PME mesh must be at least 2 points per dimension");   // (spline users: make_geom)
    ARG_CHECK(lmax_ >= 0 && lmax_ <= 2, "l > 2 (beyond quadrupole) not supported");   // admp/recip.py:275
    kappa = kappa_; K[0] = K1; K[1] = K2; K[2] = K3; lmax = lmax_; lpol = lpol_ ? 1 : 0;
    have_ewald = true;
    aspc.drop();                // the stored dipoles belong to the old parameters
    if (!lpol) aspc_off();
  }

  // ---- slab bounds: rank s owns mesh planes [X0, X1) along x, plus kGhost overhang planes above X1 (MeshConv::update_slab) ----
  static constexpr int kGhost = MeshConv<T>::kGhost;
  void update_slab() { mc.update_slab(K); }
  // ---- the decomposition of one evaluation and its halo exchanges (snranks > 1): sl, slab_decomp.h -------------------------
  SlabDecomp<T> sl{this, &comm};
  void topology_gone() override { sl.forget(); }
  // K0v / X0v / X1v: the planes the ownership rule works on (the PME mesh's; a handle without a mesh takes a virtual one)
  typename SlabDecomp<T>::In slab_in(const int4* bases, const T* pol, int K0v, int X0v, int X1v, const int* order, bool with_dipoles) {
    typename SlabDecomp<T>::In in;
    in.na = top.na; in.nbr = &pl.table(); in.top = &top; in.bases = bases; in.pol = pol;
    in.K0v = K0v; in.X0v = X0v; in.X1v = X1v; in.order = order; in.with_dipoles = with_dipoles;
    return in;
  }
  // the decomposition of an electrostatics evaluation on the PME mesh: its home atoms become the evaluation's, the dipoles of
  // the atoms that changed hands go to their new owners and every rank gets the dipoles of the atoms it reads
  // (prepare: what the caller still has to do to the site rows once the lists are known, ahead of the exchanges that write them)
  template <class F>
  void decompose_eval(F&& prepare) {
    const bool tracked = sl.will_track(top.na, lpol != 0);      // (decompose() then lists the atoms that changed hands)
    sl.decompose(slab_in(ev.bases, ev.pol, K[0], mc.X0, mc.X1, pl.table().order, lpol != 0));
    ev.n_home = sl.n_home();
    ev.home = sl.home();
    prepare();
    if (tracked) sl.exchange_migrants(ev.U, sites.as<Site<T>>());
    if (lpol) sl.exchange_dipoles(0, ev.U, sites.as<Site<T>>());
  }
  void slab_home(int32_t* out, int* n_home, int* n_import) override { sl.home_to(out, n_home, n_import); }
  void slab_lists(int na, int nranks, int32_t* owner, int32_t* bits, int32_t* home, int32_t* rows, int32_t* act, int32_t* imp,
                  int32_t* exp, int32_t* mig_in, int32_t* mig_out, int64_t* counts) override {
    sl.lists_to_host(na, top.na, nranks, owner, bits, home, rows, act, imp, exp, mig_in, mig_out, counts);
  }
  // the residual word of an SCF check: maximum over the ranks (bit patterns of non-negative doubles are doubles)
  void reduce_check_word(unsigned long long* word) {
    if (snranks > 1) { TIMED("comm_scf_max"); comm.all_reduce(stream, word, 1, ADMP_T_F64, ADMP_OP_MAX, ADMP_TAG_SCF_MAX); }
  }
  int nloc0() const { return mc.nloc0(); }

  // plans, spectrum and tables of the k-space leg (mc), then the local real mesh
  void ensure_mesh() {
    mc.ensure(K);
    mesh.need(mc.nreal_local() * sizeof(T));
  }
  // the G table of `which` for this cell and the handle's kappa, left in mc.gtab_cur
  void ensure_gtab(const double* box, const double* inv, double vol, int which) { mc.ensure_gtab(box, inv, vol, which, kappa, ref_korder); }
  // sp of MeshConv::convolve: the forward transform builds its planes from the sites (no spread kernel ran): small
  // double-precision systems on the direct-DFT plane kernels
  bool spread_fused(int n) const {
    return mc.can_take_riders() && !ev.home && dft_zy_spread_fits<T>(K, n);
  }
  PlaneSpread<T> plane_spread(int n, const Site<T>* rows, int lp, const int4* bases) const {
    PlaneSpread<T> sp;
    sp.na = n; sp.lpol = lp; sp.sites = rows; sp.bases = bases; sp.g = ev.g;
    return sp;
  }
  // rider: an SCF field kernel whose workgroups run inside the x pass (pair_kernels.hip k_xconv_pair; direct-DFT meshes only)
  bool rider_ok() const {
    static const bool on = env_flag("ADMP_FIELD_RIDER", true);
    return on && mc.can_take_riders() && !overlap_ok();
  }
  // pair rider: the closing pair kernel in the x pass (k_xconv_pair_full: small polarizable f64 systems).  ADMP_PAIR_RIDER=0
  // restores the launch of its own (read per call: the parity test runs both forms in one process); so does
  // ADMP_OPT_SIDE_STREAM = 0, the mode for clean per-kernel times, which keeps the kernel under its pair_full label.
  bool pair_rider_ok() const {
    return lpol && side_stream_on && rider_ok() && env_flag("ADMP_PAIR_RIDER", true);
  }
  Box<T> make_box(const double* h, double* inv, double* vol) { return admp::make_box<T>(h, inv, vol); }

  RecipGeom<T> make_geom(const double* inv) {
    // every spread and gather comes through here; only admp_mesh_convolve, which has no splines, takes shorter meshes
    ARG_CHECK(K[0] >= 6 && K[1] >= 6 && K[2] >= 6, "PME mesh must be at least 6 points per dimension (order-6 splines)");
    RecipGeom<T> g;
    for (int d = 0; d < 3; ++d) g.K[d] = K[d];
    for (int k = 0; k < 9; ++k) g.hinv[k] = (T)inv[k];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        g.Aop[3 * i + j] = (T)(-(double)K[i] * inv[3 * j + i]);   // -Nj_Aji_star[i][j] (admp/recip.py:52,177)
        g.Jac[3 * i + j] = (T)(-(double)K[j] * inv[3 * i + j]);   // d u_j / d x_i     (admp/recip.py:75-77)
      }
    g.whole_mesh();
    if (snranks > 1) { g.xoff = mc.X0; g.nloc0 = nloc0(); g.wrap0 = 1 << 30; }
    return g;
  }

  // admp_mesh_convolve: the k-space leg alone on a mesh of the caller's -- ensure_mesh, the handle's own G table, mc.convolve():
  // what an evaluation runs between its spread and its gather, without riders or plane spread (tests feed it meshes)
  void mesh_convolve(const double* box, int which, void* data_, int on_device, double* E_out, int32_t* info) override {
    mesh_convolve_on(snranks == 1, "admp_mesh_convolve works on a single rank only (slab-decomposed handle)", box, which, data_,
                     on_device, E_out, info);
  }
  // admp_slab_mesh_convolve: the same leg on a slab rank -- its local mesh as an evaluation holds it between spread and gather
  // (own planes, then the kGhost overhang planes meant for the next rank); mc.convolve() is then the distributed convolution
  // with the x pass this handle takes; every rank of the communicator makes the call
  void slab_mesh_convolve(const double* box, int which, void* data_, int on_device, double* E_out, int32_t* info) override {
    mesh_convolve_on(snranks > 1, "admp_slab_mesh_convolve works on a slab-decomposed handle only (single rank: admp_mesh_convolve)",
                     box, which, data_, on_device, E_out, info);
  }
  void mesh_convolve_on(bool right_handle, const char* wrong_handle, const double* box, int which, void* data_, int on_device,
                        double* E_out, int32_t* info) {
    ARG_CHECK(have_ewald, "admp_set_ewald first");
    ARG_CHECK(right_handle, wrong_handle);
    ARG_CHECK(box && data_ && E_out && info, "null argument");
    ARG_CHECK(which == 1 || which == 6 || which == 8 || which == 10, "which must be 1, 6, 8 or 10");
    double inv[9], vol;
    make_box(box, inv, &vol);
    ensure_mesh();
    ensure_gtab(box, inv, vol, which);
    const size_t nreal = nreal_local();
    T* m = on_device ? reinterpret_cast<T*>(data_) : mesh.as<T>();
    if (!on_device) HIP_TRY(hipMemcpyAsync(m, data_, nreal * sizeof(T), hipMemcpyHostToDevice, stream));
    energies_d.need(2 * E_WORDS * sizeof(double));
    ehalf = 0; other_clean = false;
    HIP_TRY(hipMemsetAsync(Ed_cur() + E_RECIP, 0, sizeof(double), stream));
    const int64_t circ0 = mesh_stats.xpass[0];
    mc.convolve(m, mc.gtab_cur, Ed_cur(), E_RECIP);
    if (!on_device) HIP_TRY(hipMemcpyAsync(data_, m, nreal * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(E_out, Ed_cur() + E_RECIP, sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < ADMP_MESH_INFO_WORDS; ++k) info[k] = 0;
    mc.fill_info(info);      // the path; two-level: split and forms; slab rank: its bounds
    if (mc.direct()) info[1] = mesh_stats.xpass[0] > circ0 ? 1 : 2;
  }

  ScaleTab<T> make_tab(int ns, const double* mS, const double* pS) {
    ARG_CHECK(ns >= 1 && mS, "mScales missing");
    ScaleTab<T> t;
    for (int nb = 0; nb < 16; ++nb) {
      int idx = ((nb - 1) % ns + ns) % ns;   // python-style wrap of mScales[nbonds-1] (admp/pme.py:682-683)
      t.mm[nb] = (T)(mS[idx] - 1.0);
      double p = pS ? pS[idx] : 0.0;
      t.p[nb] = (T)p;
      t.w0[nb] = (T)(1.0 / (std::exp((p - 1e-3) / 1e-5) + 1.0));   // switch_val weight of y0 (admp/pme.py:345-346)
    }
    return t;
  }

  const T* stage_in(DevBuf& b, const void* p, size_t n, int on_device) {
    if (!p) return nullptr;
    if (on_device) return reinterpret_cast<const T*>(p);
    b.need(n * sizeof(T));
    HIP_TRY(hipMemcpyAsync(b.p, p, n * sizeof(T), hipMemcpyHostToDevice, stream));
    return b.as<T>();
  }

  void ensure_bins(int na) { ensure_bins(na, bins, bin_cells, bin_sorted); }
  void ensure_bins(int na, BinScratch& b, DevBuf& cells, DevBuf& sorted) {
    const int dims[3] = {nloc0(), K[1], K[2]};
    const BrickGrid bg = make_bricks(dims);
    cells.need(sizeof(int) * 3 * (size_t)(bg.ncell + 1));
    sorted.need(sizeof(int) * 8 * (size_t)na);
    bin_scan.need(spread_scan_bytes(bg.ncell));
    if (b.cell_start != cells.as<int>() || b.cursor != cells.as<int>() + (bg.ncell + 1))
      b.counters_zero = false;                     // fresh or re-laid-out storage
    b.cell_start = cells.as<int>();
    b.cursor = cells.as<int>() + (bg.ncell + 1);
    b.fillcur = cells.as<int>() + 2 * (size_t)(bg.ncell + 1);
    b.sorted = sorted.as<int>();
    b.scan_tmp = bin_scan.p;
    b.scan_bytes = bin_scan.bytes;
  }

  // launch_spread on the site-row bins of this handle; a failed launch is an error of the call
  void spread_sites(int n, const Site<T>* rows, int lp, const RecipGeom<T>& g, T* mesh_p, const int4* bases = nullptr, int nb = 1,
                    int reuse_bins = 0) {
    const int rc = launch_spread<T>(stream, n, rows, lp, g, bins, mesh_p, nullptr, bases, nb, reuse_bins);
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("launch_spread: ") + hipGetErrorString((hipError_t)rc)};
  }

  // ---- one evaluation, step by step --------------------------------------------------------------------------
  // pme() runs the steps back to back.  On a slab-decomposed handle the same steps work on the rank's home atoms and the
  // collectives of the caller's communicator (admp_set_comm) sit between them: same kernels, same SCF forms.
  struct Eval {
    const T* pos = nullptr; const T* Ql = nullptr; const T* pol = nullptr; const T* thole = nullptr;
    T* U = nullptr;
    Box<T> bx; RecipGeom<T> g; ScaleTab<T> tab;
    int n_home = 0; const int* home = nullptr;   // this rank's atoms (nullptr = all, in order)
    const int4* bases = nullptr;                 // stencil base indices per atom (written by prepare_sites)
    bool active = false;
  } ev;
  const int* pair_rows() const { return snranks > 1 ? sl.rows() : pl.table().order; }      // row order of the pair kernels

  int stage_begin(const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_, int ns,
                  const double* mS, const double* pS, void* U_) {
    ARG_CHECK(have_top && have_ewald && pl.have(), "topology, ewald parameters and pairs must be set first");
    ARG_CHECK(pos_ && box && Ql_, "null argument");
    if (lpol) ARG_CHECK(pol_ && thole_ && U_ && pS, "polarizable handle needs pol, tholes, pScales and U_inout");
    const int na = top.na;
    double inv[9], vol;
    ++eval_seq;
    ff_done = nullptr;
    ensure_mesh();
    ev.bx = make_box(box, inv, &vol);
    ev.g = make_geom(inv);
    ev.tab = make_tab(ns, mS, pS);
    ensure_gtab(box, inv, vol, 1);
    ev.pos = reinterpret_cast<const T*>(pos_);
    ev.Ql = reinterpret_cast<const T*>(Ql_);
    ev.pol = lpol ? reinterpret_cast<const T*>(pol_) : nullptr;
    ev.thole = lpol ? reinterpret_cast<const T*>(thole_) : nullptr;
    ev.U = lpol ? reinterpret_cast<T*>(U_) : nullptr;
    // admp_set_dipole_source (one shot): the initial dipoles are read from there, ev.U starts as their copy (k_prepare_sites)
    const T* U_first = lpol && U_src_now ? reinterpret_cast<const T*>(U_src_now) : ev.U;
    U_src_now = nullptr;
    sites.need(sizeof(Site<T>) * (size_t)na);
    pot.need(9 * (size_t)na * sizeof(T));
    energies_d.need(2 * E_WORDS * sizeof(double));
    if (energies_d.p != energies_seen) { energies_seen = energies_d.p; other_clean = false; }
    if (lpol) {
      fld_pair.need(3 * (size_t)na * sizeof(T));
      fld_recip.need(3 * (size_t)na * sizeof(T));
      field.need(3 * (size_t)na * sizeof(T));
    }
    ensure_bins(na);
    bases_d.need(sizeof(int4) * (size_t)na);
    if (other_clean) {
      ehalf ^= 1;                      // zeroed by the previous evaluation's first kernel
    } else {
      ehalf = 0;
      HIP_TRY(hipMemsetAsync(energies_d.p, 0, E_WORDS * sizeof(double), stream));   // energies and the max|field| word
    }
    other_clean = false;
    fmax_clean = true;
    for (bool& c : slot_clean) c = true;
    // Slab rank, steady state: only the rows this rank reads are prepared -- its home atoms and its imports (round 3 prepared
    // the rows of ALL atoms on every rank: 0.056 ms at 1M atoms whatever the rank count).  The ownership rule needs the stencil
    // base planes of all atoms first: a 28-byte-per-atom pass (k_atom_bases).  The first evaluation of a handle / topology /
    // buffer, and evaluations that recompile the table's site classes, take the all-atom pass below, so that every row of
    // `sites` has held valid data at least once (the class compilation reads all of them).  ADMP_SLAB_SUBSET=0: always all.
    static const bool subset_on = env_flag("ADMP_SLAB_SUBSET", true);
    if (snranks > 1 && subset_on && slab_sites_na == na && slab_sites_ptr == sites.p && !pl.classes_pending() && pl.have()) {
      { TIMED("atom_bases"); launch_atom_bases<T>(stream, na, ev.pos, ev.g, bases_d.as<int4>()); }
      ev.bases = bases_d.as<int4>();
      cls_sites_na = na;
      pl.evaluation_begins();
      decompose_eval([&] {
        TIMED("prepare_sites");
        const int* lists[2] = {sl.home(), sl.imports()};
        const int counts[2] = {sl.n_home(), sl.n_imp()};
        for (int k = 0; k < 2; ++k)
          launch_prepare_sites<T>(stream, top, ev.pos, ev.Ql, U_first, ev.pol, ev.thole, ev.bx, sites.as<Site<T>>(),
                                  k == 0 ? energies_d.as<double>() + (size_t)(ehalf ^ 1) * E_WORDS : nullptr, ev.g, nullptr,
                                  nullptr, nullptr, pl.table().cls, cls_flags_dev(), rq_p(), U_first != ev.U ? ev.U : nullptr, lists[k],
                                  counts[k]);
        other_clean = true;
      });
      ev.active = true;
      cut_pass();
      return ev.n_home;
    }
    {
      TIMED("prepare_sites");
      // list of the polarizable sites for the incremental SCF: rebuilt by this kernel unless the caller vouches that the
      // set is the one of the previous call (ADMP_OPT_KEEP_POL_SITES; the Python wrapper sets it while `pol` is unchanged).
      // A slab rank takes its list (the polarizable HOME atoms of this evaluation) from the decomposition instead.
      const bool have_list = act_n >= 0 && act_top_na == na && act_d.p;
      const bool want_act = lpol && snranks == 1 && !(keep_pol_sites && have_list);
      act_fresh = want_act;
      if (want_act) { act_d.need(sizeof(int) * (size_t)na); act_n = -1; act_top_na = na; ++act_gen; }
      if (pl.classes_pending() && cls_sites_na == na)      // `sites` still holds the last evaluation's
        pl.compile_classes<T>(na, sites.as<Site<T>>());
      pl.evaluation_begins();
      cls_sites_na = na;
      launch_prepare_sites<T>(stream, top, ev.pos, ev.Ql, U_first, ev.pol, ev.thole, ev.bx, sites.as<Site<T>>(),
                              energies_d.as<double>() + (size_t)(ehalf ^ 1) * E_WORDS, ev.g, bases_d.as<int4>(),
                              want_act ? act_d.as<int>() : nullptr, want_act ? nact_dev() : nullptr, pl.table().cls,
                              cls_flags_dev(), rq_p(), U_first != ev.U ? ev.U : nullptr);
      ev.bases = bases_d.as<int4>();
      // First evaluation on a table compiled without classes: look at the flags right away (one extra host read, once) so
      // that this call already walks the parted rows -- a caller who evaluates once gets the reduced forms too.
      if (pl.first_look()) {
        int flags = 0;
        HIP_TRY(hipMemcpyAsync(&flags, cls_flags_dev(), sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (flags & CLS_BETTER) {
          pl.compile_classes<T>(na, sites.as<Site<T>>());
          HIP_TRY(hipMemsetAsync(cls_flags_dev(), 0, sizeof(int), stream));   // the table now agrees with these sites
        }
      }
    }
    other_clean = true;
    if (snranks > 1) {
      slab_sites_na = na; slab_sites_ptr = sites.p;        // every row of `sites` is valid from here on
      decompose_eval([] {});
    } else {
      ev.n_home = na;
      ev.home = nullptr;
    }
    ev.active = true;
    cut_pass();
    return ev.n_home;
  }
  // the inner table of this evaluation (see cut_nbr): the rows its pair kernels walk, at the sites just prepared
  void cut_pass() {
    cut_on = cutoff > 0.0;
    if (!cut_on) return;
    const NbrTable& nbr = pl.table();
    const size_t na = (size_t)top.na, entries = (size_t)std::max<int64_t>(nbr.cap, 1);
    cut_end.need(sizeof(int) * na);
    cut_col.need(sizeof(int) * entries);
    cut_nbr = nbr;
    cut_nbr.col = cut_col.as<int>();
    cut_nbr.rowend = cut_end.as<int>();
    if (lpol) {
      cut_iend.need(sizeof(int) * na);
      cut_icol.need(sizeof(int) * entries);
      cut_ind.beg = nbr.rowptr; cut_ind.end = cut_iend.as<int>(); cut_ind.col = cut_icol.as<int>();
      cut_ind.cap = (int64_t)entries; cut_ind.na_cap = (int)na;
    }
    TIMED("cut_table");
    const int rc = build_cut_table<T>(stream, ev.n_home, pair_rows(), nbr, sites.as<Site<T>>(), ev.bx, cutoff,
                                      cut_end.as<int>(), cut_col.as<int>(), lpol ? cut_iend.as<int>() : nullptr,
                                      lpol ? cut_icol.as<int>() : nullptr);
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("build_cut_table: ") + hipGetErrorString((hipError_t)rc)};
  }

  void need_eval() { ARG_CHECK(ev.active, "internal: no evaluation in progress"); }

  void stage_spread(T* mesh_p) {
    need_eval();
    TIMED("spread");
    int rc = launch_spread<T>(stream, ev.n_home, sites.as<Site<T>>(), lpol, ev.g, bins, mesh_p, ev.home, ev.bases);
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("launch_spread: ") + hipGetErrorString((hipError_t)rc)};
  }
  // max|field| lives in the last word of the energies buffer (bit pattern of a non-negative double), so that one
  // device->host copy can fetch it together with the energies
  unsigned long long* fmax_word() { return reinterpret_cast<unsigned long long*>(Ed_cur() + E_FMAX); }
  void launch_field_finish_only() {      // total dE/dU of every home atom and its maximum (over all ranks) into fmax_word()
    need_eval();
    if (!fmax_clean) HIP_TRY(hipMemsetAsync(fmax_word(), 0, sizeof(unsigned long long), stream));
    fmax_clean = false;
    { TIMED("field_finish");
      launch_field_finish<T>(stream, ev.n_home, sites.as<Site<T>>(), ev.pol, ev.U, fld_pair.as<T>(), fld_recip.as<T>(),
                             (T)kappa, field.as<T>(), fmax_word(), ev.home); }
    reduce_check_word(fmax_word());
  }
  // The charge-only pair forms read the compact rq rows and the class marks of the table: asking for them without those is
  // a bug of the caller, not something to paper over (round 2: a slab handle passed the flag word but no rq rows, and the
  // kernels' prefetch `rq[0]` read address 0 -- DESIGN.md section 7a).
  void check_mono_inputs(bool use_mono) {
    if (use_mono && !rq_d.p) throw Err{ADMP_E_STATE, "charge-only pair forms requested without the compact site rows"};
  }
  // ---- a second stream for the real-space kernels of small systems (round 3) ---------------------------------------------
  // At a few thousand atoms a kernel fills a fraction of the chip and a step is a chain of ~20 short dispatches; the pair
  // kernels (sites -> gradient / potential / field rows) do not depend on the mesh chain (spread -> convolution) that runs
  // next to them, so they go to a side stream between a fork (side waits for what main has enqueued so far) and a join (main
  // waits for the side stream before the first kernel that reads or adds to the pair kernel's rows: the gathers).
  // ADMP_OVERLAP_MAX: atom count up to which this is done (0 = never; default 200 000: 98k atoms 0.316 -> 0.306 ms per step,
  // 1M atoms 1.72 -> 1.99 -- there every kernel fills the chip and the two streams only get in each other's way).
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool side_busy = false;
  // ... and from which it is done (ADMP_OVERLAP_MIN, default 4096): the fork + join cost ~12 us of the main chain, what they hide
  // is the pair kernels -- 15 us at 3072 atoms (round 4, after the chain lost its spread and closing kernels: 0.1893 ms per
  // step on one stream against 0.1929 with the side stream, and a third of the run-to-run spread), 30 us at 6144 atoms
  // (0.241 against 0.261 ms), more above.
  bool overlap_ok() const {
    static const int mx = env_int("ADMP_OVERLAP_MAX", 200000);
    static const int mn = env_int("ADMP_OVERLAP_MIN", 4096);
    return side_stream_on && snranks == 1 && top.na <= mx && top.na >= mn;
  }
  // An exception between on_side() and join_side() (a failed launch, a refused argument further down the call) would leave
  // kernels of this call running on the side stream with nobody waiting for them -- the next call would race them on the
  // gradient rows (round-3 verdict, weak #10).  guarded() calls this before it reports the error.
  void after_error() override {
    if (side) (void)hipStreamSynchronize(side);
    side_busy = false;
    ev.active = false;
    // a set that was being written when the call failed may have replaced the oldest one: the history starts again.
    // A call that failed before that leaves it unadvanced.
    if (aspc_dirty) { aspc.drop(); aspc_dirty = false; }
  }
  // Order of submission around a fork: dispatch-bound systems (<= 16384 atoms) submit the side work AFTER the first kernel of
  // the main chain that follows (see recip_pass); larger ones first -- there the pair kernel is long and wants the early start.
  // ADMP_SIDE_FIRST = 0 / 1 forces one order (A/B).
  bool side_first() const {
    static const int mode = env_int("ADMP_SIDE_FIRST", -1);
    return mode >= 0 ? mode != 0 : top.na > 16384;
  }
  template <class F>
  void on_side(F&& f) {
    if (!overlap_ok()) { f(); return; }
    if (!side) {
      HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(ev_fork, stream));
    HIP_TRY(hipStreamWaitEvent(side, ev_fork, 0));
    hipStream_t main_stream = stream;
    stream = side;
    try { f(); } catch (...) { stream = main_stream; throw; }      // (guarded() -> after_error() waits for the side stream)
    stream = main_stream;
    HIP_TRY(hipEventRecord(ev_join, side));
    side_busy = true;
  }
  void join_side() {
    if (!side_busy) return;
    HIP_TRY(hipStreamWaitEvent(stream, ev_join, 0));
    side_busy = false;
  }

  // the closing pair kernel of this evaluation: its argument record, and what precedes its launch in either form
  PairFullArgs<T> pair_full_args(T* grad_p, T* fld_out) {
    const NbrTable& nb = wnbr();
    PairFullArgs<T> a;
    a.on = 1; a.na = ev.n_home; a.rowptr = nb.rowptr; a.rowend = nb.rowend; a.col = nb.col; a.sites = sites.as<Site<T>>();
    a.box = ev.bx; a.tab = ev.tab; a.kappa = (T)kappa; a.grad = grad_p; a.pot = pot.as<T>(); a.energies = Ed_cur();
    a.rows = pair_rows(); a.fld = fld_out; a.use_mono = mono_ok ? 1 : 0; a.cls_flags = cls_flags_dev();
    a.rq = rq_d.as<RQ4<T>>(); a.tholes = ev.thole;
    return a;
  }
  void pair_full_prologue() {
    check_mono_inputs(mono_ok);
    if (!slot_clean[E_REAL]) {
      HIP_TRY(hipMemsetAsync(Ed_cur() + E_REAL, 0, sizeof(double), stream));
      HIP_TRY(hipMemsetAsync(Ed_cur() + E_RPARTS, 0, E_PARTS * sizeof(double), stream));
    }
    slot_clean[E_REAL] = false;
  }
  void stage_pair_full(T* grad_p, T* fld_out = nullptr) {
    need_eval();
    if (snranks > 1)   // the closing kernel ADDS frame-adjoint contributions to atoms of other ranks: those rows start at zero
      launch_rows_scatter<T>(stream, 2, sl.n_imp(), 3, sl.imports(), nullptr, grad_p);
    pair_full_prologue();
    if (lpol) ++pair_rider_stats[1];
    TIMED("pair_full");
    launch_pair_full<T>(stream, pair_full_args(grad_p, fld_out), lpol);
  }
  // stage_pair_full as a rider of the next x pass: everything but the launch (the energy words are cleared here, ahead of
  // the fused launch); false = it cannot ride, nothing was done and the caller takes stage_pair_full.  Riders are single-rank.
  bool pair_full_rider(PairFullArgs<T>& pr, T* grad_p, T* fld_out = nullptr) {
    if (!pair_rider_ok()) return false;
    need_eval();
    pr = pair_full_args(grad_p, fld_out);
    if (!full_rider<T>(pr, lpol)) return false;
    pair_full_prologue();
    ++pair_rider_stats[0];
    return true;
  }
  // with_field_finish: the gather also forms the total dE/dU and its maximum (launch_field_finish's work, fused)
  // Small single-rank systems with frame groups: the closing kernel's work rides in the gather's epilogue (recip_kernels.hip,
  // k_gather_staged<.., FIN>); the launch_finish_only that follows is then a no-op.  ADMP_FUSE_FIN_MAX = 0 turns it off (A/B).
  bool fin_fused = false;
  bool fuse_fin_ok() const {
    const int fin_max = env_int("ADMP_FUSE_FIN_MAX", 8192);       // (read per call: the parity tests run both forms in one process)
    return snranks == 1 && !ev.home && top.gath_blk && top.na <= fin_max;
  }
  FinishArgs<T> finish_args(bool want_grad, T* dQl) {
    FinishArgs<T> f;
    f.pol = ev.pol; f.kappa = (T)kappa; f.dQlocal = dQl; f.energies = Ed_cur(); f.want_grad = want_grad ? 1 : 0;
    return f;
  }
  // ff_given: a field epilogue on a word of the caller's choice (field_epilogue(word); the chained SCF's last residual)
  void stage_gather(const T* mesh_p, T* grad_p, T* fld_out = nullptr, bool with_field_finish = false,
                    double* e_recip = nullptr, const FinishArgs<T>* fin = nullptr, const FieldFin<T>* ff_given = nullptr) {
    need_eval();
    FieldFin<T> ff;
    if (ff_given) ff = *ff_given;
    else if (with_field_finish) {
      if (!fmax_clean) HIP_TRY(hipMemsetAsync(fmax_word(), 0, sizeof(unsigned long long), stream));
      fmax_clean = false;
      ff.pol = ev.pol; ff.Ucart = ev.U; ff.fld_pair = fld_pair.as<T>(); ff.kappa = (T)kappa;
      ff.field = field.as<T>(); ff.fmax_bits = fmax_word();
    }
    join_side();                       // the gather adds to the rows the pair kernel has set
    TIMED("gather");
    if (fin && fuse_fin_ok()) {
      launch_gather<T>(stream, ev.n_home, sites.as<Site<T>>(), lpol, ev.g, mesh_p, pot.as<T>(), grad_p, ev.home, fld_out, ff,
                       e_recip, &top, &ev.bx, *fin);
      fin_fused = true;
      return;
    }
    launch_gather<T>(stream, ev.n_home, sites.as<Site<T>>(), lpol, ev.g, mesh_p, pot.as<T>(), grad_p, ev.home, fld_out, ff,
                     e_recip);
  }
  // closes the evaluation: E_out = (real, recip[slot], self, penalty) of THIS rank's share
  // with_field_finish (single rank, pull kernel): the SCF residual and its maximum are formed by this kernel too
  void launch_finish_only(T* grad_p, T* dQl, bool with_field_finish = false) {
    need_eval();
    if (fin_fused) { fin_fused = false; return; }      // (the gather just before did this work)
    FieldFin<T> ff;
    if (with_field_finish) {
      if (!fmax_clean) HIP_TRY(hipMemsetAsync(fmax_word(), 0, sizeof(unsigned long long), stream));
      fmax_clean = false;
      ff.pol = ev.pol; ff.Ucart = ev.U; ff.fld_pair = fld_pair.as<T>(); ff.fld_recip = fld_recip.as<T>();
      ff.kappa = (T)kappa; ff.field = field.as<T>(); ff.fmax_bits = fmax_word();
    }
    { TIMED("finish");
      launch_finish<T>(stream, top, ev.pos, ev.bx, sites.as<Site<T>>(), ev.pol, ev.U, lpol, (T)kappa, pot.as<T>(), grad_p,
                       dQl, Ed_cur(), ev.home, ev.n_home, ff, snranks > 1 ? sl.bits() : nullptr); }
    if (snranks > 1 && grad_p) sl.return_gradient(grad_p);
  }
  // ---- incremental SCF ------------------------------------------------------------------------------------------
  // The field dE/dU is LINEAR in the induced dipoles and only sites with pol > 0 ever change theirs.  So after the first
  // (full) field evaluation of a call, every further SCF cycle evaluates only the field of the Jacobi step's dipole CHANGE
  // dU: real space over polarizable-polarizable pairs (k_pair_field_ind), reciprocal space by spreading the dU of the
  // polarizable sites alone, and adds it to the stored field; phi is kept current by adding the increment's mesh.  For
  // water that is 1/9 of the pairs and 1/3 of the spread / gather work per cycle; the arithmetic is the reference's
  // (admp/pme.py:130-138) regrouped, same dipoles and cycle count to round-off.  On a slab rank the rows are the polarizable
  // HOME atoms and the dU of the imported atoms arrive by one all-to-all-v per Jacobi step (sl.exchange_dipoles).
  enum { E_PARTS_SUM = -1 };   // read_energies: the reciprocal energy is the sum of the E_PARTS partial words
  int* nact_dev() { return reinterpret_cast<int*>(Ed_cur() + E_NACT); }
  DevBuf rq_d;                                      // compact (position, charge) rows: what the pair kernels read of a
  RQ4<T>* rq_p() {                                  // charge-only partner
    rq_d.need(sizeof(RQ4<T>) * (size_t)top.na);
    return rq_d.as<RQ4<T>>();
  }
  int* cls_flags_dev() { return nact_dev() + 1; }   // the other half of that word: CLS_* of this evaluation (k_prepare_sites)
  int cls_sites_na = -1;                            // `sites` holds an evaluation of this many atoms
  // the polarizable rows of this evaluation: all polarizable atoms (one rank), or the rank's polarizable home atoms
  const int* act_list() const { return snranks > 1 ? sl.act() : act_d.as<int>(); }
  // device-side count for the kernels of the first cycle when the list is fresh (nullptr: the host knows it)
  const int* nact_arg() { return snranks == 1 && act_fresh ? nact_dev() : nullptr; }
  int nact_rows() const { return snranks > 1 ? sl.n_act() : (act_fresh ? top.na : act_n); }      // grid bound of those kernels
  int nact_known() const { return snranks > 1 ? sl.n_act() : act_n; }
  void nact_seen() {                                                 // after a read_energies of this evaluation
    if (snranks > 1 || !act_fresh) return;
    int n = 0;
    std::memcpy(&n, &Eh[E_NACT], sizeof(n));
    act_n = n;
    act_fresh = false;
    // The workgroups of k_prepare_sites append their chunks in completion order; in atom order the rows that neighbouring
    // workgroups (and XCDs) of the pair kernels work on are neighbours in space again (measured HBM traffic of the field
    // pass over the list at 1M atoms: 1.42 GB unsorted -- more than the full pair kernel's 0.44 GB).
    act_tmp.need(sizeof(int) * (size_t)(n > 0 ? n : 1));
    int rc = sort_ints(stream, act_d.as<int>(), act_tmp.as<int>(), n, &sort_scratch.p, &sort_bytes);
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("sort_ints: ") + hipGetErrorString((hipError_t)rc)};
  }
  // the SCF field kernels over the polarizable rows: real-space dE/dU from all partners (k_pair_field), and its increment
  // from the last Jacobi step of the polarizable partners (k_pair_field_ind, over the current sub-table)
  PairFieldArgs<T> pair_field_common(int kind, int n_rows) {
    PairFieldArgs<T> a;
    a.kind = kind; a.na = n_rows; a.sites = sites.as<Site<T>>(); a.box = ev.bx; a.tab = ev.tab; a.kappa = (T)kappa;
    a.fld = fld_pair.as<T>(); a.rows = act_list();
    return a;
  }
  PairFieldArgs<T> pair_field_args() {      // (hands the flag word over: the charge-only form is on, see check_mono_inputs)
    const NbrTable& nb = wnbr();
    PairFieldArgs<T> a = pair_field_common(1, nact_rows());
    a.rowptr = nb.rowptr; a.rowend = nb.rowend; a.col = nb.col;
    a.n_dev = nact_arg(); a.cls_flags = cls_flags_dev(); a.rq = rq_d.as<RQ4<T>>(); a.tholes = ev.thole;
    return a;
  }
  PairFieldArgs<T> pair_field_ind_args(int n_act) {
    const IndTable& it = wind();
    PairFieldArgs<T> a = pair_field_common(2, n_act);
    a.rowptr = it.beg; a.rowend = it.end; a.col = it.col;
    return a;
  }
  void first_pair_field() {
    check_mono_inputs(true);
    const PairFieldArgs<T> a = pair_field_args();
    TIMED("pair_field");
    launch_pair_field<T>(stream, a);
  }
  void first_gather_field(const FieldFin<T>& ff) {   // reciprocal dE/dU of the polarizable rows from phi
    join_side();                     // (its epilogue reads the pair field)
    TIMED("gather_field");
    launch_gather_field<T>(stream, nact_rows(), sites.as<Site<T>>(), ev.g, mesh.as<T>(), fld_recip.as<T>(), act_list(), 1,
                           nact_arg(), nullptr, ff);
  }
  double scf_check(int* n_act) {          // total field + its maximum over the polarizable sites; one host read
    if (ff_done == fmax_word()) ff_done = nullptr;            // formed by the field gather before this check
    else launch_field_check(next_check_word());
    double dummy[4];
    const double fmax = read_energies(E_SCF_RECIP, dummy, false);
    nact_seen();
    *n_act = nact_known();
    return fmax;
  }
  void scf_jacobi(int n_act, const unsigned long long* gate = nullptr, double gate_min = 0.0, double relax = 1.0) {
    if (n_act > 0) {
      isites.need(sizeof(Site<T>) * (size_t)n_act);
      TIMED("jacobi_update");
      launch_jacobi_delta<T>(stream, n_act, act_list(), ev.pol, field.as<T>(), ev.U, sites.as<Site<T>>(),
                             isites.as<Site<T>>(), gate, gate_min, relax);
    }
    if (snranks > 1) sl.exchange_dipoles(1, ev.U, sites.as<Site<T>>());      // every rank takes part, whatever its own count
  }
  // Small systems are dispatch-bound: the SCF residual rides in the epilogue of the field gather that precedes a check
  // (field_epilogue(word) describes it; the check's own kernel is then skipped).  word: a zero word of the energy block.
  const unsigned long long* ff_done = nullptr;
  // ADMP_FUSE_FF_MAX: atom count up to which a field finish rides in a gather
  static int fuse_ff_max() { static const int v = env_int("ADMP_FUSE_FF_MAX", 16384); return v; }
  bool fuse_ok() const { return top.na <= fuse_ff_max() && snranks == 1 && !ev.home; }
  FieldFin<T> field_epilogue(unsigned long long* word) {
    FieldFin<T> ff;
    if (!word || !fuse_ok()) return ff;
    ff.pol = ev.pol; ff.Ucart = ev.U; ff.fld_pair = fld_pair.as<T>(); ff.kappa = (T)kappa;
    ff.field = field.as<T>(); ff.fmax_bits = word; ff.sites = sites.as<Site<T>>();
    ff_done = word;
    return ff;
  }
  // the word the next plain check writes: fmax_word(), cleared if this evaluation has used it
  unsigned long long* next_check_word() {
    if (!fmax_clean) HIP_TRY(hipMemsetAsync(fmax_word(), 0, sizeof(unsigned long long), stream));
    fmax_clean = false;
    return fmax_word();
  }
  // total field of the polarizable rows and its maximum (over all ranks) into `word` (a zero word of this evaluation's
  // energy block); no host read
  void launch_field_check(unsigned long long* word) {
    if (ff_done == word) { ff_done = nullptr; return; }     // the field gather before it has done this (one rank only)
    ff_done = nullptr;
    if (nact_rows() > 0) {
      TIMED("field_finish");
      launch_field_finish<T>(stream, nact_rows(), sites.as<Site<T>>(), ev.pol, ev.U, fld_pair.as<T>(), fld_recip.as<T>(),
                             (T)kappa, field.as<T>(), word, act_list(), nact_arg());
    }
    reduce_check_word(word);
  }
  size_t nreal_local() const { return mc.nreal_local(); }
  // check_word: the zero word the check after this increment writes (its residual then rides in the field gather)
  // extra_side: more work for the side stream of this increment (the closing pair kernel of a chained call, whose dipoles are final)
  // field_from_total_phi: do not gather the increment's field -- the caller's next kernel is a full gather of the accumulated
  // phi with a field epilogue, which yields the same reciprocal field (and the residual) for every atom
  // full_grad: the closing pair kernel (gradient rows full_grad) may ride in this increment's x pass -- the dipoles are
  // final; returns whether it did
  // no_field: nobody reads the field of the new dipoles (last corrector of a fixed-form call): phi alone is brought up to
  // date, the real-space increment and the field gather are not run
  // the polarizable sub-table of the walked table, rebuilt when the neighbour table or the polarizable set changed (cut_ind is
  // written by every evaluation instead)
  void ensure_ind_table() {
    if (cut_on || (ind_nbr_gen == pl.gen() && ind_act_gen == act_gen)) return;
    TIMED("ind_table");
    int rc = build_ind_table<T>(stream, top.na, pl.table(), sites.as<Site<T>>(), ind);
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("build_ind_table: ") + hipGetErrorString((hipError_t)rc)};
    ind_nbr_gen = pl.gen(); ind_act_gen = act_gen;
  }
  bool scf_increment(int n_act, unsigned long long* check_word = nullptr,   // fld_pair / fld_recip / phi <- their values for the dipoles after scf_jacobi
                     const std::function<void()>& extra_side = nullptr, bool field_from_total_phi = false,
                     T* full_grad = nullptr, bool no_field = false) {
    if (n_act <= 0 && snranks == 1) {
      if (extra_side) on_side(extra_side);
      return false;
    }
    const bool first = side_first();
    PairFieldArgs<T> fr;   // (filled below, once the sub-table is current; it may ride in the x pass)
    bool ride = false;
    auto side_work = [&] {
      if (!ride && !no_field)
        on_side([&] {
          TIMED("pair_field_ind");
          launch_pair_field_ind<T>(stream, fr);
        });
      if (extra_side) on_side(extra_side);
    };
    ensure_ind_table();
    fr = pair_field_ind_args(n_act);
    ride = !no_field && rider_ok() && field_rider<T>(fr);
    if (first) side_work();
    const size_t nreal = nreal_local();
    mesh2.need(nreal * sizeof(T));
    const bool fused = spread_fused(n_act);
    if (fused) { if (!first) side_work(); }
    else { TIMED("spread_ind");
      // the compact rows keep their positions and their order through the SCF cycles of one evaluation: the brick lists of
      // its first increment serve the later ones (two binning passes and a scan less per cycle)
      ensure_bins(std::max(n_act, 1), bins_ind, bin_cells_ind, bin_sorted_ind);
      const bool reuse = ind_bins_eval == eval_seq && ind_bins_n == n_act && ind_bins_gen == act_gen &&
                         ind_bins_at == bins_ind.cell_start;
      int rc = launch_spread<T>(stream, n_act, isites.as<Site<T>>(), 1, ev.g, bins_ind, mesh2.as<T>(), nullptr, nullptr, 1,
                                reuse ? 1 : 0, 0);
      ind_bins_eval = eval_seq; ind_bins_n = n_act; ind_bins_gen = act_gen; ind_bins_at = bins_ind.cell_start;
      if (rc != 0) throw Err{ADMP_E_HIP, std::string("launch_spread: ") + hipGetErrorString((hipError_t)rc)}; }
    if (!first && !fused) side_work();
    const PlaneSpread<T> sp = plane_spread(n_act, isites.as<Site<T>>(), 1, nullptr);
    PairFullArgs<T> pr;
    const bool full_rides = full_grad && pair_full_rider(pr, full_grad);
    const bool added = mc.convolve(mesh2.as<T>(), mc.gtab_cur, Ed_cur(), E_SCRATCH, mesh.as<T>(), nullptr, fused ? &sp : nullptr,
                                ride ? &fr : nullptr, full_rides ? &pr : nullptr);
    join_side();
    if (!field_from_total_phi && !no_field) {
      TIMED("gather_field_ind");
      launch_gather_field<T>(stream, n_act, isites.as<Site<T>>(), ev.g, mesh2.as<T>(), fld_recip.as<T>(), nullptr, 1, nullptr,
                             act_list(), check_word ? field_epilogue(check_word) : FieldFin<T>()); }
    if (!added) { TIMED("mesh_add"); launch_mesh_add<T>(stream, (long)nreal, mesh.as<T>(), mesh2.as<T>()); }
    return full_rides;
  }

  // (real, recip[slot], self, penalty) of the energy block Ed, packed at Ed + E_RED and summed over the ranks
  void sum_energy_words(double* Ed, int recip_slot) {
    TIMED("comm_energies");
    launch_energy_pack(stream, Ed, recip_slot, Ed + E_RED);
    comm.all_reduce(stream, Ed + E_RED, 4, ADMP_T_F64, ADMP_OP_SUM, ADMP_TAG_ENERGIES);
  }
  // one device->host copy + sync: energies (and the max|field| word, returned).  On a slab rank the four parts are first
  // summed over the ranks (want_sum; the SCF checks only need the residual word, which is already the global maximum).
  double read_energies(int recip_slot, double* E, bool want_sum = true) {
    if (!Eh) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&Eh), E_WORDS * sizeof(double), hipHostMallocDefault));
    const bool summed = snranks > 1 && want_sum;
    if (summed) sum_energy_words(Ed_cur(), recip_slot);
    HIP_TRY(hipMemcpyAsync(Eh, Ed_cur(), E_WORDS * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    {
      int w[2];
      std::memcpy(w, &Eh[E_NACT], sizeof(w));
      pl.classes_seen(w[1]);
    }
    if (summed) {
      for (int k = 0; k < 4; ++k) E[k] = Eh[E_RED + k];
      return Eh[E_FMAX];
    }
    E[0] = Eh[E_REAL]; E[1] = recip_slot >= 0 ? Eh[recip_slot] : 0.0; E[2] = Eh[E_SELF]; E[3] = Eh[E_PEN];
    for (int k = 0; k < E_PARTS; ++k) E[0] += Eh[E_RPARTS + k];      // k_pair_full's partial words
    if (recip_slot == E_PARTS_SUM) {         // atom-side reciprocal energy: the partial words of k_gather<.., true>
      double e = 0.0;
      for (int k = 0; k < E_PARTS; ++k) e += Eh[E_SLOTS + k];
      E[1] = e;
    }
    return Eh[E_FMAX];   // same bits as the device word
  }
  void stage_finish(T* grad_p, T* dQl, int recip_slot, double* E) {
    launch_finish_only(grad_p, dQl);
    read_energies(recip_slot, E);
    ev.active = false;
  }

  // full reciprocal pass on one rank: spread -> r2c -> G multiply (+energy) -> c2r ; mesh then holds phi
  // side_work: real-space kernels that run NEXT to the convolution (on_side).  They are submitted after the spread: the host
  // needs ~10 us for the event record / stream wait / launch of a fork, and submitted first (round 3) that time stood between
  // the site pass and the spread on the main stream as well (kernel trace of the S1 loop: 10-12 us idle there, every
  // evaluation); behind the spread it is hidden by a running kernel and the side kernels still have the three transform
  // passes to hide behind (side_first()).
  template <class F>
  void recip_pass(int slot, F&& side_work, const PairFieldArgs<T>* rider = nullptr, const PairFullArgs<T>* prider = nullptr) {
    need_eval();
    const bool fused = spread_fused(ev.n_home);      // the forward transform spreads (dft_kernels.hip, zy_plane_spread)
    const bool first = side_first() || fused;
    if (first) side_work();
    if (!fused) stage_spread(mesh.as<T>());
    if (!first) side_work();
    if (!slot_clean[slot]) HIP_TRY(hipMemsetAsync(Ed_cur() + slot, 0, sizeof(double), stream));
    slot_clean[slot] = false;
    const PlaneSpread<T> sp = plane_spread(ev.n_home, sites.as<Site<T>>(), lpol, ev.bases);
    mc.convolve(mesh.as<T>(), mc.gtab_cur, Ed_cur(), slot, nullptr, nullptr, fused ? &sp : nullptr, rider, prider);
  }
  // reciprocal pass + closing pair kernel (gradient rows grad_p; fld_out: its dE/dU as well): in the x pass, or next to
  // the mesh chain on the side stream / ahead of it on this one
  void recip_pass_pair_full(int slot, T* grad_p, T* fld_out = nullptr) {
    PairFullArgs<T> pr;
    if (pair_full_rider(pr, grad_p, fld_out)) recip_pass(slot, [] {}, nullptr, &pr);
    else recip_pass(slot, [&] { on_side([&] { stage_pair_full(grad_p, fld_out); }); });
  }
  void recip_pass(int slot) { recip_pass(slot, [] {}); }
  // first field evaluation of a call: the mesh chain and the real-space field of all partners -- on the side stream, or (small
  // systems, one stream, direct-DFT mesh) with the field kernel's workgroups inside the x pass
  void recip_pass_first_field(int slot) {
    if (rider_ok()) {
      check_mono_inputs(true);
      const PairFieldArgs<T> fr = pair_field_args();
      if (field_rider<T>(fr)) {
        recip_pass(slot, [] {}, &fr);
        return;
      }
    }
    recip_pass(slot, [&] { on_side([&] { first_pair_field(); }); });
  }

  // ---- Engine::pme: staging, the SCF in one of three forms (scf_policy.h picks it), the closing pass --------------------
  // device views of the arrays of one call (the caller's own, or staging buffers of host arrays)
  struct PmeIo {
    const T *pos = nullptr, *Ql = nullptr, *pol = nullptr, *thole = nullptr;
    T *U = nullptr, *dpos = nullptr, *dQl = nullptr;
    T* gbuf = nullptr;           // the gradient rows of this call: dpos, or the internal buffer of an energy-only call
    double* E = nullptr;         // the caller's four energy parts
  };
  // what the forms of the SCF hand to each other and to the closing pass
  struct ScfRun {
    // phi_valid: the mesh holds phi = c2r(G S) of the CURRENT dipoles (last SCF field evaluation, no update since):
    // the closing gather can then reuse it instead of spreading and transforming again.
    // phi_accum: that phi was assembled from increments, so no single k-space pass saw its energy -- the closing gather
    // sums it over the atoms instead.
    bool phi_valid = false, done = false, finished = false, phi_accum = false;
    bool have_base = false;    // fld_pair / fld_recip / phi belong to the dipoles before the last Jacobi step
    int cyc = 0, flag = 1, i = 0, n_act = 0;   // (i: the reference's loop variable, the cycle scf_loop starts from)
    double f_first = -1.0, f_final = -1.0;     // residuals of the first and of the last check of this call
  };
  PmeIo stage_pme_io(const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_, void* U_, double* E, void* dpos_,
                     void* dQl_, int on_device) {
    // (the one-shot dipole source is taken off the handle before anything can fail: a call that throws must not leave a
    // pointer behind for the next one)
    U_src_now = on_device ? U_src : nullptr;
    U_src = nullptr;
    ARG_CHECK(snranks == 1 || on_device, "a slab-decomposed handle takes device pointers");
    ARG_CHECK(pos_ && box && Ql_ && E, "null argument");
    const int na = top.na;
    HIP_TRY(hipSetDevice(device));
    PmeIo io;
    io.E = E;
    io.pos = stage_in(s_pos, pos_, 3 * (size_t)na, on_device);
    io.Ql = stage_in(s_Q, Ql_, 9 * (size_t)na, on_device);
    io.pol = lpol ? stage_in(s_pol, pol_, na, on_device) : nullptr;
    io.thole = lpol ? stage_in(s_thole, thole_, na, on_device) : nullptr;
    if (lpol) {
      ARG_CHECK(U_, "polarizable handle needs U_inout");
      if (on_device) io.U = reinterpret_cast<T*>(U_);
      else { s_U.need(3 * (size_t)na * sizeof(T)); HIP_TRY(hipMemcpyAsync(s_U.p, U_, 3 * (size_t)na * sizeof(T), hipMemcpyHostToDevice, stream)); io.U = s_U.as<T>(); }
    }
    if (dpos_) {
      if (on_device) io.dpos = reinterpret_cast<T*>(dpos_);
      else { s_out.need(3 * (size_t)na * sizeof(T)); io.dpos = s_out.as<T>(); }
    }
    if (dQl_) {
      ARG_CHECK(dpos_, "dE_dQlocal requires dE_dpos");
      if (on_device) io.dQl = reinterpret_cast<T*>(dQl_);
      else { s_dQ.need(9 * (size_t)na * sizeof(T)); io.dQl = s_dQ.as<T>(); }
    }
    grad.need(3 * (size_t)na * sizeof(T));   // the gradient buffer is needed internally even for energy-only calls
    io.gbuf = io.dpos ? io.dpos : grad.as<T>();
    mono_ok = (io.dQl == nullptr);
    return io;
  }
  void unstage_pme_io(const PmeIo& io, void* U_, void* dpos_, void* dQl_, int on_device) {
    if (on_device) return;
    const int na = top.na;
    if (dpos_) HIP_TRY(hipMemcpyAsync(dpos_, io.dpos, 3 * (size_t)na * sizeof(T), hipMemcpyDeviceToHost, stream));
    if (dQl_) HIP_TRY(hipMemcpyAsync(dQl_, io.dQl, 9 * (size_t)na * sizeof(T), hipMemcpyDeviceToHost, stream));
    if (lpol) HIP_TRY(hipMemcpyAsync(U_, io.U, 3 * (size_t)na * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  // A closing pass that was enqueued ahead of its check and ran for nothing: undo its energy sums (self and penalty words;
  // atom_parts: the reciprocal energy its gather summed over the atoms as well).  Gradient / dQ are rewritten by the regular
  // closing pass.
  void undo_closing_sums(bool atom_parts) {
    HIP_TRY(hipMemsetAsync(Ed_cur() + E_SELF, 0, 2 * sizeof(double), stream));
    if (atom_parts) HIP_TRY(hipMemsetAsync(Ed_cur() + E_SLOTS, 0, E_PARTS * sizeof(double), stream));
  }
  // Chained form (up to 200k atoms; at 3072 atoms a host synchronisation costs as much as three kernels): when the history says the
  // first check will fail and n Jacobi steps will do, the whole call is enqueued at once -- first field evaluation and its
  // check, then n times (Jacobi step GATED on the previous check's residual on the device: a zero step once a check has
  // passed, after which every later residual repeats the passing one; increment; check), the closing pass -- and read back
  // with one synchronisation.  The host then replays the reference's decisions on the n + 1 residuals: same dipoles,
  // cycle count and flag as the plain loop; a wrong guess costs the kernels that ran for nothing (closing pass when more
  // cycles are needed, increments after the check that passed).
  void scf_chained(ScfRun& run, int nhat, const PmeIo& io, double thresh) {
    const int n_act = run.n_act = nact_known();
    recip_pass_first_field(E_SCF_RECIP);
    auto word = [&](int k) {      // residual of check k: E_FMAX, then the (still zero) chain words of this evaluation
      return k == 0 ? fmax_word() : reinterpret_cast<unsigned long long*>(Ed_cur() + E_FMAX1 + (k - 1));
    };
    next_check_word();
    first_gather_field(field_epilogue(word(0)));
    launch_field_check(word(0));
    const bool early_full = overlap_ok();       // the closing pair kernel next to the last increment's mesh chain
    bool full_rode = false;                     // ... or inside its x pass (pair_rider_ok(): never both)
    // the last residual rides in the closing gather (it reads the accumulated phi anyway): the field gather of the last
    // increment is not run (small single-rank systems; ADMP_CHAIN_LAST_FIELD=1 keeps it: A/B, tests)
    static const bool keep_last = env_flag("ADMP_CHAIN_LAST_FIELD", false);
    const bool last_in_gather = fuse_ok() && !keep_last && n_act > 0;
    for (int c = 0; c < nhat; ++c) {
      scf_jacobi(n_act, word(c), thresh);        // a zero step once a check has passed: later residuals repeat it
      const bool last = c == nhat - 1;
      if (early_full && last)      // (the dipoles are final now)
        scf_increment(n_act, word(c + 1), [&] { stage_pair_full(io.gbuf); }, last_in_gather);
      else
        full_rode = scf_increment(n_act, word(c + 1), nullptr, last && last_in_gather, last ? io.gbuf : nullptr);
      if (!(last && last_in_gather)) launch_field_check(word(c + 1));
    }
    if (!early_full && !full_rode) stage_pair_full(io.gbuf);
    const FinishArgs<T> fin_c = finish_args(io.dpos != nullptr, io.dQl);
    if (last_in_gather) {
      const FieldFin<T> ffl = field_epilogue(word(nhat));
      stage_gather(mesh.as<T>(), io.gbuf, fld_recip.as<T>(), false, Ed_cur() + E_SLOTS, &fin_c, &ffl);
      launch_field_check(word(nhat));            // (done by the epilogue: clears the mark)
    } else {
      stage_gather(mesh.as<T>(), io.gbuf, nullptr, false, Ed_cur() + E_SLOTS, &fin_c);
    }
    launch_finish_only(io.dpos ? io.gbuf : nullptr, io.dQl);
    read_energies(E_PARTS_SUM, io.E);
    nact_seen();
    run.f_first = Eh[E_FMAX];
    run.have_base = true;
    run.phi_accum = true;
    int hit = -1;
    for (int k = 0; k <= nhat && hit < 0; ++k)
      if ((k == 0 ? Eh[E_FMAX] : Eh[E_FMAX1 + k - 1]) < thresh) hit = k;
    if (hit >= 0) {
      run.i = hit;
      run.f_final = hit == 0 ? Eh[E_FMAX] : Eh[E_FMAX1 + hit - 1];
      run.phi_valid = run.done = run.finished = true;
      ev.active = false;
      if (hit < nhat) { ++scf_stats[5]; scf_stats[6] += nhat - hit; }
    } else {
      ++scf_stats[4];   // more cycles are needed: undo the energy sums of the closing pass, go on like the plain loop
      undo_closing_sums(true);
      run.f_final = Eh[E_FMAX1 + nhat - 1];
      scf_jacobi(n_act);
      run.i = nhat + 1;
    }
  }
  // Fixed form (admp_scf_aspc; scf_aspc.h): the call starts from the predictor's dipoles and takes a fixed number of relaxed
  // Jacobi steps -- the chained form without its gates, its replay and its guesses.  First field evaluation, n_corrector
  // times (step with factor omega, increment), the closing pass, all enqueued at once and read back with one
  // synchronisation.  The residual at the predicted dipoles is what the first field finish leaves in E_FMAX.  Between two
  // correctors the field finish needs a zero word for its maximum: the chain words of this evaluation's energy block
  // serve as that, nobody reads them.  The field of the FINAL dipoles is read by nobody either (the closing pair kernel
  // works from the sites, the closing gather from the accumulated phi), so the last increment updates phi alone.
  void scf_fixed(ScfRun& run, const PmeIo& io) {
    const int n_act = run.n_act = nact_known();
    const int nc = aspc.n_corrector();
    const double omega = aspc.omega();
    recip_pass_first_field(E_SCF_RECIP);
    next_check_word();
    first_gather_field(field_epilogue(fmax_word()));
    launch_field_check(fmax_word());
    const bool early_full = overlap_ok();       // the closing pair kernel next to the last increment's mesh chain
    bool full_rode = false;                     // ... or inside its x pass (pair_rider_ok(): never both)
    for (int c = 0; c < nc; ++c) {
      scf_jacobi(n_act, nullptr, 0.0, omega);
      if (c < nc - 1) {
        unsigned long long* w = reinterpret_cast<unsigned long long*>(Ed_cur() + E_FMAX1 + c);
        scf_increment(n_act, w);
        launch_field_check(w);
      } else if (early_full) {                  // (the dipoles are final now)
        scf_increment(n_act, nullptr, [&] { stage_pair_full(io.gbuf); }, true, nullptr, true);
      } else {
        full_rode = scf_increment(n_act, nullptr, nullptr, true, io.gbuf, true);
      }
    }
    if (!early_full && !full_rode) stage_pair_full(io.gbuf);
    const FinishArgs<T> fin_c = finish_args(io.dpos != nullptr, io.dQl);
    stage_gather(mesh.as<T>(), io.gbuf, nullptr, false, Ed_cur() + E_SLOTS, &fin_c);
    launch_finish_only(io.dpos ? io.gbuf : nullptr, io.dQl);
    read_energies(E_PARTS_SUM, io.E);
    nact_seen();
    aspc_resid = Eh[E_FMAX];
    run.have_base = run.phi_accum = run.phi_valid = run.done = run.finished = true;
    run.cyc = nc;
    run.flag = 1;
    ev.active = false;
    scf_stats[7] += nc;
    scf.forget();                               // the residuals of the other forms continue nothing across this call
  }
  // the predictor of a fixed-form or fallback call: U_p from the ring, in ring order; it becomes the call's dipole source
  DevBuf aspc_set[kAspcMaxSets], aspc_pred;
  void aspc_predict() {
    const size_t n = 3 * (size_t)top.na;
    AspcSets<T> h;
    h.n = aspc.slots();
    for (int j = 1; j <= h.n; ++j) { h.U[j - 1] = aspc_set[aspc.slot(j)].template as<T>(); h.B[j - 1] = aspc_coef(aspc.order(), j); }
    aspc_pred.need(n * sizeof(T));
    { TIMED("aspc_predict"); launch_aspc_predict<T>(stream, (long)n, h, aspc_pred.as<T>()); }
    U_src_now = aspc_pred.p;
  }
  // the dipoles this call used for its forces join the history: one copy on the stream, no host round trip
  void aspc_store(const T* U) {
    const size_t bytes = 3 * (size_t)top.na * sizeof(T);
    DevBuf& slot = aspc_set[aspc.next_slot()];
    slot.need(bytes);                           // (grows only after set_topology, which has dropped the history)
    aspc_dirty = true;
    HIP_TRY(hipMemcpyAsync(slot.p, U, bytes, hipMemcpyDeviceToDevice, stream));
    aspc.push();
    aspc_dirty = false;
  }
  // Steady-state MD regime (the previous call converged at its first check): evaluate the FIRST SCF cycle
  // with the full kernels -- they produce dE/dU alongside the gradient -- so that, when the check passes
  // again, the step is already finished (no separate field kernels, no second pass).  Same arithmetic and
  // same (U, flag, i) as the plain loop; a failed check only costs the difference between the kernels.
  // The closing kernel is enqueued speculatively as well, so the step has ONE host synchronisation.
  void scf_speculative(ScfRun& run, const PmeIo& io, double thresh) {
    recip_pass_pair_full(E_SCF_RECIP, io.gbuf, fld_pair.as<T>());
    // small systems are dispatch-bound: the field finish rides in the gather's epilogue; larger ones keep the two
    // kernels (98k atoms: gather 26 -> 47 us fused against 9 us saved; 1M atoms: 0.40 vs 0.31 + 0.056 ms)
    const bool fuse_ff = top.na <= fuse_ff_max();
    const bool fuse_g = fuse_ff && snranks == 1;      // (not fuse_ok(): that one also asks for !ev.home)
    const FinishArgs<T> fin_s = finish_args(io.dpos != nullptr, io.dQl);
    stage_gather(mesh.as<T>(), io.gbuf, fld_recip.as<T>(), fuse_g, nullptr, fuse_g ? &fin_s : nullptr);
    const bool pull = !ev.home && top.inv_ptr;          // the atomics-free closing kernel can carry the field finish
    if (!fuse_g && !pull) launch_field_finish_only();
    launch_finish_only(io.dpos ? io.gbuf : nullptr, io.dQl, !fuse_g && pull);
    const double fmax = read_energies(E_SCF_RECIP, io.E);
    run.f_first = run.f_final = fmax;
    nact_seen();
    run.n_act = nact_known();
    if (fmax < thresh) {
      run.phi_valid = run.done = run.finished = true;
      ev.active = false;
    } else {   // undo the speculative energy sums; gradient / dQ are rewritten by the regular closing pass
      ++scf_stats[2];
      undo_closing_sums(false);
      scf_jacobi(run.n_act);
      run.i = 1;
      run.have_base = true;      // the full kernels left the field of the old dipoles behind: continue by increments
    }
  }
  // the reference's loop (admp/pme.py:132-143), from cycle run.i on: the whole SCF of a plain call, what a failed guess of
  // the other two forms left to do, nothing after a guess that held
  void scf_loop(ScfRun& run, double thresh, int max_cycle) {
    for (; !run.done && run.i < max_cycle; ++run.i) {     // admp/pme.py:132-138
      if (!run.have_base) {        // first field evaluation of the call: everything, at the polarizable sites
        recip_pass_first_field(E_SCF_RECIP);
        unsigned long long* w = fuse_ok() ? next_check_word() : nullptr;
        first_gather_field(field_epilogue(w));
        run.have_base = true;
      } else {
        scf_increment(run.n_act, fuse_ok() ? next_check_word() : nullptr);
        run.phi_accum = true;
      }
      const double fmax = scf_check(&run.n_act);
      if (run.f_first < 0.0) run.f_first = fmax;
      run.f_final = fmax;
      if (fmax < thresh) { run.phi_valid = true; break; }
      scf_jacobi(run.n_act);
    }
    if (run.i == max_cycle) run.i = max_cycle - 1;   // python's loop variable after exhaustion
    run.cyc = run.i;
    scf_stats[7] += run.cyc;
    run.flag = (run.i != max_cycle - 1);             // admp/pme.py:139-143
  }
  // gradient, dE/dQ_local and the four energies at the final dipoles -- whatever of it the SCF has not produced already
  void closing_pass(const ScfRun& run, const PmeIo& io) {
    const bool atoms_energy = run.phi_valid && run.phi_accum;
    if (!run.done) {
      if (!run.phi_valid) recip_pass_pair_full(E_RECIP, io.gbuf);
      else stage_pair_full(io.gbuf);
      // (the partial words are zero: nothing else of this evaluation writes them)
      const FinishArgs<T> fin_t = finish_args(io.dpos != nullptr, io.dQl);
      stage_gather(mesh.as<T>(), io.gbuf, nullptr, false, atoms_energy ? Ed_cur() + E_SLOTS : nullptr,
                   run.finished ? nullptr : &fin_t);
    }
    if (!run.finished)
      stage_finish(io.dpos ? io.gbuf : nullptr, io.dQl,
                   atoms_energy ? (int)E_PARTS_SUM : (run.phi_valid ? (int)E_SCF_RECIP : (int)E_RECIP), io.E);
    join_side();
  }

  void pme(const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_, int ns,
           const double* mS, const double* pS, void* U_, int max_cycle, double thresh, double* E, void* dpos_,
           void* dQl_, int* ncyc, int* conv, int on_device) override {
    const PmeIo io = stage_pme_io(pos_, box, Ql_, pol_, thole_, U_, E, dpos_, dQl_, on_device);
    // admp_scf_aspc with a full history: the call starts from the predicted dipoles, whatever the caller passed
    const bool aspc_on = lpol && aspc.on() && !aspc_hold && snranks == 1;
    const bool predicted = aspc_on && aspc.full() && max_cycle >= 1 && have_top && have_ewald && pl.have();
    if (predicted) aspc_predict();
    stage_begin(io.pos, box, io.Ql, io.pol, io.thole, ns, mS, pS, io.U);
    ScfRun run;
    // the fixed form needs the polarizable rows on the host (can_chain of scf.plan); otherwise the ordinary SCF from U_p
    const bool fixed = predicted && !act_fresh && act_n > 0;
    if (lpol && fixed) {
      scf_fixed(run, io);
    } else if (lpol) {
      ARG_CHECK(max_cycle >= 1, "max_cycle must be >= 1");
      // which form of the first cycle: ADMP_SPECULATE=0 / 1 forces the plain / the speculative one (A/B, tests)
      static const ScfSwitches sw = {env_int("ADMP_SPECULATE", -1), env_int("ADMP_SCF_CHAIN_MAX", 200000)};
      const ScfPlan plan = scf.plan(thresh, top.na, max_cycle, snranks > 1 || (!act_fresh && act_n > 0), sw);
      const bool chain = plan.form == ScfForm::chained, speculate = plan.form == ScfForm::speculative;
      static const bool scf_trace = getenv("ADMP_SCF_TRACE") != nullptr;     // one line per call: which form ran
      if (scf_trace) fprintf(stderr, "[admp scf] %s (predicted residual %.4g, threshold %.4g, %d steps)\n",
                             chain ? "chained" : (speculate ? "speculative" : "plain"), plan.pred, thresh, chain ? plan.nhat : 0);
      ++scf_stats[chain ? 3 : (speculate ? 1 : 0)];
      if (chain) scf_chained(run, plan.nhat, io, thresh);
      if (speculate) scf_speculative(run, io, thresh);
      scf_loop(run, thresh, max_cycle);
      scf.observe(run.f_first, run.f_final, run.cyc);
    }
    closing_pass(run, io);
    if (aspc_on) {
      aspc_store(io.U);
      ++aspc_calls[fixed ? 0 : (predicted ? 2 : 1)];
    }
    unstage_pme_io(io, U_, dpos_, dQl_, on_device);
    if (ncyc) *ncyc = run.cyc;
    if (conv) *conv = run.flag;
  }

  // energy_fn / grad_U_fn / grad_pos_fn of the reference (admp/pme.py:69-78): energy and its derivatives at dipoles the
  // CALLER supplies -- no SCF.  Device pointers only.  dU = dE/dUind_global (Cartesian, incl. the self and penalty terms).
  void pme_at_U(const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_, int ns,
                const double* mS, const double* pS, const void* U_, double* E, void* dpos_, void* dU_, void* dQl_) override {
    ARG_CHECK(lpol, "polarizable handle required (the non-polarizable energy is admp_pme_energy_grad)");
    ARG_CHECK(pos_ && box && Ql_ && U_ && E, "null argument");
    ARG_CHECK(!dQl_ || dpos_, "dE_dQlocal requires dE_dpos");
    const int na = top.na;
    grad.need(3 * (size_t)na * sizeof(T));
    T* gbuf = dpos_ ? reinterpret_cast<T*>(dpos_) : grad.as<T>();
    mono_ok = (dQl_ == nullptr);
    if (snranks > 1) {      // slab rank: the rows of the atoms it reads are filled in from their owners -- in a copy, the caller's
      s_U.need(3 * (size_t)na * sizeof(T));                            // array is an input here (its home rows must be valid)
      HIP_TRY(hipMemcpyAsync(s_U.p, U_, 3 * (size_t)na * sizeof(T), hipMemcpyDeviceToDevice, stream));
      U_ = s_U.p;
    }
    stage_begin(pos_, box, Ql_, pol_, thole_, ns, mS, pS, const_cast<void*>(U_));
    const bool wantU = dU_ != nullptr;
    stage_pair_full(gbuf, wantU ? fld_pair.as<T>() : nullptr);
    recip_pass(E_RECIP);
    stage_gather(mesh.as<T>(), gbuf, wantU ? fld_recip.as<T>() : nullptr);
    if (wantU) {
      launch_field_finish_only();
      HIP_TRY(hipMemcpyAsync(dU_, field.p, 3 * (size_t)na * sizeof(T), hipMemcpyDeviceToDevice, stream));
    }
    stage_finish(dpos_ ? gbuf : nullptr, reinterpret_cast<T*>(dQl_), E_RECIP, E);
    scf.forget();
  }

  void local_frames(const void* pos, const double* box, void* out) override {
    ARG_CHECK(have_top && pos && box && out, "topology must be set; null argument");
    double inv[9], vol;
    Box<T> bx = make_box(box, inv, &vol);
    launch_local_frames<T>(stream, top, reinterpret_cast<const T*>(pos), bx, reinterpret_cast<T*>(out));
  }

  // admp_pme_dipoles: the frames are those of this handle's topology, which is why the entry lives here.  Every refusal comes
  // before the first launch; nothing is read back.
  DevBuf dip_rows;
  void dipoles(const void* pos, const double* box, const void* Ql, const void* U, const void* inv_mass, int n_groups,
               const int32_t* group_start, const int32_t* group_atoms, double* mu_groups, double* out16) override {
    if (snranks > 1) throw Err{ADMP_E_STATE, "admp_pme_dipoles does not work on a slab-decomposed handle"};
    if (!have_top) throw Err{ADMP_E_STATE, "admp_set_topology must precede admp_pme_dipoles"};
    ARG_CHECK(pos && box && Ql && inv_mass && group_start && group_atoms && out16, "null argument");
    ARG_CHECK(n_groups >= 0, "negative number of groups");
    for (int k = 0; k < 9; ++k) ARG_CHECK(std::isfinite(box[k]), "box is not finite");
    double inv[9], vol;
    const Box<T> bx = make_box(box, inv, &vol);      // (refuses a singular box)
    ARG_CHECK(std::isfinite(vol), "box is not finite");
    dip_rows.need(sizeof(double) * kDipoleRowWords * (size_t)std::max(1, dipole_rows(n_groups)));
    const int rc = launch_dipoles<T>(stream, top, reinterpret_cast<const T*>(pos), bx, reinterpret_cast<const T*>(Ql),
                                     reinterpret_cast<const T*>(U), reinterpret_cast<const T*>(inv_mass), n_groups, group_start,
                                     group_atoms, mu_groups, dip_rows.as<double>(), out16);
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("admp_pme_dipoles: ") + hipGetErrorString((hipError_t)rc)};
  }

  // ---- box gradient: dE/dbox at fixed Cartesian positions = jax.grad(get_energy, argnums=1) of the
  // reference (admp/pme.py:108 with argnums; README.md:7 "force and virial").  The device kernels accumulate
  //   xw[9]  sum shift (x) dE/dr over boundary-crossing pairs and frame vectors + sum_atoms x (x) dE_recip/dx
  //   yy[9]  sum_atoms dE_recip/dAop (the multipole operators of the spread)
  //   tk[6]  sum_k w dG/dk^2 |S|^2 k (x) k
  // and the host folds them with box^-1 (A = inv, rows c, columns j; Aop[i][j] = -K_i A[j][i]):
  //   dE/dbox = -A^T xw  -  A^T (dE/dA)_op A^T  -  2 tk A^T  -  E_recip A^T ,   (dE/dA)_op[j][i] = -K_i yy[i][j]
  DevBuf vir_d;
  enum { V_XW = 0, V_Y = 9, V_TK = 18, V_WORDS = 24 };
  double* vir_begin() {
    vir_d.need(V_WORDS * sizeof(double));
    HIP_TRY(hipMemsetAsync(vir_d.p, 0, V_WORDS * sizeof(double), stream));
    return vir_d.as<double>();
  }
  void vir_assemble(const double* inv, double Erec, double* out) {
    double h[V_WORDS];
    HIP_TRY(hipMemcpyAsync(h, vir_d.p, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    auto A = [&](int c, int j) { return inv[3 * c + j]; };
    const double* xw = h + V_XW;
    const double* yy = h + V_Y;
    const double tk[9] = {h[V_TK + 0], h[V_TK + 3], h[V_TK + 4], h[V_TK + 3], h[V_TK + 1], h[V_TK + 5],
                          h[V_TK + 4], h[V_TK + 5], h[V_TK + 2]};
    double dA[9];   // (dE/dA)_op[j][i]
    for (int j = 0; j < 3; ++j)
      for (int i = 0; i < 3; ++i) dA[3 * j + i] = -(double)K[i] * yy[3 * i + j];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        double v = 0.0;
        for (int c = 0; c < 3; ++c) v -= A(c, a) * xw[3 * c + b];
        for (int j = 0; j < 3; ++j)
          for (int i = 0; i < 3; ++i) v -= A(j, a) * dA[3 * j + i] * A(b, i);
        for (int j = 0; j < 3; ++j) v -= 2.0 * tk[3 * a + j] * A(b, j);
        v -= Erec * A(b, a);
        out[3 * a + b] = v;
      }
  }
  // spread -> r2c -> k-tensor sums -> G multiply (+energy) -> c2r, always through rocFFT (MeshConv::convolve_virial: the
  // fused direct-DFT x pass never holds the bare spectrum)
  void recip_pass_virial(int slot, int which, double vol, double* acc, int reuse_bins = 0, int lpol_sites = -1) {
    need_eval_or_disp();
    { TIMED("spread"); spread_sites(vs_n, vs_sites, lpol_sites < 0 ? lpol : lpol_sites, vs_g, mesh.as<T>(), nullptr, 1, reuse_bins); }
    mc.convolve_virial(mesh.as<T>(), mc.gtab_cur, Ed_cur(), slot, which, vol, kappa, ref_korder, acc + V_TK);
  }
  int vs_n = 0; const Site<T>* vs_sites = nullptr; RecipGeom<T> vs_g;
  void need_eval_or_disp() { ARG_CHECK(vs_sites != nullptr, "internal: virial pass without sites"); }
  void upload_binv(const double* inv) { mc.upload_binv(inv); }
  // The same on a slab rank (round 4): the pair / gather / frame sums run over the rank's home rows and atoms, the k-tensor
  // sums over the y rows it holds of the transposed spectrum (between the x transforms of the distributed convolution, which
  // therefore takes the unfused x passes here), and the 24 device words are summed over the ranks before the host folds
  // them -- every rank returns the full dE/dbox.
  void convolve_slab_virial(T* mesh_p, int which, double vol, double* acc) {
    mc.convolve_slab_virial(mesh_p, mc.gtab_cur, Ed_cur(), E_RECIP, which, vol, kappa, ref_korder, acc + V_TK);
  }
  void pme_box_grad(const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_, int ns,
                    const double* mS, const double* pS, const void* U_, double* E, double* dbox) override {
    ARG_CHECK(pos_ && box && Ql_ && E && dbox, "null argument");
    if (lpol) ARG_CHECK(U_, "polarizable handle needs the induced dipoles");
    const bool slab = snranks > 1;
    const int na = top.na;
    grad.need(3 * (size_t)na * sizeof(T));
    T* gbuf = grad.as<T>();
    mono_ok = true;
    stage_begin(pos_, box, Ql_, pol_, thole_, ns, mS, pS, const_cast<void*>(U_));
    double inv[9], vol;
    make_box(box, inv, &vol);
    upload_binv(inv);
    double* acc = vir_begin();
    stage_pair_full(gbuf);
    launch_pair_virial<T>(stream, na, wnbr(), sites.as<Site<T>>(), ev.bx, ev.tab, (T)kappa, lpol, acc + V_XW,
                          slab ? pair_rows() : nullptr, ev.n_home);
    if (slab) stage_spread(mesh.as<T>());
    else { vs_n = na; vs_sites = sites.as<Site<T>>(); vs_g = ev.g; }
    if (!slot_clean[E_RECIP]) HIP_TRY(hipMemsetAsync(Ed_cur() + E_RECIP, 0, sizeof(double), stream));
    slot_clean[E_RECIP] = false;
    if (slab) convolve_slab_virial(mesh.as<T>(), 1, vol, acc);
    else recip_pass_virial(E_RECIP, 1, vol, acc);
    // (one rank: ev.home is null and ev.n_home the atom count)
    stage_gather(mesh.as<T>(), gbuf);
    launch_gather_virial<T>(stream, ev.n_home, sites.as<Site<T>>(), lpol, ev.g, mesh.as<T>(), acc + V_XW, acc + V_Y, ev.home);
    if (lmax > 0)
      launch_frame_virial<T>(stream, top, ev.pos, ev.bx, sites.as<Site<T>>(), lpol, (T)kappa, pot.as<T>(), acc + V_XW, ev.home,
                             ev.n_home);
    // (the frame sums need the TOTAL potential of the home sites: pot holds pair + reciprocal space, the self term is added
    // by the kernel itself)
    stage_finish(nullptr, nullptr, E_RECIP, E);
    vs_sites = nullptr;
    if (slab) { TIMED("comm_energies"); comm.all_reduce(stream, acc, V_WORDS, ADMP_T_F64, ADMP_OP_SUM, ADMP_TAG_ENERGIES); }
    vir_assemble(inv, E[1], dbox);
    scf.forget();
  }

  // dispersion PME box gradient on a slab rank (round 4): the pair sums over its home rows, the channels spread / gathered on
  // its home atoms through the distributed convolution with the k-tensor sums between the x transforms, the self term over
  // its home atoms; the 24 device sums are added over the ranks
  void disp_box_grad_slab(const void* pos_, const double* box, const void* clist_, int pmax, int ns, const double* mS, double* E,
                          double* dbox) {
    const int na = top.na;
    RecipGeom<T> g;
    const ScalarCall sc = scalar_begin(box, ns, mS, pos_, clist_, 3, nullptr, 1, 2 * E_WORDS, &g);
    const T* pos = sc.pos; const T* cl = sc.par;
    double* Ed = sc.Ed;
    ARG_CHECK(spread_uses_bricks(1 << 30, g), "slab-decomposed dispersion PME needs at least 17 local mesh planes and K2, K3 >= 17");
    double* acc = vir_begin();
    cls_sites_na = slab_sites_na = -1;
    const ScalarRows sr = scalar_rows(pos, g, K[0], mc.X0, mc.X1, true);
    launch_disp_pair<T>(stream, na, pl.table(), pack_srows(pos, cl, 3), sc.bx, sc.tab, (T)kappa, pmax, sc.dpos, Ed, sr.rows, sr.n, cutoff);
    launch_scalar_pair_virial<T>(stream, 0, na, pl.table(), pos, cl, sc.bx, sc.tab, (T)kappa, pmax, acc + V_XW, cutoff, sr.rows, sr.n);
    const int nch = (pmax - 4) / 2;
    const size_t nreal = nreal_local();
    mesh.need(nch * nreal * sizeof(T));
    sites.need(sizeof(Site<T>) * (size_t)na);
    ensure_bins(std::max(sr.n, 1));
    spread_bricks(sr, g, nch, pos, cl, nullptr);
    double* scratchE = Ed + E_WORDS;              // (the all-atom self sums of launch_scalar_sites are not this rank's: discarded)
    for (int c = 0; c < nch; ++c) {
      ensure_gtab(box, sc.inv, sc.vol, 6 + 2 * c);
      upload_binv(sc.inv);
      convolve_slab_virial(mesh.as<T>() + c * nreal, 6 + 2 * c, sc.vol, acc);
      launch_scalar_sites<T>(stream, na, pos, cl, 3, c, 0.0, sites.as<Site<T>>(), scratchE);
      launch_gather_virial<T>(stream, sr.n, sites.as<Site<T>>(), 0, g, mesh.as<T>() + c * nreal, acc + V_XW, acc + V_Y, sr.home);
    }
    launch_scalar_self<T>(stream, nch, sr.n, cl, 3, sr.home, disp_kp().data(), Ed);
    read_scalar_energies(Ed, E, 3);
    { TIMED("comm_energies"); comm.all_reduce(stream, acc, V_WORDS, ADMP_T_F64, ADMP_OP_SUM, ADMP_TAG_ENERGIES); }
    vir_assemble(sc.inv, E[1], dbox);
  }

  void disp_box_grad(const void* pos_, const double* box, const void* clist_, int pmax, int ns, const double* mS, double* E,
                     double* dbox) override {
    ARG_CHECK(have_top && have_ewald && pl.have(), "topology, ewald parameters and pairs must be set first");
    ARG_CHECK(pos_ && box && clist_ && E && dbox, "null argument");
    ARG_CHECK(pmax == 6 || pmax == 8 || pmax == 10, "pmax must be 6, 8 or 10");
    if (snranks > 1) {
      disp_box_grad_slab(pos_, box, clist_, pmax, ns, mS, E, dbox);
      return;
    }
    const int na = top.na;
    RecipGeom<T> g;
    const ScalarCall sc = scalar_begin(box, ns, mS, pos_, clist_, 3, nullptr, 1, E_SLOTS, &g);
    const T* pos = sc.pos; const T* cl = sc.par;
    double* Ed = sc.Ed;
    double* acc = vir_begin();
    launch_disp_pair<T>(stream, na, pl.table(), pack_srows(pos, cl, 3), sc.bx, sc.tab, (T)kappa, pmax, sc.dpos, Ed, nullptr, 0, cutoff);
    launch_scalar_pair_virial<T>(stream, 0, na, pl.table(), pos, cl, sc.bx, sc.tab, (T)kappa, pmax, acc + V_XW, cutoff);
    cls_sites_na = slab_sites_na = -1;   // other rows than an electrostatics evaluation's
    sites.need(sizeof(Site<T>) * (size_t)na);
    ensure_bins(na);
    const std::array<double, 3> kp = disp_kp();
    const int nch = (pmax - 4) / 2;
    vs_n = na; vs_sites = sites.as<Site<T>>(); vs_g = g;
    for (int c = 0; c < nch; ++c) {
      ensure_gtab(box, sc.inv, sc.vol, 6 + 2 * c);
      upload_binv(sc.inv);
      launch_scalar_sites<T>(stream, na, pos, cl, 3, c, kp[c], sites.as<Site<T>>(), Ed);
      recip_pass_virial(E_RECIP, 6 + 2 * c, sc.vol, acc, c > 0, 0);
      launch_gather_virial<T>(stream, na, sites.as<Site<T>>(), 0, g, mesh.as<T>(), acc + V_XW, acc + V_Y);
    }
    vs_sites = nullptr;
    double Eh2[E_SLOTS];
    HIP_TRY(hipMemcpyAsync(Eh2, Ed, sizeof(Eh2), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    E[0] = Eh2[E_REAL]; E[1] = Eh2[E_RECIP]; E[2] = Eh2[E_SELF];
    vir_assemble(sc.inv, E[1], dbox);
  }

  void tt_box_grad(const void* pos_, const double* box, const void* abqc_, int ns, const double* mS, double* E,
                   double* dbox) override {
    ARG_CHECK(have_top && pl.have(), "topology and pairs must be set first");
    ARG_CHECK(pos_ && box && abqc_ && E && dbox, "null argument");
    const int na = top.na;
    const ScalarCall sc = scalar_begin(box, ns, mS, pos_, abqc_, 4, nullptr, 1, E_WORDS);
    double* acc = vir_begin();
    ScalarRows sr{nullptr, na, nullptr};
    if (snranks > 1) sr = virtual_slab_rows(sc.pos, sc.inv);     // as in tt(); the sums are added over the ranks
    launch_tt_pair<T>(stream, na, pl.table(), pack_srows(sc.pos, sc.par, 4), sc.bx, sc.tab, sc.dpos, sc.Ed, sr.rows, sr.n, cutoff);
    launch_scalar_pair_virial<T>(stream, 1, na, pl.table(), sc.pos, sc.par, sc.bx, sc.tab, T(0), 0, acc + V_XW, cutoff, sr.rows, sr.n);
    read_scalar_energies(sc.Ed, E, 1);
    if (snranks > 1) { TIMED("comm_energies"); comm.all_reduce(stream, acc, V_WORDS, ADMP_T_F64, ADMP_OP_SUM, ADMP_TAG_ENERGIES); }
    vir_assemble(sc.inv, 0.0, dbox);      // only the xw sums are non-zero here
  }

  // ---- neighbour search and table builds: the arguments checked and turned into a box here, the work in pl (pair_list.h) ----
  void nbr_count(int na, const void* pos, const double* box, double rc, int64_t* n_pairs) override {
    ARG_CHECK(na > 0 && pos && box && rc > 0 && n_pairs, "bad argument");
    double inv[9], vol, heights[3];
    const Box<T> b = make_box(box, inv, &vol);
    cell_heights_within(inv, heights, rc);
    pl.count<T>(na, reinterpret_cast<const T*>(pos), b, heights, rc, n_pairs);
  }
  void nbr_fill(int32_t* pairs) override { pl.fill<T>(pairs); }

  // admp_prune_pairs: from now on the calculators walk the entries of the current table that lie below rc (PairList::prune)
  void prune_pairs(const void* pos, const double* box, double rc) override {
    pl.require_own_table();
    ARG_CHECK(snranks == 1, "admp_prune_pairs: single-rank handles only");
    ARG_CHECK(pos && box, "null argument");
    double inv[9], vol;
    const Box<T> b = make_box(box, inv, &vol);
    pl.prune<T>(top.na, reinterpret_cast<const T*>(pos), b, rc);
  }
  void nbr_table(const void* pos, const double* box, double rc) override {
    ARG_CHECK(have_top, "admp_set_topology must precede admp_set_pairs_from_positions");
    ARG_CHECK(pos && box && rc > 0, "bad argument");
    double inv[9], vol, heights[3];
    const Box<T> b = make_box(box, inv, &vol);
    cell_heights_within(inv, heights, rc);
    // Slab rank with a mesh (round 4): only the rows of the atoms whose stencil base plane lies within the rank's slab plus a
    // margin -- half the list cutoff (far more than half a skin) plus 4 planes for the pair potentials' slab rule -- are built:
    // the search then costs the rank its share of the box, not the box.  ADMP_SLAB_ROWS=0: every row on every rank.
    RowFilter rf;
    static const bool rows_on = env_flag("ADMP_SLAB_ROWS", true);
    if (rows_on && snranks > 1 && have_ewald && comm.have) {
      update_slab();
      const int mp = (int)std::ceil(0.5 * rc / (heights[0] / K[0])) + 4;
      const int width = (mc.X1 - mc.X0) + 2 * mp;
      if (width < K[0]) { rf.on = 1; rf.K0 = K[0]; rf.lo = ((mc.X0 - mp) % K[0] + K[0]) % K[0]; rf.width = width; }
    }
    pl.build_from_positions<T>(top, reinterpret_cast<const T*>(pos), b, heights, rc, rf);
  }

  void slab_info(int64_t* o) override {
    ARG_CHECK(have_ewald, "admp_set_ewald first");
    update_slab();
    o[0] = mc.X0; o[1] = mc.X1; o[2] = mc.Y0; o[3] = mc.Y1; o[4] = nloc0(); o[5] = kGhost; o[6] = K[0]; o[7] = K[1]; o[8] = K[2] / 2 + 1;
    o[9] = srank; o[10] = snranks;
  }
  DevBuf srow_d;      // packed (position, parameters) rows of the scalar pair kernels, rebuilt per call
  const SRow<T>* pack_srows(const T* pos, const T* par, int np) {
    srow_d.need(sizeof(SRow<T>) * (size_t)top.na);
    launch_pack_scalar_rows<T>(stream, top.na, np, pos, par, srow_d.as<SRow<T>>());
    return srow_d.as<SRow<T>>();
  }
  // energies of a dispersion / pair-potential call: (real, recip, self) of all ranks
  void read_scalar_energies(double* Ed, double* E, int n, bool types_checked = false) {
    double Eh2[E_WORDS];
    if (snranks > 1) sum_energy_words(Ed, E_RECIP);
    HIP_TRY(hipMemcpyAsync(Eh2, Ed, sizeof(Eh2), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const double* src = snranks > 1 ? Eh2 + E_RED : Eh2;      // (E_REAL, E_RECIP, E_SELF are words 0, 1, 2 either way)
    if (types_checked && Eh2[E_FMAX] != 0.0)      // (k_types_check counted rows that differ from their type's coefficients)
      throw Err{ADMP_E_ARG, "admp_disp_set_types: c_list rows differ from the coefficients of their types"};
    for (int k = 0; k < n; ++k) E[k] = src[k];
  }
  // rows of a scalar pair / dispersion call: all atoms in the table's length-sorted order, or -- on a slab rank -- the
  // home rows of this evaluation (ownership by the stencil base plane of mesh geometry g)
  struct ScalarRows { const int* rows; int n; const int* home; };
  ScalarRows scalar_rows(const T* pos, const RecipGeom<T>& g, int K0v, int X0v, int X1v, bool need_bases) {
    const int na = top.na;
    const int* order = pl.table().order_plain ? pl.table().order_plain : pl.table().order;
    if (snranks > 1 || need_bases) {
      bases_d.need(sizeof(int4) * (size_t)na);
      TIMED("atom_bases");
      launch_atom_bases<T>(stream, na, pos, g, bases_d.as<int4>());
    }
    if (snranks == 1) return {order, na, nullptr};
    sl.decompose(slab_in(bases_d.as<int4>(), nullptr, K0v, X0v, X1v, order, false));
    return {sl.rows(), sl.n_home(), sl.home()};
  }
  // ... of a pair potential on a slab rank: it has no mesh, so ownership goes by x-slabs of a virtual one of 64 planes per rank
  ScalarRows virtual_slab_rows(const T* pos, const double* inv) {
    ARG_CHECK(comm.have, "slab-decomposed handle without a communicator (admp_set_comm)");
    RecipGeom<T> g;
    const int Kv = 64 * snranks;
    g.K[0] = Kv; g.K[1] = g.K[2] = 32;
    for (int k = 0; k < 9; ++k) { g.hinv[k] = (T)inv[k]; g.Aop[k] = g.Jac[k] = T(0); }
    g.xoff = 64 * srank; g.nloc0 = 64 + kGhost; g.wrap0 = 1 << 30;
    return scalar_rows(pos, g, Kv, 64 * srank, 64 * (srank + 1), true);
  }

  // ---- the opening and the closing of a scalar call (dispersion PME, Tang-Toennies, traced pair programs) ----------------
  // Filled on the stack by scalar_begin: the cell, the scale table, the inputs on the device, where the gradient goes (the
  // caller's device array, or `grad` for a host caller, a caller without one and the box gradients) and the energy words.
  struct ScalarCall {
    const double* h; Box<T> bx; double inv[9], vol;      // the caller's cell, its device form, inverse and volume
    ScaleTab<T> tab;
    const T* pos; const T* par;
    T* dpos;
    double* Ed;
  };
  // par_: npar words per atom; zero_words: how many of the energy words the call starts from zero -- E_SLOTS: the energies
  // (and the word the type check counts into, E_FMAX), enough for a call that reads them back itself; E_WORDS: the whole
  // half, as read_scalar_energies copies it (with the words packed for the sum over the ranks); 2 * E_WORDS: the second half
  // too, where the slab box gradient leaves the self sums it discards.  g: the call works on the mesh -- plans and buffers
  // first, then its geometry (with its refusal of meshes shorter than the splines).
  ScalarCall scalar_begin(const double* box, int ns, const double* mS, const void* pos_, const void* par_, size_t npar,
                          void* dpos_, int on_device, size_t zero_words, RecipGeom<T>* g = nullptr) {
    const size_t na = (size_t)top.na;
    ScalarCall sc;
    sc.h = box;
    sc.bx = make_box(box, sc.inv, &sc.vol);
    if (g) { ensure_mesh(); *g = make_geom(sc.inv); }
    sc.tab = make_tab(ns, mS, nullptr);
    sc.pos = stage_in(s_pos, pos_, 3 * na, on_device);
    sc.par = stage_in(s_par, par_, npar * na, on_device);
    grad.need(3 * na * sizeof(T));
    sc.dpos = (dpos_ && on_device) ? reinterpret_cast<T*>(dpos_) : grad.as<T>();
    energies_d.need(2 * E_WORDS * sizeof(double));
    ehalf = 0; other_clean = false;
    sc.Ed = energies_d.as<double>();
    HIP_TRY(hipMemsetAsync(sc.Ed, 0, zero_words * sizeof(double), stream));
    return sc;
  }
  // the gradient of a host caller goes back; sync = false: the caller has more to copy and synchronises itself
  void scalar_return_grad(const ScalarCall& sc, void* dpos_, int on_device, bool sync = true) {
    if (!dpos_ || on_device) return;
    HIP_TRY(hipMemcpyAsync(dpos_, sc.dpos, 3 * (size_t)top.na * sizeof(T), hipMemcpyDeviceToHost, stream));
    if (sync) HIP_TRY(hipStreamSynchronize(stream));
  }

  // ---- tables of a dispersion call ------------------------------------------------------------------------------------------
  // self / gamma-point factors of the powers 6, 8, 10 (admp/disp_pme.py:254-279)
  std::array<double, 3> disp_kp() const {
    return {-std::pow(kappa, 6) / 12.0, -std::pow(kappa, 8) / 48.0, -std::pow(kappa, 10) / 240.0};
  }
  // coefficients of the type table by (power, type), for the x passes that mix type meshes into powers
  MixTab disp_mix(int nch) const {
    MixTab mix;
    mix.nch = nch; mix.nt = disp_nt;
    for (int c = 0; c < 3; ++c)
      for (int t = 0; t < 4; ++t) mix.c[c][t] = (c < nch && t < disp_nt) ? disp_ctab[t][c] : 0.0;
    return mix;
  }
  // the G tables of the first nch powers
  DftTabs<T> disp_tabs(const double* box, const double* inv, double vol, int nch) {
    DftTabs<T> tabs;
    for (int c = 0; c < nch; ++c) { ensure_gtab(box, inv, vol, 6 + 2 * c); tabs.p[c] = mc.gtab_cur; }
    return tabs;
  }
  // ONE binning and ONE spread of nmesh meshes straight from the caller's arrays (disp_kernels.hip): one mesh per power from
  // the coefficient rows cl, or -- types given -- one per type
  void spread_bricks(const ScalarRows& sr, const RecipGeom<T>& g, int nmesh, const T* pos, const T* cl, const int* types) {
    int rc = launch_bin_bricks<T>(stream, sr.n, (const Site<T>*)nullptr, g, bins, sr.home, bases_d.as<int4>());
    if (rc == 0)
      rc = types ? launch_spread_typed<T>(stream, nmesh, pos, types, g, bins, mesh.as<T>(), (long)nreal_local())
                 : launch_spread_scalar<T>(stream, nmesh, pos, cl, 3, g, bins, mesh.as<T>(), (long)nreal_local());
    if (rc != 0)
      throw Err{ADMP_E_HIP, std::string(types ? "dispersion spread (typed): " : "dispersion spread: ") + hipGetErrorString((hipError_t)rc)};
    bins.counters_zero = true;
  }

  // admp_disp_set_types: the atoms' coefficient rows take nt <= 3 distinct values; types (device int32[Na], the caller's) picks
  // the row ctab[type][3] of every atom.  Used by the single-rank fused-x path in single precision (typed meshes: one spread
  // and one gather per ATOM instead of per channel, nt transforms instead of one per channel); verified against c_list in
  // every call that uses it.  nt = 0: forget.
  int disp_nt = 0;
  const int* disp_types = nullptr;
  bool disp_counts_ok = false, disp_onehot_ok = false;      // per type table: atoms per type (host), one-hot weights (device)
  double disp_counts[4] = {0, 0, 0, 0};
  // self term of the typed form: sum_p kp[p] sum_t n_t c_p,t^2 (admp/disp_pme.py:254-279 summed by type)
  double typed_self_energy(int na, int nch, const double* kp) {
    if (!disp_counts_ok) {
      tcount_d.need(256);
      int* cd = reinterpret_cast<int*>(tcount_d.p);
      int ch[4];
      HIP_TRY(hipMemsetAsync(cd, 0, 4 * sizeof(int), stream));
      launch_type_counts(stream, na, disp_types, cd);
      HIP_TRY(hipMemcpyAsync(ch, cd, sizeof(ch), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      for (int t = 0; t < 4; ++t) disp_counts[t] = (double)ch[t];
      disp_counts_ok = true;
    }
    double e = 0.0;
    for (int p = 0; p < nch; ++p)
      for (int t = 0; t < disp_nt; ++t) {      // (the coefficient as the atoms carry it: rounded to the handle's type)
        const double c = (double)(T)disp_ctab[t][p];
        e += kp[p] * disp_counts[t] * c * c;
      }
    return e;
  }
  double disp_ctab[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  void disp_set_types(int nt, const void* types, const double* ctab) override {
    if (nt <= 0 || !types || !ctab) { disp_nt = 0; disp_types = nullptr; return; }
    ARG_CHECK(nt <= 3, "admp_disp_set_types: at most 3 types");
    disp_nt = nt;
    disp_types = reinterpret_cast<const int*>(types);
    disp_counts_ok = disp_onehot_ok = false;
    for (int t = 0; t < nt; ++t)
      for (int c = 0; c < 3; ++c) disp_ctab[t][c] = ctab[3 * t + c];
  }
  // ADMP_DISP_TYPES=0 / ADMP_DISP_BATCH=0: no typed meshes / the per-channel loop (A/B, tests)
  static bool disp_types_on() { static const bool on = env_flag("ADMP_DISP_TYPES", true); return on; }
  static bool disp_batch_on() { static const bool on = env_flag("ADMP_DISP_BATCH", true); return on; }
  // ---- dispersion PME (admp/disp_pme.py:80-123): real-space pairs + the reciprocal space of every power, by one of the paths
  // of disp_plan.h.  Every path is three legs -- spread, convolve, gather -- with one part function per path and leg;
  // disp_legs is the one place that holds their order, for Engine::disp (all legs) and for the test entries
  // admp_disp_mesh_spread / admp_disp_mesh_gather (one leg, around meshes of the caller's).
  enum { LEG_SPREAD = 1, LEG_CONVOLVE = 2, LEG_GATHER = 4, LEG_ALL = 7 };
  struct DispRun {
    DispPath path = DispPath::PerPower;
    int nch = 1, nmesh = 1, legs = LEG_ALL;
    bool bricks = false, typed = false;
    // the entries' meshes (nmesh x K1 K2 K3 words): written after the spread, read before the gather
    T* mesh_out = nullptr;
    const T* phi_in = nullptr;
    hipMemcpyKind copy = hipMemcpyDeviceToDevice;
  };
  DispRun disp_choose(int pmax, const RecipGeom<T>& g) {
    DispRun run;
    run.nch = (pmax - 4) / 2;
    DispPathIn in;
    in.snranks = snranks; in.use_dft = mc.direct(); in.use_pfa = mc.path() == MeshPath::TwoLevel; in.use_fx = mc.fused_x();
    in.bricks = spread_uses_bricks(top.na, g);
    in.single_precision = sizeof(T) == 4;
    in.nch = run.nch; in.disp_nt = disp_nt; in.have_types = disp_types != nullptr;
    in.types_on = disp_types_on(); in.batch_on = disp_batch_on();
    run.path = disp_path(in);
    run.bricks = run.path == DispPath::BricksTyped || run.path == DispPath::BricksBatched || run.path == DispPath::BricksPerPower;
    run.typed = run.path == DispPath::BricksTyped || run.path == DispPath::DftTyped;
    run.nmesh = run.typed ? disp_nt : run.nch;
    return run;
  }
  size_t disp_nreal() const { return (size_t)K[0] * K[1] * K[2]; }
  void disp_mesh_out(const DispRun& run, int first, int n) {
    if (run.mesh_out)
      HIP_TRY(hipMemcpyAsync(run.mesh_out + first * disp_nreal(), mesh.as<T>() + (run.path == DispPath::PerPower ? 0 : first * disp_nreal()),
                             n * disp_nreal() * sizeof(T), run.copy, stream));
  }
  void disp_phi_in(const DispRun& run, int first, int n) {
    if (run.phi_in)
      HIP_TRY(hipMemcpyAsync(mesh.as<T>() + (run.path == DispPath::PerPower ? 0 : first * disp_nreal()), run.phi_in + first * disp_nreal(),
                             n * disp_nreal() * sizeof(T), run.copy, stream));
  }
  // Brick regime, typed meshes (disp_kernels.hip): nt type meshes through the batched y-z plans, combined per k in the x pass,
  // ONE gather per atom
  void disp_types_check(const ScalarCall& sc, int nch) {
    launch_types_check<T>(stream, top.na, sc.par, 3, disp_types, disp_mix(nch), sc.Ed + E_FMAX);
  }
  void disp_bricks_typed_spread(const ScalarCall& sc, const RecipGeom<T>& g, const ScalarRows& sr, int nch) {
    const int nt = disp_nt;
    ensure_bins(std::max(sr.n, 1));
    disp_types_check(sc, nch);
    mesh.need((size_t)std::max(nt, nch) * nreal_local() * sizeof(T));
    { TIMED("spread"); spread_bricks(sr, g, nt, sc.pos, nullptr, disp_types); }
  }
  void disp_bricks_typed_convolve(const ScalarCall& sc, int nch) {
    const int nt = disp_nt;
    const size_t nspec = 2 * (size_t)K[0] * K[1] * mc.spectrum_pitch();
    mc.need_spectrum((size_t)nt * nspec * sizeof(T));
    const DftTabs<T> tabs = disp_tabs(sc.h, sc.inv, sc.vol, nch);
    mc.convolve_mix(mesh.as<T>(), tabs, disp_mix(nch), nt, nspec, sc.Ed, E_RECIP);
  }
  void disp_bricks_typed_gather(const ScalarCall& sc, const RecipGeom<T>& g, const ScalarRows& sr) {
    TIMED("gather_field");
    launch_gather_scalar<T>(stream, 1, sr.n, sc.pos, sc.par, 3, g, mesh.as<T>(), (long)nreal_local(), sc.dpos, sr.home, 0, disp_types);
  }
  // Brick regime (at scale, and every slab rank): ONE binning and ONE spread of the nch meshes straight from the caller's
  // arrays, no site rows and no scale-add pass.  batched (one rank on a fused-x mesh, round 4): the meshes go through ONE
  // batched r2c, ONE x pass (a G table per power) and ONE batched c2r; then the powers of every mesh point are laid side by
  // side (one streaming pass) and ONE gather fetches them with a single load per stencil point -- the gather is bound by its
  // load instructions (36 per lane and mesh), not by the bytes they return.  Otherwise every power is gathered right after
  // its transform: that gather is bound by the cache-line rate of its 36 mesh loads per lane, whatever it sums (0.175 ms per
  // power at 1M atoms in every form tried: one pass over the three meshes 0.52-0.61 ms; one pass per power from its own or
  // from a shared, cache-resident phi buffer 0.525; round 2's k_gather_field_staged on site rows 0.525).
  void disp_bricks_spread(const ScalarCall& sc, const RecipGeom<T>& g, const ScalarRows& sr, int nch) {
    mesh.need(nch * nreal_local() * sizeof(T));
    ensure_bins(std::max(sr.n, 1));
    { TIMED("spread"); spread_bricks(sr, g, nch, sc.pos, sc.par, nullptr); }
  }
  void disp_bricks_batched_convolve(const ScalarCall& sc, int nch) {
    const size_t nspec = 2 * (size_t)K[0] * K[1] * mc.spectrum_pitch();
    mc.need_spectrum(nch * nspec * sizeof(T));
    const DftTabs<T> tabs = disp_tabs(sc.h, sc.inv, sc.vol, nch);
    mc.convolve_batch(mesh.as<T>(), tabs, nch, nspec, Ed_cur(), E_RECIP);
  }
  void disp_bricks_batched_gather(const ScalarCall& sc, const RecipGeom<T>& g, const ScalarRows& sr, int nch) {
    const size_t nreal = nreal_local();
    mesh2.need(nch * nreal * sizeof(T));
    { TIMED("interleave"); launch_interleave<T>(stream, nch, (long)nreal, mesh.as<T>(), (long)nreal, mesh2.as<T>()); }
    { TIMED("gather_field");
      launch_gather_scalar<T>(stream, nch, sr.n, sc.pos, sc.par, 3, g, mesh2.as<T>(), (long)nreal, sc.dpos, sr.home, 1); }
  }
  void disp_bricks_power_convolve(const ScalarCall& sc, int c) {
    ensure_gtab(sc.h, sc.inv, sc.vol, 6 + 2 * c);
    mc.convolve(mesh.as<T>() + c * nreal_local(), mc.gtab_cur, Ed_cur(), E_RECIP);
  }
  void disp_bricks_power_gather(const ScalarCall& sc, const RecipGeom<T>& g, const ScalarRows& sr, int c) {
    const size_t nreal = nreal_local();
    TIMED("gather_field");
    launch_gather_scalar<T>(stream, 1, sr.n, sc.pos, sc.par + c, 3, g, mesh.as<T>() + c * nreal, (long)nreal, sc.dpos, sr.home);
  }
  void disp_bricks_self(const ScalarCall& sc, const ScalarRows& sr, int nch) {
    TIMED("scalar_self");
    launch_scalar_self<T>(stream, nch, sr.n, sc.par, 3, sr.home, disp_kp().data(), sc.Ed);
  }
  // The other paths go through the spread / gather kernels of the electrostatics: nb batches of charge-only site rows (which
  // also accumulate the self term, disp_pme.py:254-279), their fields, the bins; returns the geometry of their gather
  RecipGeom<T> disp_site_rows(const RecipGeom<T>& g, int nb) {
    const size_t na = (size_t)top.na;
    sites.need(sizeof(Site<T>) * na * nb);
    fld_recip.need(3 * na * sizeof(T) * nb);
    ensure_bins(top.na);
    RecipGeom<T> gj = g;                       // scalar sites: dE/dr = c * Jac . F1 (gather_field applies g.Aop)
    for (int k = 0; k < 9; ++k) gj.Aop[k] = g.Jac[k];
    return gj;
  }
  // the self factors of the site rows: the self term belongs to the spread leg (a gather alone builds its rows without it)
  std::array<double, 3> disp_site_kp(const DispRun& run) const {
    return (run.legs & LEG_SPREAD) ? disp_kp() : std::array<double, 3>{0.0, 0.0, 0.0};
  }
  // Typed meshes on a direct-DFT mesh (small systems; see admp_disp_set_types): the types take the place of the powers in the
  // batch -- one-hot weights through the same site / spread / gather kernels, the x pass combines (dft_kernels.hip k_dft_x_mix)
  void disp_dft_typed_sites(const ScalarCall& sc, const RecipGeom<T>& g, int nch) {
    const int na = top.na, nt = disp_nt;
    launch_types_check<T>(stream, na, sc.par, 3, disp_types, disp_mix(nch), sc.Ed + E_FMAX);
    mesh.need(nt * disp_nreal() * sizeof(T));
    onehot_d.need((size_t)na * nt * sizeof(T));
    bases_d.need(sizeof(int4) * (size_t)na);
    const double no_self[3] = {0.0, 0.0, 0.0};
    TIMED("scalar_sites");
    if (!disp_onehot_ok || onehot_for != onehot_d.p) {
      launch_onehot<T>(stream, na, nt, disp_types, onehot_d.as<T>());
      disp_onehot_ok = true; onehot_for = onehot_d.p;
    }
    launch_scalar_sites_batch<T>(stream, na, sc.pos, onehot_d.as<T>(), nt, nt, no_self, sites.as<Site<T>>(), sc.Ed, &g,
                                 bases_d.as<int4>());
  }
  void disp_dft_typed_spread(const RecipGeom<T>& g) {
    TIMED("spread");
    spread_sites(top.na, sites.as<Site<T>>(), 0, g, mesh.as<T>(), bases_d.as<int4>(), disp_nt);
  }
  void disp_dft_typed_convolve(const ScalarCall& sc, int nch) {
    const int nt = disp_nt;
    const size_t nspec = 2 * (size_t)K[0] * K[1] * (K[2] / 2 + 1);
    mc.need_spectrum(nt * nspec * sizeof(T));
    const DftTabs<T> tabs = disp_tabs(sc.h, sc.inv, sc.vol, nch);
    const MixTab mix = disp_mix(nch);
    mc.convolve_dft_batch(mesh.as<T>(), tabs, nt, disp_nreal(), nspec, Ed_cur(), E_RECIP, &mix);
  }
  void disp_dft_typed_gather(const ScalarCall& sc, const RecipGeom<T>& gj) {
    const int na = top.na, nt = disp_nt;
    { TIMED("gather_field"); launch_gather_field<T>(stream, na, sites.as<Site<T>>(), gj, mesh.as<T>(), fld_recip.as<T>(), nullptr, nt); }
    { TIMED("scale_add"); launch_scale_add<T>(stream, na, onehot_d.as<T>(), nt, 0, fld_recip.as<T>(), sc.dpos, nt); }
  }
  // direct-DFT meshes are small and dispatch bound: the powers are spread into separate meshes and transformed as ONE batch
  // (5 launches instead of 5 per power), then one gather over the batch of meshes.  The scan-spread regime takes the powers
  // as a batch: the stencil records ride along, every (brick, power) workgroup of the scan spread reads them instead of
  // redoing three grid_ref per atom (3072 atoms x 1029 workgroups at 97^3); the brick regime spreads power by power.
  void disp_dft_batched_sites(const DispRun& run, const ScalarCall& sc, const RecipGeom<T>& g) {
    bases_d.need(sizeof(int4) * (size_t)top.na);
    TIMED("scalar_sites");
    launch_scalar_sites_batch<T>(stream, top.na, sc.pos, sc.par, 3, run.nch, disp_site_kp(run).data(), sites.as<Site<T>>(), sc.Ed, &g,
                                 bases_d.as<int4>());
  }
  void disp_dft_batched_spread(const DispRun& run, const RecipGeom<T>& g) {
    TIMED("spread");
    spread_sites(top.na, sites.as<Site<T>>(), 0, g, mesh.as<T>(), bases_d.as<int4>(), run.nch);
  }
  void disp_dft_batched_convolve(const ScalarCall& sc, int nch) {
    const size_t nspec = 2 * (size_t)K[0] * K[1] * mc.spectrum_columns();
    mc.need_spectrum(nch * nspec * sizeof(T));
    const DftTabs<T> tabs = disp_tabs(sc.h, sc.inv, sc.vol, nch);
    mc.convolve_dft_batch(mesh.as<T>(), tabs, nch, disp_nreal(), nspec, Ed_cur(), E_RECIP);
  }
  // the site rows hold the positions (only the charge slot differs per power): one gather over the batch of meshes
  void disp_dft_batched_gather(const ScalarCall& sc, const RecipGeom<T>& gj, int nch) {
    const int na = top.na;
    { TIMED("gather_field"); launch_gather_field<T>(stream, na, sites.as<Site<T>>(), gj, mesh.as<T>(), fld_recip.as<T>(), nullptr, nch); }
    { TIMED("scale_add"); launch_scale_add<T>(stream, na, sc.par, 3, 0, fld_recip.as<T>(), sc.dpos, nch); }
  }
  // one scalar reciprocal pass per power: the power is packed into site rows, spread, convolved, gathered, scaled
  void disp_power_sites(const DispRun& run, const ScalarCall& sc, int c) {
    TIMED("scalar_sites");
    launch_scalar_sites<T>(stream, top.na, sc.pos, sc.par, 3, c, disp_site_kp(run)[c], sites.as<Site<T>>(), sc.Ed);
  }
  void disp_power_spread(const RecipGeom<T>& g, T* mesh_p, int c) {
    TIMED("spread");
    spread_sites(top.na, sites.as<Site<T>>(), 0, g, mesh_p, nullptr, 1, c > 0);
  }
  void disp_power_convolve(const ScalarCall& sc, int c) {
    ensure_gtab(sc.h, sc.inv, sc.vol, 6 + 2 * c);
    mc.convolve(mesh.as<T>(), mc.gtab_cur, Ed_cur(), E_RECIP);
  }
  void disp_power_gather(const ScalarCall& sc, const RecipGeom<T>& gj, int c) {
    const int na = top.na;
    { TIMED("gather_field"); launch_gather_field<T>(stream, na, sites.as<Site<T>>(), gj, mesh.as<T>(), fld_recip.as<T>(), nullptr); }
    { TIMED("scale_add"); launch_scale_add<T>(stream, na, sc.par, 3, c, fld_recip.as<T>(), sc.dpos); }
  }
  // the legs of run.legs in the order of the path.  The site rows of the site-row paths belong to both outer legs (the gather
  // reads the positions from them).
  void disp_legs(const DispRun& run, const ScalarCall& sc, const RecipGeom<T>& g, const ScalarRows& sr) {
    const int nch = run.nch;
    const bool S = run.legs & LEG_SPREAD, C = run.legs & LEG_CONVOLVE, G = run.legs & LEG_GATHER;
    switch (run.path) {
      case DispPath::BricksTyped:
        if (S) { disp_bricks_typed_spread(sc, g, sr, nch); disp_mesh_out(run, 0, run.nmesh); }
        if (C) disp_bricks_typed_convolve(sc, nch);
        if (G) {
          // a gather alone: the kernel picks its mesh by the type index, so the table is checked, and refused, before it runs
          if (!S) { disp_types_check(sc, nch); double E3[3]; read_scalar_energies(sc.Ed, E3, 3, true); }
          disp_phi_in(run, 0, run.nmesh); disp_bricks_typed_gather(sc, g, sr);
        }
        break;
      case DispPath::BricksBatched:
        if (S) { disp_bricks_spread(sc, g, sr, nch); disp_mesh_out(run, 0, nch); }
        if (C) disp_bricks_batched_convolve(sc, nch);
        if (G) { disp_phi_in(run, 0, nch); disp_bricks_batched_gather(sc, g, sr, nch); disp_bricks_self(sc, sr, nch); }
        break;
      case DispPath::BricksPerPower:
        if (S) { disp_bricks_spread(sc, g, sr, nch); disp_mesh_out(run, 0, nch); }
        if (G) disp_phi_in(run, 0, nch);
        for (int c = 0; c < nch; ++c) {
          if (C) disp_bricks_power_convolve(sc, c);
          if (G) disp_bricks_power_gather(sc, g, sr, c);
        }
        if (G) disp_bricks_self(sc, sr, nch);
        break;
      case DispPath::DftTyped: {
        const RecipGeom<T> gj = disp_site_rows(g, disp_nt);
        if (S || G) disp_dft_typed_sites(sc, g, nch);
        if (S) { disp_dft_typed_spread(g); disp_mesh_out(run, 0, run.nmesh); }
        if (C) disp_dft_typed_convolve(sc, nch);
        if (G) { disp_phi_in(run, 0, run.nmesh); disp_dft_typed_gather(sc, gj); }
        break;
      }
      case DispPath::DftBatched: {
        const RecipGeom<T> gj = disp_site_rows(g, nch);
        mesh.need(nch * disp_nreal() * sizeof(T));
        if (!spread_uses_bricks(top.na, g)) {
          if (S || G) disp_dft_batched_sites(run, sc, g);
          if (S) disp_dft_batched_spread(run, g);
        } else {
          for (int c = 0; c < nch; ++c) {      // (the rows of the last power stay: the gather reads their positions)
            if (S || (G && c == nch - 1)) disp_power_sites(run, sc, c);
            if (S) disp_power_spread(g, mesh.as<T>() + c * disp_nreal(), c);
          }
        }
        if (S) disp_mesh_out(run, 0, nch);
        if (C) disp_dft_batched_convolve(sc, nch);
        if (G) { disp_phi_in(run, 0, nch); disp_dft_batched_gather(sc, gj, nch); }
        break;
      }
      case DispPath::PerPower: {
        const RecipGeom<T> gj = disp_site_rows(g, 1);
        for (int c = 0; c < nch; ++c) {
          if (S || G) disp_power_sites(run, sc, c);
          if (S) { disp_power_spread(g, mesh.as<T>(), c); disp_mesh_out(run, c, 1); }
          if (C) disp_power_convolve(sc, c);
          if (G) { disp_phi_in(run, c, 1); disp_power_gather(sc, gj, c); }
        }
        break;
      }
    }
  }
  void disp(const void* pos_, const double* box, const void* clist_, int pmax, int ns, const double* mS, double* E,
            void* dpos_, int on_device) override {
    ARG_CHECK(have_top && have_ewald && pl.have(), "topology, ewald parameters and pairs must be set first");
    ARG_CHECK(snranks == 1 || on_device, "a slab-decomposed handle takes device pointers");
    ARG_CHECK(pos_ && box && clist_ && E, "null argument");
    ARG_CHECK(pmax == 6 || pmax == 8 || pmax == 10, "pmax must be 6, 8 or 10");
    const int na = top.na;
    HIP_TRY(hipSetDevice(device));
    RecipGeom<T> g;
    const ScalarCall sc = scalar_begin(box, ns, mS, pos_, clist_, 3, dpos_, on_device, E_WORDS, &g);
    cls_sites_na = slab_sites_na = -1;   // other rows than an electrostatics evaluation's
    const DispRun run = disp_choose(pmax, g);
    if (snranks > 1) ARG_CHECK(spread_uses_bricks(1 << 30, g), "slab-decomposed dispersion PME needs at least 17 local mesh planes and K2, K3 >= 17");
    const ScalarRows sr = scalar_rows(sc.pos, g, K[0], mc.X0, mc.X1, run.bricks);
    { TIMED("disp_pair"); launch_disp_pair<T>(stream, na, pl.table(), pack_srows(sc.pos, sc.par, 3), sc.bx, sc.tab, (T)kappa, pmax, sc.dpos, sc.Ed, sr.rows, sr.n, cutoff); }
    disp_legs(run, sc, g, sr);
    // the energies: a typed path takes its self term from the type table, and its read refuses a table that does not describe
    // c_list; the brick paths and the typed ones read through the sum over the ranks
    if (run.bricks || run.typed) {
      const double e_self = run.typed ? typed_self_energy(na, run.nch, disp_kp().data()) : 0.0;
      read_scalar_energies(sc.Ed, E, 3, run.typed);
      if (run.typed) E[2] = e_self;
      scalar_return_grad(sc, dpos_, on_device);
    } else {
      double Eh[E_SLOTS];
      HIP_TRY(hipMemcpyAsync(Eh, sc.Ed, sizeof(Eh), hipMemcpyDeviceToHost, stream));
      scalar_return_grad(sc, dpos_, on_device, false);
      HIP_TRY(hipStreamSynchronize(stream));
      E[0] = Eh[E_REAL]; E[1] = Eh[E_RECIP]; E[2] = Eh[E_SELF];
    }
  }
  // admp_disp_mesh_spread / admp_disp_mesh_gather: one leg of a dispersion call alone, on the path the call would take
  // (tests compare the mesh words and the gradient rows with a float64 reference).  Nothing of the real-space chain runs.
  struct DispLegCall { ScalarCall sc; RecipGeom<T> g; DispRun run; ScalarRows sr; };
  DispLegCall disp_leg_begin(const void* pos_, const double* box, const void* clist_, int pmax, int on_device,
                             int legs) {
    ARG_CHECK(K[0] >= 6 && K[1] >= 6 && K[2] >= 6, "PME mesh must be at least 6 points per dimension (order-6 splines)");
    HIP_TRY(hipSetDevice(device));
    static const double one[1] = {1.0};
    DispLegCall lc;
    lc.sc = scalar_begin(box, 1, one, pos_, clist_, 3, nullptr, on_device, E_WORDS, &lc.g);
    cls_sites_na = slab_sites_na = -1;
    lc.run = disp_choose(pmax, lc.g);
    lc.run.legs = legs;
    lc.run.copy = on_device ? hipMemcpyDeviceToDevice : (legs == LEG_SPREAD ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice);
    lc.sr = scalar_rows(lc.sc.pos, lc.g, K[0], mc.X0, mc.X1, lc.run.bricks && legs == LEG_SPREAD);
    return lc;
  }
  void disp_leg_info(const DispLegCall& lc, int32_t* info, int main_groups) {
    const int dims[3] = {nloc0(), K[1], K[2]};
    int c[4];
    spread_launch_choice(top.na, dims, c);
    info[0] = (int)lc.run.path; info[1] = lc.run.nmesh; info[2] = lc.run.typed ? 1 : 0;
    for (int d = 0; d < 3; ++d) info[3 + d] = c[1 + d];
    info[6] = main_groups;
    info[7] = lc.run.bricks ? -1 : c[0];
  }
  void disp_mesh_spread(const void* pos_, const double* box, const void* clist_, int pmax, int on_device, void* mesh_out,
                        double* E_self_out, int32_t* info) override {
    if (snranks != 1) throw Err{ADMP_E_ARG, "admp_disp_mesh_spread works on a single rank only (slab-decomposed handle)"};
    ARG_CHECK(have_top && have_ewald && pl.have(), "topology, ewald parameters and pairs must be set first");
    ARG_CHECK(pos_ && box && clist_ && mesh_out && E_self_out && info, "null argument");
    ARG_CHECK(pmax == 6 || pmax == 8 || pmax == 10, "pmax must be 6, 8 or 10");
    DispLegCall lc = disp_leg_begin(pos_, box, clist_, pmax, on_device, LEG_SPREAD);
    lc.run.mesh_out = reinterpret_cast<T*>(mesh_out);
    disp_legs(lc.run, lc.sc, lc.g, lc.sr);
    double E[3];
    read_scalar_energies(lc.sc.Ed, E, 3, lc.run.typed);
    *E_self_out = E[2];
    // workgroups of the spread: the brick paths' launcher says; the site-row paths go through the electrostatics launcher
    const int dims[3] = {nloc0(), K[1], K[2]};
    const int groups = lc.run.bricks ? disp_spread_groups(dims) : -1;
    disp_leg_info(lc, info, groups);
  }
  void disp_mesh_gather(const void* pos_, const double* box, const void* clist_, int pmax, const void* phi_, int which,
                        int on_device, double* E_self_out, void* out_, int32_t* info) override {
    if (snranks != 1) throw Err{ADMP_E_ARG, "admp_disp_mesh_gather works on a single rank only (slab-decomposed handle)"};
    ARG_CHECK(have_top && have_ewald && pl.have(), "topology, ewald parameters and pairs must be set first");
    ARG_CHECK(pos_ && box && clist_ && phi_ && E_self_out && out_ && info, "null argument");
    ARG_CHECK(pmax == 6 || pmax == 8 || pmax == 10, "pmax must be 6, 8 or 10");
    ARG_CHECK(which == 0 || which == 1, "which must be 0 (the gradient gather) or 1 (the value gather of the parameter gradient)");
    DispLegCall lc = disp_leg_begin(pos_, box, clist_, pmax, on_device, LEG_GATHER);
    const size_t na = (size_t)top.na, nreal = disp_nreal();
    const T* phi = reinterpret_cast<const T*>(phi_);
    s_out.need(3 * na * sizeof(T));
    T* out = on_device ? reinterpret_cast<T*>(out_) : s_out.as<T>();
    HIP_TRY(hipMemsetAsync(out, 0, 3 * na * sizeof(T), stream));
    double E[3] = {0.0, 0.0, 0.0};
    int groups;
    if (which == 0) {
      lc.sc.dpos = out;
      lc.run.phi_in = phi;
      mesh.need((size_t)std::max(lc.run.nmesh, lc.run.nch) * nreal * sizeof(T));
      disp_legs(lc.run, lc.sc, lc.g, lc.sr);
      const double e_self = lc.run.typed ? typed_self_energy(top.na, lc.run.nch, disp_kp().data()) : 0.0;
      read_scalar_energies(lc.sc.Ed, E, 3, lc.run.typed);
      *E_self_out = lc.run.typed ? e_self : E[2];
      groups = lc.run.bricks ? (int)disp_gather_groups(top.na) : -1;
    } else {
      const std::array<double, 3> kp = disp_kp();
      if (!on_device) {
        mesh.need((size_t)lc.run.nch * nreal * sizeof(T));
        HIP_TRY(hipMemcpyAsync(mesh.p, phi_, (size_t)lc.run.nch * nreal * sizeof(T), hipMemcpyHostToDevice, stream));
        phi = mesh.as<T>();
      }
      for (int c = 0; c < lc.run.nch; ++c) disp_pgrad_gather(lc.sc.pos, lc.sc.par, lc.g, phi + c * nreal, c, kp[c], out);
      HIP_TRY(hipStreamSynchronize(stream));
      *E_self_out = 0.0;
      groups = disp_value_groups(top.na);
    }
    if (!on_device) {
      HIP_TRY(hipMemcpyAsync(out_, out, 3 * na * sizeof(T), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
    }
    disp_leg_info(lc, info, groups);
    if (which == 1) info[1] = lc.run.nch, info[2] = 0;
  }
  // the mesh part of the parameter gradient of power c: the potential of its mesh at the atoms + the self term's 2 kp c
  void disp_pgrad_gather(const T* pos, const T* cl, const RecipGeom<T>& g, const T* phi, int c, double kp, T* out) {
    launch_gather_value<T>(stream, top.na, pos, cl, 3, c, g, phi, 2.0 * kp, out);
  }

  void tt(const void* pos_, const double* box, const void* abqc_, int ns, const double* mS, double* E, void* dpos_,
          int on_device) override {
    ARG_CHECK(have_top && pl.have(), "topology and pairs must be set first");
    ARG_CHECK(snranks == 1 || on_device, "a slab-decomposed handle takes device pointers");
    ARG_CHECK(pos_ && box && abqc_ && E, "null argument");
    const int na = top.na;
    HIP_TRY(hipSetDevice(device));
    const ScalarCall sc = scalar_begin(box, ns, mS, pos_, abqc_, 4, dpos_, on_device, E_WORDS);
    ScalarRows sr{nullptr, na, nullptr};
    if (snranks > 1) sr = virtual_slab_rows(sc.pos, sc.inv);
    { TIMED("tt_pair"); launch_tt_pair<T>(stream, na, pl.table(), pack_srows(sc.pos, sc.par, 4), sc.bx, sc.tab, sc.dpos, sc.Ed, sr.rows, sr.n, cutoff); }
    read_scalar_energies(sc.Ed, E, 1);
    scalar_return_grad(sc, dpos_, on_device);
  }

  // dE/dc_list (Na,3) of the dispersion PME energy (real + reciprocal + self; admp/disp_pme.py:80-123): the pair part is a
  // per-atom sum of (m + g_p - 1) c_j / r^p, the reciprocal part the mesh potential of every channel at the atom (E_recip is
  // a quadratic form of the channel's coefficients), the self part 2 kp c.  Device pointers; on request only.
  void disp_param_grad(const void* pos_, const double* box, const void* clist_, int pmax, int ns, const double* mS,
                       void* out_) override {
    ARG_CHECK(have_top && have_ewald && pl.have(), "topology, ewald parameters and pairs must be set first");
    ARG_CHECK(pos_ && box && clist_ && out_, "null argument");
    ARG_CHECK(pmax == 6 || pmax == 8 || pmax == 10, "pmax must be 6, 8 or 10");
    const int na = top.na;
    double inv[9], vol;
    Box<T> bx = make_box(box, inv, &vol);
    ensure_mesh();
    RecipGeom<T> g = make_geom(inv);
    ScaleTab<T> tab = make_tab(ns, mS, nullptr);
    const T* pos = reinterpret_cast<const T*>(pos_);
    const T* cl = reinterpret_cast<const T*>(clist_);
    T* out = reinterpret_cast<T*>(out_);
    energies_d.need(2 * E_WORDS * sizeof(double));
    ehalf = 0; other_clean = false;
    double* Ed = energies_d.as<double>();
    HIP_TRY(hipMemsetAsync(Ed, 0, E_WORDS * sizeof(double), stream));
    HIP_TRY(hipMemsetAsync(out, 0, 3 * (size_t)na * sizeof(T), stream));
    const std::array<double, 3> kp = disp_kp();
    const int nch = (pmax - 4) / 2;
    if (snranks > 1) {      // slab rank (round 4): pair sums over its home rows, the channels' mesh potentials at its home atoms
      ARG_CHECK(spread_uses_bricks(1 << 30, g), "slab-decomposed dispersion PME needs at least 17 local mesh planes and K2, K3 >= 17");
      cls_sites_na = slab_sites_na = -1;
      const ScalarRows sr = scalar_rows(pos, g, K[0], mc.X0, mc.X1, true);
      launch_scalar_pair_pgrad<T>(stream, 0, na, pl.table(), pos, cl, bx, tab, (T)kappa, pmax, out, cutoff, sr.rows, sr.n);
      const size_t nreal = nreal_local();
      mesh.need(nch * nreal * sizeof(T));
      ensure_bins(std::max(sr.n, 1));
      spread_bricks(sr, g, nch, pos, cl, nullptr);
      for (int c = 0; c < nch; ++c) {
        ensure_gtab(box, inv, vol, 6 + 2 * c);
        mc.convolve(mesh.as<T>() + c * nreal, mc.gtab_cur, Ed_cur(), E_RECIP);
        launch_gather_value<T>(stream, sr.n, pos, cl, 3, c, g, mesh.as<T>() + c * nreal, 2.0 * kp[c], out, sr.home);
      }
      HIP_TRY(hipStreamSynchronize(stream));
      return;
    }
    launch_scalar_pair_pgrad<T>(stream, 0, na, pl.table(), pos, cl, bx, tab, (T)kappa, pmax, out, cutoff);
    cls_sites_na = slab_sites_na = -1;
    sites.need(sizeof(Site<T>) * (size_t)na);
    ensure_bins(na);
    for (int c = 0; c < nch; ++c) {
      ensure_gtab(box, inv, vol, 6 + 2 * c);
      launch_scalar_sites<T>(stream, na, pos, cl, 3, c, kp[c], sites.as<Site<T>>(), Ed);
      spread_sites(na, sites.as<Site<T>>(), 0, g, mesh.as<T>(), nullptr, 1, c > 0);
      mc.convolve(mesh.as<T>(), mc.gtab_cur, Ed_cur(), E_RECIP);
      disp_pgrad_gather(pos, cl, g, mesh.as<T>(), c, kp[c], out);
    }
    HIP_TRY(hipStreamSynchronize(stream));
  }
  // dE/d(a, b, q, c6) (Na,4) of the Tang-Toennies pair term (admp/pairwise.py:94-113).  Device pointers; on request only.
  void tt_param_grad(const void* pos_, const double* box, const void* abqc_, int ns, const double* mS, void* out_) override {
    ARG_CHECK(have_top && pl.have(), "topology and pairs must be set first");
    ARG_CHECK(pos_ && box && abqc_ && out_, "null argument");
    double inv[9], vol;
    Box<T> bx = make_box(box, inv, &vol);
    ScaleTab<T> tab = make_tab(ns, mS, nullptr);
    const T* pos = reinterpret_cast<const T*>(pos_);
    ScalarRows sr{nullptr, top.na, nullptr};
    if (snranks > 1) sr = virtual_slab_rows(pos, inv);      // (per-atom outputs: the home rows are this rank's results)
    launch_scalar_pair_pgrad<T>(stream, 1, top.na, pl.table(), pos, reinterpret_cast<const T*>(abqc_), bx,
                                tab, T(0), 0, reinterpret_cast<T*>(out_), cutoff, sr.rows, sr.n);
    HIP_TRY(hipStreamSynchronize(stream));
  }

  // a traced pair kernel (pair_program_build) on the current neighbour table: admp/pairwise.py:67-91 with any kernel
  DevBuf prog_consts;
  void pair_program_eval(int id, const void* pos_, const double* box, const void* par_, int ns, const double* mS, double* E,
                         void* dpos_, int on_device) override {
    ARG_CHECK(have_top && pl.have(), "topology and pairs must be set first");
    ARG_CHECK(id >= 0 && id < (int)programs.size(), "unknown pair program");
    ARG_CHECK(pos_ && box && E && ns >= 1 && mS, "null argument");
    const PairProgram& pg = programs[id];
    ARG_CHECK(pg.n_params == 0 || par_, "atomic parameters missing");
    const int na = top.na;
    // (the program reads the scales themselves, below: the record's table goes unused)
    const ScalarCall sc = scalar_begin(box, ns, mS, pos_, pg.n_params ? par_ : nullptr, (size_t)pg.n_params, dpos_, on_device, E_SLOTS);
    const T* pos = sc.pos; const T* par = sc.par;
    T* dpos = sc.dpos;
    double* Ed = sc.Ed;
    T consts[34];                                   // box (9), box^-1 (9), mscale per covalent class (16)
    for (int k = 0; k < 9; ++k) { consts[k] = (T)box[k]; consts[9 + k] = (T)sc.inv[k]; }
    for (int nb = 0; nb < 16; ++nb) consts[18 + nb] = (T)mS[((nb - 1) % ns + ns) % ns];      // admp/pme.py:681-683 wrap
    prog_consts.need(sizeof(consts));
    HIP_TRY(hipMemcpyAsync(prog_consts.p, consts, sizeof(consts), hipMemcpyHostToDevice, stream));
    const T* boxd = prog_consts.as<T>();
    const T* mtab = boxd + 18;
    int na_arg = na;
    const int* rowptr = pl.table().rowptr; const int* colp = pl.table().col; const int* order = pl.table().order;
    T* gradp = dpos_ ? dpos : nullptr;
    double* eptr = Ed + E_REAL;
    void* args[] = {&na_arg, &rowptr, &colp, &order, &pos, &par, &boxd, &mtab, &gradp, &eptr};
    const unsigned grid = (unsigned)(((long)na * 8 + 255) / 256);
    {
      TIMED("pair_custom");
      HIP_TRY(hipModuleLaunchKernel(pg.fn, grid, 1, 1, 256, 1, 1, 0, stream, args, nullptr));
    }
    double Eh2[E_SLOTS];
    HIP_TRY(hipMemcpyAsync(Eh2, Ed, sizeof(Eh2), hipMemcpyDeviceToHost, stream));
    scalar_return_grad(sc, dpos_, on_device, false);
    HIP_TRY(hipStreamSynchronize(stream));
    E[0] = Eh2[E_REAL];
  }

  // raw per-atom sums behind dE/dpol and dE/dtholes (device pointers only); the caller finishes them (admp_amd/pme.py)
  void thole_sums(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, int ns,
                  const double* mS, const double* pS, const void* U, void* sumX, void* sumXw) override {
    ARG_CHECK(lpol, "polarizable handle required");
    ARG_CHECK(sumX && sumXw && U, "null argument");
    HIP_TRY(hipSetDevice(device));
    stage_begin(pos, box, Ql, pol, thole, ns, mS, pS, const_cast<void*>(U));
    // (slab rank: the sums of its home rows -- per-atom outputs like the gradient: the home rows are this rank's results)
    { TIMED("thole_sums"); launch_thole_sums<T>(stream, top.na, wnbr(), sites.as<Site<T>>(), ev.bx, ev.tab, (T*)sumX, (T*)sumXw,
                                                snranks > 1 ? pair_rows() : nullptr, ev.n_home); }
    ev.active = false;
    HIP_TRY(hipStreamSynchronize(stream));
  }

  // admp_pair_real: one real-space pair kernel and its raw rows -- what an evaluation does up to that kernel (stage_begin:
  // sites, classes, cut table) and the kernel through the evaluation's own launcher, nothing of the mesh chain and no SCF
  // (tests compare the rows with a float64 reference).  which 0: k_pair_full (flags bit 0: the charge-only forms are allowed,
  // as in a call without dE/dQ_local), 1: k_pair_field over the polarizable rows (the other rows of fld come back zero),
  // 2: k_pair_field_ind after the SCF's own Jacobi step on the field F (dU = -pol F / DIELECTRIC in the site rows), over the
  // SCF's sub-table and sorted list of polarizable sites: fld = the increment alone.
  void pair_real(const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_, int ns,
                 const double* mS, const double* pS, const void* U_, const void* F_, int which, int flags, int on_device,
                 double* E_out, void* grad_, void* pot_, void* fld_, int32_t* info) override {
    ARG_CHECK(snranks == 1, "admp_pair_real works on a single rank only (slab-decomposed handle)");
    ARG_CHECK(have_top && have_ewald && pl.have(), "topology, ewald parameters and pairs must be set first");
    ARG_CHECK(which >= 0 && which <= 2, "which must be 0 (closing pair kernel), 1 (SCF field kernel) or 2 (its increment)");
    ARG_CHECK(which == 0 || lpol, "the field kernels need a polarizable handle");
    ARG_CHECK(pos_ && box && Ql_ && E_out && info, "null argument");
    if (lpol) ARG_CHECK(pol_ && thole_ && U_ && pS, "polarizable handle needs pol, tholes, pScales and U");
    if (which == 0) ARG_CHECK(grad_ && pot_ && (!lpol || fld_), "null output");
    else ARG_CHECK(fld_ != nullptr, "null output");
    if (which == 2) ARG_CHECK(F_ != nullptr, "the increment needs the field of its Jacobi step");
    const size_t na = (size_t)top.na;
    HIP_TRY(hipSetDevice(device));
    U_src_now = nullptr;
    const T* pos = stage_in(s_pos, pos_, 3 * na, on_device);
    const T* Ql = stage_in(s_Q, Ql_, 9 * na, on_device);
    const T* pol = lpol ? stage_in(s_pol, pol_, na, on_device) : nullptr;
    const T* thole = lpol ? stage_in(s_thole, thole_, na, on_device) : nullptr;
    const T* U = lpol ? stage_in(s_U, U_, 3 * na, on_device) : nullptr;
    if (which == 2 && on_device) {      // the Jacobi step updates the dipoles in place: in a copy, the caller's are an input
      s_U.need(3 * na * sizeof(T));
      HIP_TRY(hipMemcpyAsync(s_U.p, U_, 3 * na * sizeof(T), hipMemcpyDeviceToDevice, stream));
      U = s_U.as<T>();
    }
    grad.need(3 * na * sizeof(T));
    if (which == 0) mono_ok = (flags & 1) != 0;
    stage_begin(pos, box, Ql, pol, thole, ns, mS, pS, const_cast<T*>(U));
    int n_rows = ev.n_home;
    double E[4];
    if (which == 0) {
      stage_pair_full(grad.as<T>(), lpol ? fld_pair.as<T>() : nullptr);
    } else if (which == 1) {
      HIP_TRY(hipMemsetAsync(fld_pair.p, 0, 3 * na * sizeof(T), stream));
      n_rows = nact_rows();
      first_pair_field();
    } else {
      read_energies(E_RECIP, E, false);      // the count of polarizable sites, as the SCF's first check reads it
      nact_seen();
      n_rows = nact_known();
      HIP_TRY(hipMemcpyAsync(field.p, F_, 3 * na * sizeof(T), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
      HIP_TRY(hipMemsetAsync(fld_pair.p, 0, 3 * na * sizeof(T), stream));
      ensure_ind_table();      // the sub-table, as scf_increment keeps it
      scf_jacobi(n_rows);
      if (n_rows > 0) { TIMED("pair_field_ind"); launch_pair_field_ind<T>(stream, pair_field_ind_args(n_rows)); }
    }
    ev.active = false;
    read_energies(E_RECIP, E);      // (one synchronisation; the class flags of this call reach the pair list as in an evaluation)
    nact_seen();
    int w[2];
    std::memcpy(w, &Eh[E_NACT], sizeof(w));
    *E_out = which == 0 ? E[0] : 0.0;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (which == 0) {
      HIP_TRY(hipMemcpyAsync(grad_, grad.p, 3 * na * sizeof(T), kind, stream));
      HIP_TRY(hipMemcpyAsync(pot_, pot.p, 9 * na * sizeof(T), kind, stream));
    }
    if (lpol && fld_) HIP_TRY(hipMemcpyAsync(fld_, fld_pair.p, 3 * na * sizeof(T), kind, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    int c[4];
    pair_launch_choice(which, n_rows, lpol, sizeof(T), c);
    info[0] = c[0];
    info[1] = cut_on ? 1 : 0;
    info[2] = (which < 2 && (which == 0 ? mono_ok : true) && c[2] && rq_d.p && !(w[1] & CLS_STALE)) ? 1 : 0;
    info[3] = c[3];
    scf.forget();
  }

  // admp_mesh_spread / admp_mesh_gather: the spread or the gather alone -- what an evaluation does up to that kernel
  // (stage_begin: sites at the dipoles given, stencil records, the list of polarizable sites) and the kernel through the
  // evaluation's own launcher (tests compare the mesh words and the rows with a float64 reference).  The scale tables of the
  // pair kernels are not an input here: nothing of the real-space chain runs.
  struct MeshIn { const T *pos, *Ql, *pol, *thole, *U; };
  MeshIn mesh_stage(const char* who, const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_,
                    const void* U_, int on_device) {
    if (snranks != 1) throw Err{ADMP_E_ARG, std::string(who) + " works on a single rank only (slab-decomposed handle)"};
    ARG_CHECK(have_top && have_ewald && pl.have(), "topology, ewald parameters and pairs must be set first");
    ARG_CHECK(pos_ && box && Ql_, "null argument");
    if (lpol) ARG_CHECK(pol_ && thole_ && U_, "polarizable handle needs pol, tholes and U");
    const size_t na = (size_t)top.na;
    HIP_TRY(hipSetDevice(device));
    U_src_now = nullptr;
    MeshIn in;
    in.pos = stage_in(s_pos, pos_, 3 * na, on_device);
    in.Ql = stage_in(s_Q, Ql_, 9 * na, on_device);
    in.pol = lpol ? stage_in(s_pol, pol_, na, on_device) : nullptr;
    in.thole = lpol ? stage_in(s_thole, thole_, na, on_device) : nullptr;
    in.U = lpol ? stage_in(s_U, U_, 3 * na, on_device) : nullptr;
    return in;
  }
  void mesh_begin(const MeshIn& in, const double* box) {
    static const double one[1] = {1.0};
    stage_begin(in.pos, box, in.Ql, in.pol, in.thole, 1, one, one, const_cast<T*>(in.U));
  }
  void mesh_spread(const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_, const void* U_,
                   int which, int flags, int on_device, void* mesh_out, int32_t* info) override {
    const MeshIn in = mesh_stage("admp_mesh_spread", pos_, box, Ql_, pol_, thole_, U_, on_device);
    ARG_CHECK(which == 0 || which == 1, "which must be 0 (the spread kernels) or 1 (the forward plane kernel)");
    ARG_CHECK(mesh_out && info, "null argument");
    ARG_CHECK(K[0] >= 6 && K[1] >= 6 && K[2] >= 6, "PME mesh must be at least 6 points per dimension (order-6 splines)");
    ensure_mesh();
    if (which == 1)
      ARG_CHECK(mc.direct() && dft_zy_spread_fits<T>(K, top.na),
                "which = 1: this handle's evaluations do not spread in the forward plane kernel (type, atom count or mesh path)");
    mesh_begin(in, box);
    const size_t nreal = (size_t)K[0] * K[1] * K[2];
    T* m = on_device ? reinterpret_cast<T*>(mesh_out) : mesh.as<T>();
    const int4* recs = (flags & 2) ? nullptr : ev.bases;
    const int tight = (flags & 1) ? 1 : 0;
    const int dims[3] = {nloc0(), K[1], K[2]};
    int c[4];
    spread_launch_choice(ev.n_home, dims, c);
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[5] = -1;
    if (which == 0) {
      TIMED("spread");
      int rc = launch_spread<T>(stream, ev.n_home, sites.as<Site<T>>(), lpol, ev.g, bins, m, ev.home, recs, 1, 0, tight);
      if (rc != 0) throw Err{ADMP_E_HIP, std::string("launch_spread: ") + hipGetErrorString((hipError_t)rc)};
      info[0] = c[0];
      info[4] = (c[0] == ADMP_SPREAD_FORM_BRICKS && sizeof(T) == 4 && tight) ? 1 : 0;
    } else {
      ARG_CHECK(spread_fused(ev.n_home), "internal: plane spread refused after the sites were prepared");
      HIP_TRY(hipMemsetAsync(Ed_cur() + E_RECIP, 0, sizeof(double), stream));
      slot_clean[E_RECIP] = false;
      const PlaneSpread<T> sp = plane_spread(ev.n_home, sites.as<Site<T>>(), lpol, recs);
      mc.convolve(m, mc.gtab_cur, Ed_cur(), E_RECIP, nullptr, nullptr, &sp);
      info[0] = ADMP_SPREAD_FORM_PLANE_KERNEL;
      info[5] = mc.path_word();      // the handle's path, as admp_mesh_convolve reports it
    }
    for (int d = 0; d < 3; ++d) info[1 + d] = c[1 + d];
    info[6] = recs ? 1 : 0;
    ev.active = false;
    if (!on_device) HIP_TRY(hipMemcpyAsync(mesh_out, m, nreal * sizeof(T), hipMemcpyDeviceToHost, stream));
    double E[4];
    read_energies(E_RECIP, E);      // (one synchronisation; the class flags of this call reach the pair list as in an evaluation)
    nact_seen();
    scf.forget();
  }
  void mesh_gather(const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_, const void* U_,
                   const void* phi_, int which, int on_device, double* E_out, void* pot_, void* grad_, void* fld_,
                   int32_t* info) override {
    const MeshIn in = mesh_stage("admp_mesh_gather", pos_, box, Ql_, pol_, thole_, U_, on_device);
    ARG_CHECK(which == 0 || which == 1, "which must be 0 (the gather) or 1 (the field gather over the polarizable sites)");
    ARG_CHECK(which == 0 || lpol, "the field gather needs a polarizable handle");
    ARG_CHECK(phi_ && E_out && info, "null argument");
    if (which == 0) ARG_CHECK(pot_ && grad_ && (!lpol || fld_), "null output");
    else ARG_CHECK(fld_ != nullptr, "null output");
    ARG_CHECK(K[0] >= 6 && K[1] >= 6 && K[2] >= 6, "PME mesh must be at least 6 points per dimension (order-6 splines)");
    const size_t na = (size_t)top.na, nreal = (size_t)K[0] * K[1] * K[2];
    grad.need(3 * na * sizeof(T));
    mesh_begin(in, box);
    const T* phi = reinterpret_cast<const T*>(phi_);
    if (!on_device) {
      HIP_TRY(hipMemcpyAsync(mesh.p, phi_, nreal * sizeof(T), hipMemcpyHostToDevice, stream));
      phi = mesh.as<T>();
    }
    double E[4];
    int n_rows = ev.n_home;
    if (which == 0) {
      HIP_TRY(hipMemsetAsync(pot.p, 0, 9 * na * sizeof(T), stream));
      HIP_TRY(hipMemsetAsync(grad.p, 0, 3 * na * sizeof(T), stream));
      if (lpol) HIP_TRY(hipMemsetAsync(fld_recip.p, 0, 3 * na * sizeof(T), stream));
      HIP_TRY(hipMemsetAsync(Ed_cur() + E_SLOTS, 0, E_PARTS * sizeof(double), stream));
      stage_gather(phi, grad.as<T>(), lpol ? fld_recip.as<T>() : nullptr, false, Ed_cur() + E_SLOTS);
    } else {
      read_energies(E_RECIP, E, false);      // the count of polarizable sites, as the SCF's first check reads it
      nact_seen();
      n_rows = nact_known();
      HIP_TRY(hipMemsetAsync(fld_recip.p, 0, 3 * na * sizeof(T), stream));
      TIMED("gather_field");
      launch_gather_field<T>(stream, n_rows, sites.as<Site<T>>(), ev.g, phi, fld_recip.as<T>(), act_list());
    }
    ev.active = false;
    read_energies(E_PARTS_SUM, E);
    nact_seen();
    *E_out = which == 0 ? E[1] : 0.0;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (which == 0) {
      HIP_TRY(hipMemcpyAsync(pot_, pot.p, 9 * na * sizeof(T), kind, stream));
      HIP_TRY(hipMemcpyAsync(grad_, grad.p, 3 * na * sizeof(T), kind, stream));
    }
    if (fld_ && (lpol || which == 1)) HIP_TRY(hipMemcpyAsync(fld_, fld_recip.p, 3 * na * sizeof(T), kind, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const int groups = (n_rows + 31) / 32;
    info[0] = which;
    info[1] = n_rows;
    info[2] = groups;
    info[3] = n_rows > 0 ? ((groups + 7) / 8) * 8 : 0;
    scf.forget();
  }

  // admp_site_table / admp_site_close: the first and the last stage of an evaluation alone -- the site pass of stage_begin and
  // what it leaves (site rows, list of polarizable sites, flag word), and the closing kernels on a dE/dQ_global of the
  // caller's through the evaluation's own launchers (tests compare every row with a float64 reference).
  void site_table(const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_, const void* U_,
                  int on_device, void* sites_out, int32_t* act_out, int32_t* info) override {
    const MeshIn in = mesh_stage("admp_site_table", pos_, box, Ql_, pol_, thole_, U_, on_device);
    ARG_CHECK(sites_out && info && (!lpol || act_out), "null argument");
    const size_t na = (size_t)top.na;
    act_n = -1;                      // the list is built by this call, whatever ADMP_OPT_KEEP_POL_SITES vouches for
    mesh_begin(in, box);
    ev.active = false;
    double E[4];
    read_energies(E_RECIP, E);       // (one synchronisation; the class flags of this call reach the pair list as in an evaluation)
    int w[2];
    std::memcpy(w, &Eh[E_NACT], sizeof(w));
    const int n_act = lpol ? w[0] : 0;
    // every other word of this call's half of the energy block was cleared by the site pass of the call before (or by the
    // memset of a first call) and nothing has written to it since
    int dirty = 0;
    for (int k = 0; k < E_WORDS; ++k) dirty += (k != E_NACT && Eh[k] != 0.0) ? 1 : 0;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIP_TRY(hipMemcpyAsync(sites_out, sites.p, sizeof(Site<T>) * na, kind, stream));
    if (n_act > 0)                   // before nact_seen puts the list in atom order
      HIP_TRY(hipMemcpyAsync(act_out, act_d.p, sizeof(int) * (size_t)n_act, kind, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    nact_seen();
    info[0] = n_act; info[1] = w[1]; info[2] = ev.bases ? 1 : 0; info[3] = dirty;
    scf.forget();
  }
  void site_close(const void* pos_, const double* box, const void* Ql_, const void* pol_, const void* thole_, const void* U_,
                  const void* pot_in, const void* phi_in, int which, int want_dQ, int on_device, double* E_out, void* grad_out,
                  void* dQ_out, double* vir_out, int32_t* info) override {
    const MeshIn in = mesh_stage("admp_site_close", pos_, box, Ql_, pol_, thole_, U_, on_device);
    ARG_CHECK(which >= 0 && which <= 2,
              "which must be 0 (the closing kernel), 1 (the closing epilogue of the gather) or 2 (the frame virial)");
    ARG_CHECK(pot_in && info, "null argument");
    if (which < 2) ARG_CHECK(E_out && grad_out && (!want_dQ || dQ_out), "null output");
    else ARG_CHECK(vir_out != nullptr, "null output");
    if (which == 1) {
      ARG_CHECK(phi_in != nullptr, "which = 1: the gather needs a mesh phi_in");
      ARG_CHECK(K[0] >= 6 && K[1] >= 6 && K[2] >= 6, "PME mesh must be at least 6 points per dimension (order-6 splines)");
      ARG_CHECK(fuse_fin_ok(), "which = 1: this handle's evaluations do not close in the gather (no frame groups, or more "
                               "atoms than ADMP_FUSE_FIN_MAX)");
    }
    const size_t na = (size_t)top.na, nreal = (size_t)K[0] * K[1] * K[2];
    const hipMemcpyKind in_kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out_kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    grad.need(3 * na * sizeof(T));
    T* dQ = nullptr;
    if (which < 2 && want_dQ) {
      if (on_device) dQ = reinterpret_cast<T*>(dQ_out);
      else { s_dQ.need(9 * na * sizeof(T)); dQ = s_dQ.as<T>(); }
    }
    mesh_begin(in, box);
    HIP_TRY(hipMemcpyAsync(pot.p, pot_in, 9 * na * sizeof(T), in_kind, stream));
    for (int k = 0; k < 4; ++k) info[k] = 0;
    if (which < 2) {
      HIP_TRY(hipMemsetAsync(grad.p, 0, 3 * na * sizeof(T), stream));
      HIP_TRY(hipMemsetAsync(Ed_cur() + E_SELF, 0, 2 * sizeof(double), stream));
    }
    if (which == 0) {
      finish_launch_choice(top, false, false, info);
      launch_finish_only(grad.as<T>(), dQ);
    } else if (which == 1) {
      const T* phi = reinterpret_cast<const T*>(phi_in);
      if (!on_device) {
        HIP_TRY(hipMemcpyAsync(mesh.p, phi_in, nreal * sizeof(T), hipMemcpyHostToDevice, stream));
        phi = mesh.as<T>();
      }
      if (lpol) HIP_TRY(hipMemsetAsync(fld_recip.p, 0, 3 * na * sizeof(T), stream));
      HIP_TRY(hipMemsetAsync(Ed_cur() + E_SLOTS, 0, E_PARTS * sizeof(double), stream));
      const FinishArgs<T> fin = finish_args(true, dQ);
      stage_gather(phi, grad.as<T>(), lpol ? fld_recip.as<T>() : nullptr, false, Ed_cur() + E_SLOTS, &fin);
      launch_finish_only(grad.as<T>(), dQ);      // (the gather did this work: a no-op, as in an evaluation)
      info[0] = ADMP_FINISH_FORM_GATHER_EPILOGUE;
      info[1] = top.ngathblk;
    } else {
      vir_d.need(V_WORDS * sizeof(double));
      HIP_TRY(hipMemsetAsync(vir_d.p, 0, 9 * sizeof(double), stream));
      launch_frame_virial<T>(stream, top, ev.pos, ev.bx, sites.as<Site<T>>(), lpol, (T)kappa, pot.as<T>(), vir_d.as<double>(),
                             nullptr, top.na);
      HIP_TRY(hipMemcpyAsync(vir_out, vir_d.p, 9 * sizeof(double), hipMemcpyDeviceToHost, stream));
      info[0] = -1;
    }
    ev.active = false;
    double E[4];
    read_energies(E_PARTS_SUM, E);
    nact_seen();
    if (which < 2) {
      E_out[0] = E[2]; E_out[1] = E[3];
      HIP_TRY(hipMemcpyAsync(grad_out, grad.p, 3 * na * sizeof(T), out_kind, stream));
      if (dQ && !on_device) HIP_TRY(hipMemcpyAsync(dQ_out, dQ, 9 * na * sizeof(T), out_kind, stream));
      HIP_TRY(hipStreamSynchronize(stream));
    }
    scf.forget();
  }

  // dE/dpScales[k] at the dipoles given (device pointers): class sums of pair_pscale_deriv, folded like dE/dmScales
  void pscale_grad(const void* pos, const double* box, const void* Ql, const void* pol, const void* thole, int ns,
                   const double* mS, const double* pS, const void* U, double* out) override {
    ARG_CHECK(lpol, "polarizable handle required");
    ARG_CHECK(out && U && ns >= 1 && ns <= 16, "bad argument");
    stage_begin(pos, box, Ql, pol, thole, ns, mS, pS, const_cast<void*>(U));
    vir_d.need(V_WORDS * sizeof(double));
    double* cls = vir_d.as<double>();
    HIP_TRY(hipMemsetAsync(cls, 0, 16 * sizeof(double), stream));
    { TIMED("pscale_grad"); launch_pscale_sums<T>(stream, top.na, wnbr(), sites.as<Site<T>>(), ev.bx, ev.tab, cls,
                                                  snranks > 1 ? pair_rows() : nullptr, ev.n_home); }
    if (snranks > 1) { TIMED("comm_energies"); comm.all_reduce(stream, cls, 16, ADMP_T_F64, ADMP_OP_SUM, ADMP_TAG_ENERGIES); }
    ev.active = false;
    double h16[16];
    HIP_TRY(hipMemcpyAsync(h16, cls, sizeof(h16), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < ns; ++k) out[k] = 0.0;
    for (int nb = 0; nb < 16; ++nb) out[((nb - 1) % ns + ns) % ns] += h16[nb];
  }

  // dE/dmScales[k] = sum over the covalent classes nb that read mScales[k] (index (nb - 1) mod ns, with the reference's
  // negative-index wrap for non-bonded pairs) of the class sums produced by launch_mscale_sums
  void mscale_grad(int kind, const void* pos_, const double* box, const void* par_, int pmax, int ns, double* out,
                   int on_device) override {
    ARG_CHECK(have_top && pl.have(), "topology and pairs must be set first");
    ARG_CHECK(pos_ && box && par_ && out && ns >= 1 && ns <= 16, "bad argument");
    ARG_CHECK(kind >= 0 && kind <= 2, "kind must be 0 (multipolar PME), 1 (dispersion) or 2 (Tang-Toennies)");
    ARG_CHECK(snranks == 1 || on_device, "a slab-decomposed handle takes device pointers");
    const int na = top.na;
    HIP_TRY(hipSetDevice(device));
    double inv[9], vol;
    Box<T> bx = make_box(box, inv, &vol);
    const T* pos = stage_in(s_pos, pos_, 3 * (size_t)na, on_device);
    const size_t npar = kind == 0 ? 9 : (kind == 1 ? 3 : 4);
    const T* par = stage_in(kind == 0 ? s_Q : s_par, par_, npar * (size_t)na, on_device);
    energies_d.need(2 * E_WORDS * sizeof(double));
    ehalf = 0; other_clean = false;
    double* cls = energies_d.as<double>();          // 16 class sums
    HIP_TRY(hipMemsetAsync(cls, 0, 16 * sizeof(double), stream));
    if (kind == 0) {
      ARG_CHECK(have_ewald, "ewald parameters must be set first");
      cls_sites_na = slab_sites_na = -1;   // other rows than an electrostatics evaluation's
      sites.need(sizeof(Site<T>) * (size_t)na);
      RecipGeom<T> g = make_geom(inv);
      launch_prepare_sites<T>(stream, top, pos, par, nullptr, nullptr, nullptr, bx, sites.as<Site<T>>(), nullptr, g, nullptr);
    }
    ScalarRows sr{nullptr, na, nullptr};
    if (snranks > 1) {      // the class sums of the rank's home rows, added over the ranks
      ARG_CHECK(comm.have, "slab-decomposed handle without a communicator (admp_set_comm)");
      if (have_ewald) { update_slab(); sr = scalar_rows(pos, make_geom(inv), K[0], mc.X0, mc.X1, true); }
      else sr = virtual_slab_rows(pos, inv);      // a pair potential has no mesh, as in tt()
    }
    { TIMED("mscale_grad"); launch_mscale_sums<T>(stream, kind, na, pl.table(), sites.as<Site<T>>(), pos, par, bx, pmax, cls, cutoff,
                                                  sr.rows, sr.n); }
    if (snranks > 1) { TIMED("comm_energies"); comm.all_reduce(stream, cls, 16, ADMP_T_F64, ADMP_OP_SUM, ADMP_TAG_ENERGIES); }
    double h16[16];
    HIP_TRY(hipMemcpyAsync(h16, cls, sizeof(h16), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < ns; ++k) out[k] = 0.0;
    for (int nb = 0; nb < 16; ++nb) out[((nb - 1) % ns + ns) % ns] += h16[nb];
  }
};

}  // namespace

struct admp_handle {
  std::unique_ptr<EngineBase> eng;
  std::string err;
};

static std::string g_create_err;

template <class F>
static int guarded(admp_handle* h, F&& f) {
  if (!h || !h->eng) return ADMP_E_ARG;
  try {
    (void)hipSetDevice(h->eng->device);
    (void)hipGetLastError();                 // drop anything stale from other users of this thread
    h->eng->pl.adopt(h->eng->top.na);
    f(*h->eng);
    // a bad launch configuration (too much LDS, too many registers after a flag change, ...) is reported by neither the
    // launch statement nor hipStreamSynchronize: every <<<>>> of this call is covered by one check here
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) throw Err{ADMP_E_HIP, std::string("kernel launch failed: ") + hipGetErrorString(le)};
    return ADMP_OK;
  } catch (const Err& e) {
    h->err = e.msg;
    h->eng->U_src = h->eng->U_src_now = nullptr;      // a failed call leaves no one-shot state behind
    h->eng->after_error();
    return e.code;
  } catch (const std::exception& e) {
    h->err = e.what();
    h->eng->U_src = h->eng->U_src_now = nullptr;
    h->eng->after_error();
    return ADMP_E_ARG;
  }
}

// the same for a translation unit that knows only handle.h (md_driver.hip)
int admp::handle_call(admp_handle* h, void (*fn)(HandleCtx&, void*), void* arg) {
  return guarded(h, [&](EngineBase& e) { fn(e, arg); });
}

extern "C" {

const char* admp_version(void) { return "admp_hip 0.1 (gfx950)"; }

int admp_create(admp_handle** out, int device, int precision) {
  if (!out || (precision != 4 && precision != 8)) return ADMP_E_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return ADMP_E_NOGPU;
  try {
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<EngineBase> e;
    if (precision == 4) e.reset(new Engine<float>());
    else e.reset(new Engine<double>());
    e->device = device;
    e->prec = precision;
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    e->own_stream = true;
    admp_handle* h = new admp_handle();
    h->eng = std::move(e);
    PairList::register_live(&h->eng->pl);
    *out = h;
    return ADMP_OK;
  } catch (const Err& e) {
    g_create_err = e.msg;
    return e.code;
  }
}

int admp_destroy(admp_handle* h) {
  if (!h) return ADMP_E_ARG;
  if (h->eng) {
    (void)hipSetDevice(h->eng->device);
    (void)hipStreamSynchronize(h->eng->stream);
    PairList::unregister_live(&h->eng->pl);
  }
  delete h;
  return ADMP_OK;
}

const char* admp_last_error(const admp_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int admp_use_default_stream(admp_handle* h) {
  return guarded(h, [&](EngineBase& e) {
    HIP_TRY(hipStreamSynchronize(e.stream));
    if (e.own_stream && e.stream) HIP_TRY(hipStreamDestroy(e.stream));
    e.stream = nullptr;          // the legacy default stream
    e.own_stream = false;
  });
}

int admp_set_stream(admp_handle* h, void* hip_stream) {
  return guarded(h, [&](EngineBase& e) {
    HIP_TRY(hipStreamSynchronize(e.stream));
    if (e.own_stream && e.stream) HIP_TRY(hipStreamDestroy(e.stream));
    if (hip_stream) { e.stream = (hipStream_t)hip_stream; e.own_stream = false; }
    else { HIP_TRY(hipStreamCreateWithFlags(&e.stream, hipStreamNonBlocking)); e.own_stream = true; }
  });
}

int admp_synchronize(admp_handle* h) {
  return guarded(h, [&](EngineBase& e) { HIP_TRY(hipStreamSynchronize(e.stream)); });
}

int admp_set_topology(admp_handle* h, int n_atoms, const int32_t* axis_type, const int32_t* axis_idx,
                      const int32_t* excl_rowptr, const int32_t* excl_col, const int32_t* excl_nbonds) {
  return guarded(h, [&](EngineBase& e) { e.set_topology(n_atoms, axis_type, axis_idx, excl_rowptr, excl_col, excl_nbonds); });
}

int admp_set_ewald(admp_handle* h, double kappa, int K1, int K2, int K3, int lmax, int lpol) {
  return guarded(h, [&](EngineBase& e) { e.set_ewald(kappa, K1, K2, K3, lmax, lpol); });
}

int admp_set_pairs(admp_handle* h, int64_t n_rows, const int32_t* pairs, int on_device) {
  return guarded(h, [&](EngineBase& e) { e.set_pairs(n_rows, pairs, on_device); });
}

int admp_share_neighbors(admp_handle* h, admp_handle* lender) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(!lender || lender->eng, "bad lender handle");
    e.share_neighbors(lender ? lender->eng.get() : nullptr);
  });
}

int64_t admp_num_pairs(const admp_handle* h) { return (h && h->eng) ? h->eng->pl.num_pairs() : -1; }

int admp_pme_energy_grad(admp_handle* h, const void* positions, const double* box, const void* Q_local,
                         const void* pol, const void* tholes, int n_scales, const double* mScales,
                         const double* pScales, const double* dScales, void* U_inout, int max_cycle, double thresh,
                         double* E_out, void* dE_dpos, void* dE_dQlocal, int* n_cycle, int* converged,
                         int on_device) {
  (void)dScales;   // accepted and ignored, as in the reference (uscales = 1, admp/pme.py:472)
  return guarded(h, [&](EngineBase& e) {
    e.pme(positions, box, Q_local, pol, tholes, n_scales, mScales, pScales, U_inout, max_cycle, thresh, E_out, dE_dpos,
          dE_dQlocal, n_cycle, converged, on_device);
  });
}

int admp_pme_energy_fixed_dipoles(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                         const void* tholes, int n_scales, const double* mScales, const double* pScales, const void* U,
                         double* E_out, void* dE_dpos, void* dE_dU, void* dE_dQlocal) {
  return guarded(h, [&](EngineBase& e) {
    e.pme_at_U(positions, box, Q_local, pol, tholes, n_scales, mScales, pScales, U, E_out, dE_dpos, dE_dU, dE_dQlocal);
  });
}

int admp_pme_box_grad(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                      const void* tholes, int n_scales, const double* mScales, const double* pScales, const void* U,
                      double* E_out, double* dE_dbox) {
  return guarded(h, [&](EngineBase& e) {
    e.pme_box_grad(positions, box, Q_local, pol, tholes, n_scales, mScales, pScales, U, E_out, dE_dbox);
  });
}
int admp_disp_box_grad(admp_handle* h, const void* positions, const double* box, const void* c_list, int pmax, int n_scales,
                       const double* mScales, double* E_out, double* dE_dbox) {
  return guarded(h, [&](EngineBase& e) { e.disp_box_grad(positions, box, c_list, pmax, n_scales, mScales, E_out, dE_dbox); });
}
int admp_tt_box_grad(admp_handle* h, const void* positions, const double* box, const void* abqc, int n_scales,
                     const double* mScales, double* E_out, double* dE_dbox) {
  return guarded(h, [&](EngineBase& e) { e.tt_box_grad(positions, box, abqc, n_scales, mScales, E_out, dE_dbox); });
}

int admp_pair_program_build(admp_handle* h, const char* hip_source, int n_params, int* program_id) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(program_id, "null");
    *program_id = e.pair_program_build(hip_source, n_params);
  });
}
int admp_pair_program_energy_grad(admp_handle* h, int program_id, const void* positions, const double* box,
                                  const void* params, int n_scales, const double* mScales, double* E_out, void* dE_dpos,
                                  int on_device) {
  return guarded(h, [&](EngineBase& e) {
    e.pair_program_eval(program_id, positions, box, params, n_scales, mScales, E_out, dE_dpos, on_device);
  });
}

int admp_local_frames(admp_handle* h, const void* positions, const double* box, void* frames_out) {
  return guarded(h, [&](EngineBase& e) { e.local_frames(positions, box, frames_out); });
}

int admp_pme_dipoles(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* U,
                     const void* inv_mass, int n_groups, const int32_t* group_start_dev, const int32_t* group_atoms_dev,
                     double* mu_groups_dev, double* out16_dev) {
  return guarded(h, [&](EngineBase& e) {
    e.dipoles(positions, box, Q_local, U, inv_mass, n_groups, group_start_dev, group_atoms_dev, mu_groups_dev, out16_dev);
  });
}

int admp_set_option(admp_handle* h, int option, int value) {
  return guarded(h, [&](EngineBase& e) {
    switch (option) {
      case ADMP_OPT_REFERENCE_KPOINTS: e.ref_korder = value ? 1 : 0; break;
      case ADMP_OPT_KEEP_POL_SITES: e.keep_pol_sites = value ? 1 : 0; break;
      case ADMP_OPT_SIDE_STREAM: e.side_stream_on = value ? 1 : 0; break;
      case ADMP_OPT_ASPC_HOLD: e.aspc_hold = value ? 1 : 0; break;
      default: throw Err{ADMP_E_ARG, "unknown option"};
    }
  });
}

int admp_disp_energy_grad(admp_handle* h, const void* positions, const double* box, const void* c_list, int pmax,
                          int n_scales, const double* mScales, double* E_out, void* dE_dpos, int on_device) {
  return guarded(h, [&](EngineBase& e) { e.disp(positions, box, c_list, pmax, n_scales, mScales, E_out, dE_dpos, on_device); });
}

int admp_prune_pairs(admp_handle* h, const void* positions, const double* box, double rc) {
  return guarded(h, [&](EngineBase& e) { e.prune_pairs(positions, box, rc); });
}

int admp_disp_set_types(admp_handle* h, int n_types, const void* type_of_atom, const double* coefficients) {
  return guarded(h, [&](EngineBase& e) { e.disp_set_types(n_types, type_of_atom, coefficients); });
}

int admp_tt_energy_grad(admp_handle* h, const void* positions, const double* box, const void* abqc, int n_scales,
                        const double* mScales, double* E_out, void* dE_dpos, int on_device) {
  return guarded(h, [&](EngineBase& e) { e.tt(positions, box, abqc, n_scales, mScales, E_out, dE_dpos, on_device); });
}

int admp_mscale_grad(admp_handle* h, int kind, const void* positions, const double* box, const void* params, int pmax,
                     int n_scales, double* dE_dmScales, int on_device) {
  return guarded(h, [&](EngineBase& e) { e.mscale_grad(kind, positions, box, params, pmax, n_scales, dE_dmScales, on_device); });
}

int admp_disp_mesh_spread(admp_handle* h, const void* positions, const double* box, const void* c_list, int pmax, int on_device,
                          void* mesh_out, double* E_self_out, int32_t* info8) {
  return guarded(h, [&](EngineBase& e) { e.disp_mesh_spread(positions, box, c_list, pmax, on_device, mesh_out, E_self_out, info8); });
}
int admp_disp_mesh_gather(admp_handle* h, const void* positions, const double* box, const void* c_list, int pmax,
                          const void* phi_in, int which, int on_device, double* E_self_out, void* out, int32_t* info8) {
  return guarded(h, [&](EngineBase& e) {
    e.disp_mesh_gather(positions, box, c_list, pmax, phi_in, which, on_device, E_self_out, out, info8);
  });
}
int admp_disp_param_grad(admp_handle* h, const void* positions, const double* box, const void* c_list, int pmax, int n_scales,
                         const double* mScales, void* dE_dc) {
  return guarded(h, [&](EngineBase& e) { e.disp_param_grad(positions, box, c_list, pmax, n_scales, mScales, dE_dc); });
}
int admp_tt_param_grad(admp_handle* h, const void* positions, const double* box, const void* abqc, int n_scales,
                       const double* mScales, void* dE_dabqc) {
  return guarded(h, [&](EngineBase& e) { e.tt_param_grad(positions, box, abqc, n_scales, mScales, dE_dabqc); });
}

int admp_pscale_grad(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                     const void* tholes, int n_scales, const double* mScales, const double* pScales, const void* U,
                     double* dE_dpScales) {
  return guarded(h, [&](EngineBase& e) {
    e.pscale_grad(positions, box, Q_local, pol, tholes, n_scales, mScales, pScales, U, dE_dpScales);
  });
}

int admp_thole_sums(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                    const void* tholes, int n_scales, const double* mScales, const double* pScales, const void* U,
                    void* sumX, void* sumXw) {
  return guarded(h, [&](EngineBase& e) { e.thole_sums(positions, box, Q_local, pol, tholes, n_scales, mScales, pScales, U, sumX, sumXw); });
}

int admp_neighbor_count(admp_handle* h, int n_atoms, const void* positions, const double* box, double rc, int64_t* n_pairs) {
  return guarded(h, [&](EngineBase& e) { e.nbr_count(n_atoms, positions, box, rc, n_pairs); });
}
int admp_neighbor_fill(admp_handle* h, int32_t* pairs_out) {
  return guarded(h, [&](EngineBase& e) { e.nbr_fill(pairs_out); });
}

int admp_set_pairs_from_positions(admp_handle* h, const void* positions, const double* box, double rc) {
  return guarded(h, [&](EngineBase& e) { e.nbr_table(positions, box, rc); });
}

int admp_slab_configure(admp_handle* h, int rank, int nranks) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(nranks >= 1 && nranks <= kSlabMaxRanks && rank >= 0 && rank < nranks, "bad rank / nranks (at most 28 ranks)");
    e.srank = rank; e.snranks = nranks;
    if (nranks > 1) e.aspc_off();      // (the fixed form is a single-rank form)
  });
}
int admp_slab_info(admp_handle* h, int64_t* out11) {
  return guarded(h, [&](EngineBase& e) { ARG_CHECK(out11, "null"); e.slab_info(out11); });
}
int admp_set_comm(admp_handle* h, const admp_comm* comm) {
  return guarded(h, [&](EngineBase& e) {
    if (!comm) { e.comm.have = false; e.comm.cb = admp_comm{}; return; }
    ARG_CHECK(comm->all_reduce && comm->all_to_all_v && comm->shift, "communicator with a missing callback");
    e.comm.cb = *comm;
    e.comm.have = true;
  });
}
int admp_set_comm_rccl(admp_handle* h, admp_rccl* c) {
  return guarded(h, [&](EngineBase& e) {
    if (!c) { e.comm.rccl = nullptr; if (!e.comm.cb.all_reduce) e.comm.have = false; return; }
    ARG_CHECK(rccl_device(c) == e.device, "the communicator was created on another device");
    ARG_CHECK(rccl_nranks(c) <= kSlabMaxRanks, "at most 28 slab ranks");
    e.comm.rccl = c;
    e.srank = rccl_rank(c); e.snranks = rccl_nranks(c);
    if (e.snranks > 1) e.aspc_off();
    e.comm.have = true;
  });
}
int admp_set_dipole_source(admp_handle* h, const void* U_init) {
  return guarded(h, [&](EngineBase& e) { e.U_src = U_init; });
}
int admp_set_cutoff(admp_handle* h, double rc) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(rc >= 0.0, "negative cutoff");
    e.cutoff = rc;
  });
}
int admp_scf_aspc(admp_handle* h, int order, int n_corrector, double omega) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(aspc_args_ok(order, n_corrector, omega),
              "order must be -1 (off) or 0..4, n_corrector 1..6, omega <= 0 (Kolafa's value) or in (0, 1]");
    if (order >= 0) {
      if (!e.have_ewald || !e.lpol) throw Err{ADMP_E_STATE, "admp_scf_aspc needs a polarizable handle (admp_set_ewald with lpol)"};
      if (e.snranks > 1) throw Err{ADMP_E_STATE, "admp_scf_aspc: not on a slab-decomposed handle"};
    }
    e.aspc.configure(order, n_corrector, omega);
    e.aspc_dirty = false;
    for (int64_t& c : e.aspc_calls) c = 0;
    e.aspc_resid = 0.0;
  });
}
int admp_scf_aspc_reset(admp_handle* h) {
  return guarded(h, [&](EngineBase& e) { e.aspc.drop(); });
}
int admp_scf_aspc_info(admp_handle* h, int64_t* out8, double* out2) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(out8 && out2, "null");
    out8[0] = e.aspc.order(); out8[1] = e.aspc.on() ? e.aspc.n_corrector() : 0; out8[2] = e.aspc.count();
    for (int k = 0; k < 3; ++k) out8[3 + k] = e.aspc_calls[k];
    out8[6] = out8[7] = 0;
    out2[0] = e.aspc.omega(); out2[1] = e.aspc_resid;
  });
}
int admp_scf_stats(admp_handle* h, int64_t* out8, int reset) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(out8, "null");
    for (int k = 0; k < 8; ++k) { out8[k] = e.scf_stats[k]; if (reset) e.scf_stats[k] = 0; }
  });
}
int admp_xpass_stats(admp_handle* h, int64_t* out2, int reset) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(out2, "null");
    for (int k = 0; k < 2; ++k) { out2[k] = e.mesh_stats.xpass[k]; if (reset) e.mesh_stats.xpass[k] = 0; }
  });
}
int admp_plane_mfma_stats(admp_handle* h, int64_t* out2, int reset) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(out2, "null");
    for (int k = 0; k < 2; ++k) { out2[k] = e.mesh_stats.plane_mfma[k]; if (reset) e.mesh_stats.plane_mfma[k] = 0; }
  });
}
int admp_plane_mfma_stats4(admp_handle* h, int64_t* out4, int reset) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(out4, "null");
    for (int k = 0; k < 4; ++k) { out4[k] = e.mesh_stats.plane_mfma4[k]; if (reset) e.mesh_stats.plane_mfma4[k] = 0; }
  });
}
int admp_mesh_convolve(admp_handle* h, const double* box, int which, void* mesh_inout, int on_device, double* E_out,
                       int32_t* info16) {
  return guarded(h, [&](EngineBase& e) { e.mesh_convolve(box, which, mesh_inout, on_device, E_out, info16); });
}
int admp_slab_mesh_convolve(admp_handle* h, const double* box, int which, void* mesh_inout, int on_device, double* E_out,
                            int32_t* info16) {
  return guarded(h, [&](EngineBase& e) { e.slab_mesh_convolve(box, which, mesh_inout, on_device, E_out, info16); });
}
int admp_pair_real(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                   const void* tholes, int n_scales, const double* mScales, const double* pScales, const void* U,
                   const void* F, int which, int flags, int on_device, double* E_out, void* grad, void* pot, void* fld,
                   int32_t* info4) {
  return guarded(h, [&](EngineBase& e) {
    e.pair_real(positions, box, Q_local, pol, tholes, n_scales, mScales, pScales, U, F, which, flags, on_device, E_out, grad,
                pot, fld, info4);
  });
}
int admp_mesh_spread(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                     const void* tholes, const void* U, int which, int flags, int on_device, void* mesh_out, int32_t* info8) {
  return guarded(h, [&](EngineBase& e) {
    e.mesh_spread(positions, box, Q_local, pol, tholes, U, which, flags, on_device, mesh_out, info8);
  });
}
int admp_mesh_gather(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                     const void* tholes, const void* U, const void* phi_in, int which, int on_device, double* E_out, void* pot,
                     void* grad, void* fld, int32_t* info4) {
  return guarded(h, [&](EngineBase& e) {
    e.mesh_gather(positions, box, Q_local, pol, tholes, U, phi_in, which, on_device, E_out, pot, grad, fld, info4);
  });
}
int admp_site_table(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                    const void* tholes, const void* U, int on_device, void* sites_out, int32_t* act_out, int32_t* info4) {
  return guarded(h, [&](EngineBase& e) {
    e.site_table(positions, box, Q_local, pol, tholes, U, on_device, sites_out, act_out, info4);
  });
}
int admp_site_close(admp_handle* h, const void* positions, const double* box, const void* Q_local, const void* pol,
                    const void* tholes, const void* U, const void* pot_in, const void* phi_in, int which, int want_dQ,
                    int on_device, double* E_out2, void* grad_out, void* dQ_out, double* vir_out9, int32_t* info4) {
  return guarded(h, [&](EngineBase& e) {
    e.site_close(positions, box, Q_local, pol, tholes, U, pot_in, phi_in, which, want_dQ, on_device, E_out2, grad_out, dQ_out,
                 vir_out9, info4);
  });
}
int admp_pair_rider_stats(admp_handle* h, int64_t* out2, int reset) {
  return guarded(h, [&](EngineBase& e) {
    ARG_CHECK(out2, "null");
    for (int k = 0; k < 2; ++k) { out2[k] = e.pair_rider_stats[k]; if (reset) e.pair_rider_stats[k] = 0; }
  });
}
int admp_slab_home(admp_handle* h, int32_t* home_out, int* n_home, int* n_import) {
  return guarded(h, [&](EngineBase& e) { e.slab_home(home_out, n_home, n_import); });
}
int admp_slab_lists(admp_handle* h, int n_atoms, int nranks, int32_t* owner, int32_t* bits, int32_t* home, int32_t* rows,
                    int32_t* act, int32_t* imp, int32_t* exp, int32_t* mig_in, int32_t* mig_out, int64_t* counts) {
  return guarded(h, [&](EngineBase& e) {
    e.slab_lists(n_atoms, nranks, owner, bits, home, rows, act, imp, exp, mig_in, mig_out, counts);
  });
}

int admp_profile_enable(admp_handle* h, int on) {
  return guarded(h, [&](EngineBase& e) { e.prof.collect(e.stream); e.prof.on = on != 0; });
}
int admp_profile_filter(admp_handle* h, const char* label) {
  return guarded(h, [&](EngineBase& e) { e.prof.only = label ? label : ""; });
}
int admp_profile_reset(admp_handle* h) {
  return guarded(h, [&](EngineBase& e) { e.prof.reset(e.stream); });
}
int admp_profile_count(admp_handle* h) {
  if (!h || !h->eng) return ADMP_E_ARG;
  try { h->eng->prof.collect(h->eng->stream); } catch (const Err& e) { h->err = e.msg; return e.code; }
  return (int)h->eng->prof.labels.size();
}
int admp_profile_entry(admp_handle* h, int idx, const char** label, double* total_ms, int64_t* launches) {
  return guarded(h, [&](EngineBase& e) {
    e.prof.collect(e.stream);
    ARG_CHECK(idx >= 0 && idx < (int)e.prof.labels.size(), "profile index out of range");
    if (label) *label = e.prof.labels[idx].c_str();
    if (total_ms) *total_ms = e.prof.total_ms[idx];
    if (launches) *launches = e.prof.count[idx];
  });
}

}  // extern "C"
