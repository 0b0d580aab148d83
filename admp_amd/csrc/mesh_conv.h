// The k-space leg of a reciprocal pass: mesh <- IFFT( G * FFT(mesh) ) with the energy sum, on whichever path the mesh takes
// (mesh_path.h), and everything that leg owns -- rocFFT plans and their work buffer, twiddle and index tables, the cached G
// tables, the circulant table, the spectrum, the slab bounds and the ghost / transpose buffers of a slab rank.  One MeshConv
// per Engine<T> (engine.hip); defined in mesh_conv.hip.  It knows the handle as a HandleCtx, the communicator and the
// arguments of each call, nothing of topology, neighbour tables or sites.
#pragma once
#include <cstdint>

#include "comm.h"
#include "dev_buf.h"
#include "handle.h"
#include "launch.h"
#include "mesh_path.h"

// (the opaque handles of rocfft/rocfft.h, so that only mesh_conv.hip needs the library's header)
typedef struct rocfft_plan_t* rocfft_plan;
typedef struct rocfft_execution_info_t* rocfft_execution_info;

namespace admp {

// counters of the direct-DFT convolution, owned by EngineBase (its admp_*_stats entry points are not templates)
struct MeshStats {
  int64_t xpass[2] = {0, 0};            // x passes of one mesh (admp_xpass_stats): [0] circulant form, [1] forward * G * inverse
  int64_t plane_mfma[2] = {0, 0};       // plane kernel launches (admp_plane_mfma_stats): [0] with a matrix-core share, [1] without
  int64_t plane_mfma4[4] = {0, 0, 0, 0};   // ... by direction (admp_plane_mfma_stats4): forward share / vector, inverse share / vector
};

template <class T>
struct MeshConv {
  MeshConv(HandleCtx* c, const Comm* cm, MeshStats* st) : ctx(c), comm(cm), stats(st) {}
  MeshConv(const MeshConv&) = delete;
  MeshConv& operator=(const MeshConv&) = delete;
  ~MeshConv() { destroy_plans(); }

  // ---- slab bounds (snranks == 1: the whole mesh is local) ----------------------------------------------------------------
  // rank s owns mesh planes [X0, X1) along x and, in the transposed (k-space) layout, rows [Y0, Y1) along y;
  // the local real mesh additionally carries kGhost planes above X1 (stencil overhang / phi halo).
  static constexpr int kGhost = 5;
  int K[3] = {0, 0, 0};
  int X0 = 0, X1 = 0, Y0 = 0, Y1 = 0;
  void update_slab(const int K_[3]);
  int nloc0() const { return ctx->snranks > 1 ? (X1 - X0) + kGhost : K[0]; }
  int nxown() const { return ctx->snranks > 1 ? (X1 - X0) : K[0]; }
  int nyown() const { return ctx->snranks > 1 ? (Y1 - Y0) : K[1]; }
  size_t nreal_local() const { return (size_t)nloc0() * K[1] * K[2]; }      // words of the local real mesh (the engine's to size)

  // plans, tables and buffers of mesh K_ on this rank: the path is chosen once (mesh_path), only what it needs is built
  void ensure(const int K_[3]);
  void destroy_plans();
  // the G table of `which` (1, 6, 8, 10) for this cell, cached per table; also left in gtab_cur
  const T* ensure_gtab(const double* box, const double* inv, double vol, int which, double kappa, int ref_korder);
  T* gtab_cur = nullptr;
  void upload_binv(const double* inv);
  T* spectrum() const { return spec.template as<T>(); }
  void need_spectrum(size_t bytes) { spec.need(bytes); }      // batches of meshes (dispersion PME) need more than ensure() gives

  // ---- what the engine may ask instead of reading flags -------------------------------------------------------------------
  MeshPath path() const { return path_; }
  bool direct() const { return path_ == MeshPath::DirectPlanes || path_ == MeshPath::DirectLines; }
  bool fused_x() const { return path_ == MeshPath::FusedX || path_ == MeshPath::SlabFusedX; }
  bool plane_kernels() const { return path_ == MeshPath::DirectPlanes; }
  bool can_take_riders() const { return direct(); }      // plane spread, field rider, pair rider: the single-rank direct forms
  int spectrum_pitch() const { return fx_khp; }          // complex numbers per kz row of the spectrum of the y-z plans
  // ... per z row of the spectrum the batched direct forms work on
  int spectrum_columns() const { return path_ == MeshPath::TwoLevel ? pfa.Khp : K[2] / 2 + 1; }
  const PfaPlan& pfa_plan() const { return pfa; }
  int path_word() const;                                 // ADMP_MESH_PATH_*
  // info words of the test entries: [0] the path; two-level: [2..13] the split and the forms; slab rank: [2..7] its bounds
  void fill_info(int32_t* info) const;

  // ---- the leg itself -------------------------------------------------------------------------------------------------
  // mesh <- IFFT( G * FFT(mesh) ), Ed[slot] += sum w G |S|^2
  // accum (optional): a second mesh the result is to be ADDED to; returns true when the last pass did that itself (the direct
  // DFT writes every word once anyway), false when the caller still has to add
  // out (optional, rocFFT paths): phi is written there instead of over mesh_p
  // sp: the forward transform builds its planes from these sites (no spread kernel ran, mesh_p holds nothing yet)
  // rider / prider: pair kernels whose workgroups run inside the x pass (pair_kernels.hip); can_take_riders() only
  bool convolve(T* mesh_p, const T* gtab, double* Ed, int slot, T* accum = nullptr, T* out = nullptr,
                const PlaneSpread<T>* sp = nullptr, const PairFieldArgs<T>* rider = nullptr,
                const PairFullArgs<T>* prider = nullptr);
  // nb meshes at mesh_p + b * nreal -> phi_b in place through batched y-z plans (fused-x path); energies of all channels
  // summed into Ed[slot]; nspec: reals between the spectra
  void convolve_batch(T* mesh_p, const DftTabs<T>& tabs, int nb, size_t nspec, double* Ed, int slot);
  // the same on a direct-DFT mesh (plain or two-level lines): five launches for the batch.  mix (plain lines only): the nb
  // meshes are type meshes, the x pass forms the powers from them at every k (k_dft_x_mix)
  void convolve_dft_batch(T* mesh_p, const DftTabs<T>& tabs, int nb, size_t nreal, size_t nspec, double* Ed, int slot,
                          const MixTab* mix = nullptr);
  // nt type meshes through the y-z plans of the fused-x path, combined into the powers per k in the x pass (k_fftx_mix)
  void convolve_mix(T* mesh_p, const DftTabs<T>& tabs, const MixTab& mix, int nt, size_t nspec, double* Ed, int slot);
  // with the k-tensor sums of the box gradient (acc_tk) taken from the bare spectrum: always through rocFFT (the fused and
  // direct x passes never hold it); binv_d as upload_binv left it
  void convolve_virial(T* mesh_p, const T* gtab, double* Ed, int slot, int which, double vol, double kappa, int ref_korder,
                       double* acc_tk);
  // ... on a slab rank: the sums over the y rows it holds, between the x transforms of the distributed convolution
  void convolve_slab_virial(T* mesh_p, const T* gtab, double* Ed, int slot, int which, double vol, double kappa, int ref_korder,
                            double* acc_tk);

 private:
  HandleCtx* ctx;
  const Comm* comm;
  MeshStats* stats;
  MeshPath path_ = MeshPath::Rocfft3D;

  DevBuf spec, fft_work, binv_d;
  rocfft_plan plan_f = nullptr, plan_b = nullptr;       // 3-D r2c / c2r (one rank, every path: the virial form needs them) or
                                                        // the batched y-z plans of a slab rank
  rocfft_plan plan_xf = nullptr, plan_xb = nullptr;     // slab rank: x lines of the transposed layout
  rocfft_plan plan2_f = nullptr, plan2_b = nullptr;     // FusedX: batched 2-D plans of the y-z planes around the fused x pass
  rocfft_plan plan2n_f[4] = {nullptr, nullptr, nullptr, nullptr}, plan2n_b[4] = {nullptr, nullptr, nullptr, nullptr};   // ... of nb meshes
  rocfft_execution_info info_f = nullptr;
  int planK[3] = {0, 0, 0}, planR = 0, planRank = 0;
  int fx_khp = 0;         // row pitch (complex numbers) of the spectrum the y-z plans write: K2/2+1, padded to whole lines
  DevBuf fx_tw;           // twiddles of the fused x pass
  DevBuf dft_tw;          // ... of the direct-DFT path
  PfaPlan pfa{};          // TwoLevel: spectrum and G tables live in slot order with pfa.Khp z columns
  DevBuf pfa_tw, pfa_fmap, pfa_ptab, gtab_nat;
  DevBuf gtabs[4];        // Ck_1, Ck_6, Ck_8, Ck_10
  struct TabKey { double box[9] = {0}, kappa = -1; int K[3] = {0, 0, 0}, Y0 = 0, ref = 0; bool pfa = false; } tabkey[4];
  // circulant form of the x pass (dft_math.h): first columns of the G table of slot 0, rebuilt with it; xctab_ok: the table
  // is even along x in every column (k_ctab's check, read back when the table is built)
  DevBuf xctab, xctab_flag;
  bool xctab_ok = false;
  // slab rank: overhang planes received, transpose blocks, transposed spectrum; reals sent to / received from every rank
  DevBuf ghost, pack, tbuf;
  int64_t tr_send[kSlabMaxRanks], tr_recv[kSlabMaxRanks];

  static constexpr int real_dtype() { return sizeof(T) == 4 ? ADMP_T_F32 : ADMP_T_F64; }
  void make_yz_plans(size_t batch, rocfft_plan* fwd, rocfft_plan* bwd);
  void upload_fx_twiddles();
  void upload_dft_twiddles();
  void upload_pfa_tables();
  void ensure_batched_plans(int nb);
  void run_plan(const char* label, rocfft_plan plan, void* in, void* out);
  void fft_forward(T* mesh_p, T* spec_p) { run_plan("rocfft_r2c", plan_f, mesh_p, spec_p); }
  void fft_inverse(T* spec_p, T* mesh_p) { run_plan("rocfft_c2r", plan_b, spec_p, mesh_p); }
  void fft_x(T* buf, int inverse) { run_plan(inverse ? "rocfft_x_inv" : "rocfft_x_fwd", inverse ? plan_xb : plan_xf, buf, buf); }
  // the x pass of a slab rank on its ny rows of the transposed spectrum
  enum class XPass { Fused, Rocfft, Virial };
  struct XArgs { const T* gtab; double* Ed; int slot; int which = 0; double vol = 0, kappa = 0; int ref_korder = 0; double* acc_tk = nullptr; };
  void slab_xpass(XPass form, const XArgs& a, T* buf, int ny, int nh);
  void slab_convolve(T* mesh_p, T* mesh_o, XPass form, const XArgs& a);
};

}  // namespace admp
