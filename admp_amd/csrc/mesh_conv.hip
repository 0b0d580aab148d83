// MeshConv<T> (mesh_conv.h): the host side of the mesh convolution -- rocFFT plans, the tables of the fused-x, direct-DFT and
// two-level paths, the cached G tables, and the launches of one k-space leg on each path.  The kernels are in
// recip_kernels.hip (G tables, k_kspace), fftx_kernels.hip, dft_kernels.hip, pfa_kernels.hip and slab_kernels.hip.
#include "mesh_conv.h"

#include <rocfft/rocfft.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "env.h"
#include "pfa_maps.h"

namespace admp {

namespace {

#define FFT_TRY(x)                                                                                       \
  do {                                                                                                   \
    rocfft_status s_ = (x);                                                                              \
    if (s_ != rocfft_status_success) throw Err{ADMP_E_FFT, std::string(#x) + ": rocfft status " + std::to_string((int)s_)}; \
  } while (0)

std::once_flag g_fft_once;

bool xcirc_on() { static const bool on = env_flag("ADMP_DFT_XCIRC", true); return on; }
int tab_slot(int which) { return which == 1 ? 0 : (which == 6 ? 1 : (which == 8 ? 2 : 3)); }

// (cos, sin)(2 pi m / n), m = 0 .. count-1, appended to tw
template <class T>
void push_twiddles(std::vector<T>& tw, int n, int count) {
  for (int m = 0; m < count; ++m) {
    const double th = 2.0 * M_PI * (double)m / (double)n;
    tw.push_back((T)std::cos(th));
    tw.push_back((T)std::sin(th));
  }
}
void upload(DevBuf& b, const void* src, size_t bytes) {
  b.need(bytes);
  HIP_TRY(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
}

}  // namespace

// what TIMED names in a member function: the handle's profiler and its stream as it is at this call
#define MC_CTX                     \
  Profiler& prof = ctx->prof;      \
  const hipStream_t stream = ctx->stream; \
  const int snranks = ctx->snranks

template <class T>
void MeshConv<T>::update_slab(const int K_[3]) {
  const int srank = ctx->srank, snranks = ctx->snranks;
  for (int d = 0; d < 3; ++d) K[d] = K_[d];
  X0 = (int)((long)srank * K[0] / snranks); X1 = (int)((long)(srank + 1) * K[0] / snranks);
  Y0 = (int)((long)srank * K[1] / snranks); Y1 = (int)((long)(srank + 1) * K[1] / snranks);
  if (snranks > 1) {
    ARG_CHECK(comm->have, "slab-decomposed handle without a communicator (admp_set_comm)");
    const int64_t nh = K[2] / 2 + 1;
    for (int s = 0; s < snranks; ++s) {
      int w = (int)((long)(s + 1) * K[0] / snranks) - (int)((long)s * K[0] / snranks);
      ARG_CHECK(w >= 6, "slab decomposition needs at least 6 mesh planes per rank along x");
      int wy = (int)((long)(s + 1) * K[1] / snranks) - (int)((long)s * K[1] / snranks);
      ARG_CHECK(wy >= 1, "slab decomposition needs at least 1 mesh row per rank along y");
      // transposes: block (x in my slab) x (y in slab s) travels to rank s, block (x in slab s) x (my y rows) comes back
      tr_send[s] = (int64_t)(X1 - X0) * wy * nh * 2;
      tr_recv[s] = (int64_t)w * (Y1 - Y0) * nh * 2;
    }
  }
}

template <class T>
void MeshConv<T>::destroy_plans() {
  for (rocfft_plan* p : {&plan_f, &plan_b, &plan_xf, &plan_xb, &plan2_f, &plan2_b}) {
    if (*p) rocfft_plan_destroy(*p);
    *p = nullptr;
  }
  for (int k = 0; k < 4; ++k) {
    if (plan2n_f[k]) rocfft_plan_destroy(plan2n_f[k]);
    if (plan2n_b[k]) rocfft_plan_destroy(plan2n_b[k]);
    plan2n_f[k] = plan2n_b[k] = nullptr;
  }
  if (info_f) rocfft_execution_info_destroy(info_f);
  info_f = nullptr;
  planK[0] = planK[1] = planK[2] = 0;
}

// batched 2-D r2c / c2r plans over `batch` y-z planes stored back to back: real rows of K2 words, spectrum rows padded to
// fx_khp complex numbers (ensure: whole 128-byte lines on the fused-x path and on a slab rank, K2/2+1 otherwise)
template <class T>
void MeshConv<T>::make_yz_plans(size_t batch, rocfft_plan* fwd, rocfft_plan* bwd) {
  const rocfft_precision pr = sizeof(T) == 4 ? rocfft_precision_single : rocfft_precision_double;
  const size_t len2[2] = {(size_t)K[2], (size_t)K[1]};
  const size_t rs[2] = {1, (size_t)K[2]}, cs[2] = {1, (size_t)fx_khp};
  const size_t rdist = (size_t)K[1] * K[2], cdist = (size_t)K[1] * fx_khp;
  rocfft_plan_description df = nullptr, db = nullptr;
  FFT_TRY(rocfft_plan_description_create(&df));
  FFT_TRY(rocfft_plan_description_set_data_layout(df, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved, nullptr,
                                                  nullptr, 2, rs, rdist, 2, cs, cdist));
  FFT_TRY(rocfft_plan_description_create(&db));
  FFT_TRY(rocfft_plan_description_set_data_layout(db, rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, nullptr,
                                                  nullptr, 2, cs, cdist, 2, rs, rdist));
  FFT_TRY(rocfft_plan_create(fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward, pr, 2, len2, batch, df));
  FFT_TRY(rocfft_plan_create(bwd, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, pr, 2, len2, batch, db));
  rocfft_plan_description_destroy(df);
  rocfft_plan_description_destroy(db);
}

// twiddles of the fused x pass (fftx_kernels.hip): cos, sin of 2 pi m / K0 for the first half turn
template <class T>
void MeshConv<T>::upload_fx_twiddles() {
  std::vector<T> tw;
  push_twiddles(tw, K[0], K[0] / 2);
  tw.resize((size_t)K[0]);
  upload(fx_tw, tw.data(), tw.size() * sizeof(T));
}
// ... of the direct-DFT lines (dft_kernels.hip): a full turn per dimension, back to back
template <class T>
void MeshConv<T>::upload_dft_twiddles() {
  std::vector<T> tw;
  for (int d = 0; d < 3; ++d) push_twiddles(tw, K[d], K[d]);
  upload(dft_tw, tw.data(), tw.size() * sizeof(T));
}
// Two-level direct DFT (pfa_kernels.hip): every dimension either fits the plain lines (<= 160) or splits into a smooth
// cofactor N1 <= 32 and a prime power N2 <= 160 (pfa.ax, set by ensure).  Twiddles, frequency maps of the G table, index tables.
template <class T>
void MeshConv<T>::upload_pfa_tables() {
  pfa.Khp = pfa.ax[2].N1 * (pfa.ax[2].N2 / 2 + 1);
  std::vector<T> tw;
  for (int d = 0; d < 3; ++d) {
    pfa.tw_off[d] = (int)(tw.size() / 2);
    for (int n : {pfa.ax[d].N2, pfa.ax[d].N1}) push_twiddles(tw, n, n);
  }
  upload(pfa_tw, tw.data(), tw.size() * sizeof(T));
  std::vector<int> fm((size_t)K[0] + K[1] + pfa.Khp);
  pfa_freq_of_slot(pfa.ax[0], fm.data());
  pfa_freq_of_slot(pfa.ax[1], fm.data() + K[0]);
  pfa_freq_of_zcolumn(pfa.ax[2], fm.data() + K[0] + K[1]);
  upload(pfa_fmap, fm.data(), fm.size() * sizeof(int));
  std::vector<int> pt((size_t)K[0] + K[1] + K[2]);
  pfa_index_table(pfa.ax[0], pt.data());
  pfa_index_table(pfa.ax[1], pt.data() + K[0]);
  pfa_index_table(pfa.ax[2], pt.data() + K[0] + K[1]);
  upload(pfa_ptab, pt.data(), pt.size() * sizeof(int));
  pfa.ptab[0] = pfa_ptab.as<int>(); pfa.ptab[1] = pfa.ptab[0] + K[0]; pfa.ptab[2] = pfa.ptab[1] + K[1];
  spec.need((size_t)K[0] * K[1] * pfa.Khp * 2 * sizeof(T));
}

template <class T>
void MeshConv<T>::ensure(const int K_[3]) {
  update_slab(K_);
  const int srank = ctx->srank, snranks = ctx->snranks;
  const size_t K2h = (size_t)(K[2] / 2 + 1);
  size_t nspec = (size_t)nxown() * K[1] * K2h;
  const size_t nspec_t = (size_t)K[0] * nyown() * K2h;
  if (nspec_t > nspec) nspec = nspec_t;
  // fused-x path: the kz rows of the spectrum are padded to whole 128-byte lines.  With K2/2+1 = 129 complex numbers per row
  // every row of a tile straddles two lines; padded to 144, rocFFT's batched 2-D r2c / c2r of the 256^3 f32 mesh take
  // 61 / 64 us instead of 88 / 91 (tools/ubench/rocfft_yz_layouts.cpp).
  static const bool fx_on = env_flag("ADMP_FUSED_X", true);
  const bool fx_ok = fx_on && fftx_usable(K[0]);
  const size_t per_line = 128 / (2 * sizeof(T));
  // (a slab rank pads the rows of its batched 2-D transforms the same way; the transposes carry the unpadded rows)
  const int khp = (fx_ok || snranks > 1) ? (int)((K2h + per_line - 1) / per_line * per_line) : (int)K2h;
  if ((size_t)nxown() * K[1] * khp > nspec) nspec = (size_t)nxown() * K[1] * khp;
  spec.need(nspec * 2 * sizeof(T));
  binv_d.need(9 * sizeof(double));
  if (planK[0] == K[0] && planK[1] == K[1] && planK[2] == K[2] && planR == snranks && planRank == srank && plan_f) return;
  fx_khp = khp;
  destroy_plans();
  // the path: the switches as they are now (ADMP_DFT is read at every set-up), the facts from the kernel files
  static const bool pfa_on = env_flag("ADMP_PFA", true);
  PfaPlan split{};      // the split of every dimension, committed to pfa only where the path is the two-level one
  MeshPathIn in;
  in.snranks = snranks;
  in.dft_mode = env_int("ADMP_DFT", -1);
  in.pfa_on = pfa_on; in.fused_x_on = fx_on;
  in.fftx_ok = fftx_usable(K[0]);
  in.splits = true;
  for (int d = 0; d < 3; ++d) { in.K[d] = K[d]; in.splits = pfa_split(K[d], &split.ax[d]) && in.splits; }
  in.zy_fits = dft_zy_fits<T>(K);
  path_ = mesh_path(in);

  std::call_once(g_fft_once, [] { rocfft_setup(); });
  const rocfft_precision pr = sizeof(T) == 4 ? rocfft_precision_single : rocfft_precision_double;
  size_t wmax = 0, w = 0;
  if (snranks == 1) {
    const size_t len[3] = {(size_t)K[2], (size_t)K[1], (size_t)K[0]};   // rocFFT: fastest dimension first
    FFT_TRY(rocfft_plan_create(&plan_f, rocfft_placement_notinplace, rocfft_transform_type_real_forward, pr, 3, len, 1, nullptr));
    FFT_TRY(rocfft_plan_create(&plan_b, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, pr, 3, len, 1, nullptr));
    if (path_ == MeshPath::FusedX) {
      make_yz_plans((size_t)K[0], &plan2_f, &plan2_b);
      FFT_TRY(rocfft_plan_get_work_buffer_size(plan2_f, &w)); if (w > wmax) wmax = w;
      FFT_TRY(rocfft_plan_get_work_buffer_size(plan2_b, &w)); if (w > wmax) wmax = w;
      upload_fx_twiddles();
    }
  } else {
    // distributed transform = batched 2-D r2c over the owned planes, all-to-all transpose (slab_convolve), batched strided
    // 1-D c2c along x
    make_yz_plans((size_t)nxown(), &plan_f, &plan_b);
    const size_t len1[1] = {(size_t)K[0]};
    const size_t stride[1] = {(size_t)nyown() * K2h};
    const size_t batch = (size_t)nyown() * K2h;
    for (int dir = 0; dir < 2; ++dir) {
      rocfft_plan_description desc = nullptr;
      FFT_TRY(rocfft_plan_description_create(&desc));
      FFT_TRY(rocfft_plan_description_set_data_layout(desc, rocfft_array_type_complex_interleaved,
                                                      rocfft_array_type_complex_interleaved, nullptr, nullptr, 1, stride, 1,
                                                      1, stride, 1));
      FFT_TRY(rocfft_plan_create(dir == 0 ? &plan_xf : &plan_xb, rocfft_placement_inplace,
                                 dir == 0 ? rocfft_transform_type_complex_forward : rocfft_transform_type_complex_inverse,
                                 pr, 1, len1, batch, desc));
      FFT_TRY(rocfft_plan_description_destroy(desc));
    }
    FFT_TRY(rocfft_plan_get_work_buffer_size(plan_xf, &w)); if (w > wmax) wmax = w;
    FFT_TRY(rocfft_plan_get_work_buffer_size(plan_xb, &w)); if (w > wmax) wmax = w;
    if (path_ == MeshPath::SlabFusedX) upload_fx_twiddles();   // the fused x pass works on the transposed layout [K0][ny][K2/2+1] as well
  }
  FFT_TRY(rocfft_plan_get_work_buffer_size(plan_f, &w)); if (w > wmax) wmax = w;
  FFT_TRY(rocfft_plan_get_work_buffer_size(plan_b, &w)); if (w > wmax) wmax = w;
  fft_work.need(wmax + 16);
  FFT_TRY(rocfft_execution_info_create(&info_f));
  if (wmax) FFT_TRY(rocfft_execution_info_set_work_buffer(info_f, fft_work.p, wmax));
  planK[0] = K[0]; planK[1] = K[1]; planK[2] = K[2]; planR = snranks; planRank = srank;
  for (auto& k : tabkey) k.kappa = -1;   // mesh changed: tables stale
  if (direct()) upload_dft_twiddles();
  if (path_ == MeshPath::TwoLevel) {
    for (int d = 0; d < 3; ++d) pfa.ax[d] = split.ax[d];
    upload_pfa_tables();
  }
}

template <class T>
const T* MeshConv<T>::ensure_gtab(const double* box, const double* inv, double vol, int which, double kappa, int ref_korder) {
  MC_CTX;
  const bool two = path_ == MeshPath::TwoLevel;
  const int slot = tab_slot(which);
  TabKey& key = tabkey[slot];
  DevBuf& buf = gtabs[slot];
  const size_t nspec_t = (size_t)K[0] * nyown() * spectrum_columns();
  buf.need(nspec_t * sizeof(T));
  gtab_cur = buf.template as<T>();
  bool same = key.kappa == kappa && key.K[0] == K[0] && key.K[1] == K[1] && key.K[2] == K[2] &&
              key.Y0 == (snranks > 1 ? Y0 : 0) && key.ref == ref_korder && key.pfa == two;
  for (int k = 0; k < 9 && same; ++k) same = key.box[k] == box[k];
  if (same) return gtab_cur;
  upload_binv(inv);
  {
    TIMED("gtab");
    launch_gtab<T>(stream, K, snranks > 1 ? Y0 : 0, nyown(), binv_d.as<double>(), std::fabs(vol), kappa, which, gtab_cur, ref_korder,
                   two ? pfa_fmap.as<int>() : nullptr, two ? pfa.Khp : 0);
  }
  std::memcpy(key.box, box, sizeof(key.box));
  key.kappa = kappa; key.K[0] = K[0]; key.K[1] = K[1]; key.K[2] = K[2]; key.Y0 = snranks > 1 ? Y0 : 0; key.ref = ref_korder;
  key.pfa = two;
  if (slot == 0) {
    xctab_ok = false;
    if (direct() && xcirc_on()) {
      xctab.need((size_t)(K[0] / 2 + 1) * K[1] * (K[2] / 2 + 1) * sizeof(T));
      xctab_flag.need(sizeof(int));
      HIP_TRY(hipMemsetAsync(xctab_flag.p, 0, sizeof(int), stream));
      { TIMED("xcirc_table"); launch_ctab<T>(stream, K, gtab_cur, xctab.as<T>(), xctab_flag.as<int>()); }
      int uneven = 1;
      HIP_TRY(hipMemcpyAsync(&uneven, xctab_flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      xctab_ok = uneven == 0;
    }
  }
  return gtab_cur;
}

template <class T>
void MeshConv<T>::upload_binv(const double* inv) {
  HIP_TRY(hipMemcpyAsync(binv_d.p, inv, 9 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));   // `inv` is a caller stack array
}

template <class T>
int MeshConv<T>::path_word() const {
  switch (path_) {
    case MeshPath::TwoLevel: return ADMP_MESH_PATH_TWO_LEVEL;
    case MeshPath::DirectPlanes: return ADMP_MESH_PATH_DIRECT_PLANES;
    case MeshPath::DirectLines: return ADMP_MESH_PATH_DIRECT_LINES;
    case MeshPath::FusedX: case MeshPath::SlabFusedX: return ADMP_MESH_PATH_FUSED_X;
    case MeshPath::Rocfft3D: case MeshPath::SlabRocfftX: break;
  }
  return ADMP_MESH_PATH_ROCFFT;
}

template <class T>
void MeshConv<T>::fill_info(int32_t* info) const {
  info[0] = path_word();
  if (path_ == MeshPath::TwoLevel) {
    int forms[9];
    pfa_forms(pfa, sizeof(T), forms);
    for (int d = 0; d < 3; ++d) { info[2 + d] = pfa.ax[d].N1; info[5 + d] = pfa.ax[d].N2; info[12 + d] = forms[3 * d + 1]; }
    info[8] = forms[0]; info[9] = forms[3]; info[10] = forms[6]; info[11] = forms[8];
  } else if (ctx->snranks > 1) {
    info[2] = X0; info[3] = X1; info[4] = Y0; info[5] = Y1; info[6] = fx_khp; info[7] = K[2] / 2 + 1;
  }
}

template <class T>
void MeshConv<T>::run_plan(const char* label, rocfft_plan plan, void* in, void* out) {
  MC_CTX;
  (void)snranks;
  TIMED(label);
  FFT_TRY(rocfft_execution_info_set_stream(info_f, stream));
  void* i[1] = {in};
  void* o[1] = {out};
  FFT_TRY(rocfft_execute(plan, i, o, info_f));
}

template <class T>
void MeshConv<T>::slab_xpass(XPass form, const XArgs& a, T* buf, int ny, int nh) {
  MC_CTX;
  (void)snranks;
  if (form == XPass::Fused) {
    TIMED("fftx_kspace");
    launch_fftx_conv<T>(stream, K, fx_tw.as<T>(), buf, a.gtab, a.Ed, a.slot, nh, ny);
    return;
  }
  fft_x(buf, 0);
  if (form == XPass::Virial)
    launch_kspace_virial<T>(stream, K, binv_d.as<double>(), std::fabs(a.vol), a.kappa, a.which, a.ref_korder, buf, a.acc_tk, Y0, ny);
  { TIMED("kspace"); launch_kspace<T>(stream, K, ny, a.gtab, buf, a.Ed, a.slot); }
  fft_x(buf, 1);
}

// The distributed convolution of an x-slab rank around its x pass.  The stencils of the home atoms overhang into kGhost
// planes of the next rank (added there before the transform), the 3-D transform is batched 2-D r2c on the owned planes ->
// transpose (all-to-all over the ranks: every GPU exchanges a block with each of the others) -> slab_xpass(tbuf, ny, nh): the x
// lines forward * G * inverse on the ny y rows this rank owns, nh complex numbers each -> transpose back -> 2-D c2r into
// mesh_o, and the gather needs the next rank's first planes of phi as its ghost planes.  Every rank makes the same
// collective calls in the same order.
template <class T>
void MeshConv<T>::slab_convolve(T* mesh_p, T* mesh_o, XPass form, const XArgs& a) {
  MC_CTX;
  T* spec_p = spectrum();
  const size_t plane = (size_t)K[1] * K[2];
  const int nx = nxown(), ny = nyown(), nh = K[2] / 2 + 1;
  ghost.need(kGhost * plane * sizeof(T));
  pack.need((size_t)nx * K[1] * nh * 2 * sizeof(T));
  tbuf.need((size_t)K[0] * ny * nh * 2 * sizeof(T));
  { TIMED("comm_ghost"); comm->shift(stream, mesh_p + (size_t)nx * plane, ghost.p, (int64_t)(kGhost * plane), real_dtype(), 1, ADMP_TAG_GHOST); }
  { TIMED("mesh_add"); launch_mesh_add<T>(stream, (long)(kGhost * plane), mesh_p, ghost.as<T>()); }
  fft_forward(mesh_p, spec_p);
  { TIMED("transpose_pack"); launch_transpose_pack<T>(stream, nx, K[1], nh, fx_khp, snranks, 0, spec_p, pack.as<T>()); }
  { TIMED("comm_transpose"); comm->all_to_all_v(stream, pack.p, tr_send, tbuf.p, tr_recv, real_dtype(), ADMP_TAG_TRANSPOSE); }
  slab_xpass(form, a, tbuf.as<T>(), ny, nh);
  { TIMED("comm_transpose"); comm->all_to_all_v(stream, tbuf.p, tr_recv, pack.p, tr_send, real_dtype(), ADMP_TAG_TRANSPOSE); }
  { TIMED("transpose_pack"); launch_transpose_pack<T>(stream, nx, K[1], nh, fx_khp, snranks, 1, spec_p, pack.as<T>()); }
  fft_inverse(spec_p, mesh_o);
  { TIMED("comm_ghost"); comm->shift(stream, mesh_o, mesh_o + (size_t)nx * plane, (int64_t)(kGhost * plane), real_dtype(), 0, ADMP_TAG_GHOST); }
}

template <class T>
bool MeshConv<T>::convolve(T* mesh_p, const T* gtab, double* Ed, int slot, T* accum, T* out, const PlaneSpread<T>* sp,
                           const PairFieldArgs<T>* rider, const PairFullArgs<T>* prider) {
  MC_CTX;
  T* spec_p = spectrum();
  T* mesh_o = out ? out : mesh_p;
  ARG_CHECK(!sp || can_take_riders(), "internal: plane spread on a transform path without it");
  ARG_CHECK(!(rider && rider->kind) || can_take_riders(), "internal: field rider on a transform path without it");
  ARG_CHECK(!(prider && prider->on) || (can_take_riders() && !(rider && rider->kind == 1)),
            "internal: pair rider on a transform path without it");
  if (snranks > 1) {
    slab_convolve(mesh_p, mesh_o, path_ == MeshPath::SlabFusedX ? XPass::Fused : XPass::Rocfft, XArgs{gtab, Ed, slot});
    return false;
  }
  if (path_ == MeshPath::TwoLevel) {
    const T* tw = pfa_tw.as<T>();
    { TIMED("dft_z_r2c"); launch_pfa_z<T>(stream, pfa, tw, mesh_p, spec_p, 0); }
    { TIMED("dft_y_fwd"); launch_pfa_y<T>(stream, pfa, tw, spec_p, 0); }
    DftTabs<T> tabs;
    tabs.p[0] = gtab;
    { TIMED("dft_x_kspace"); launch_pfa_x_conv<T>(stream, pfa, tw, spec_p, tabs, Ed, slot); }
    { TIMED("dft_y_inv"); launch_pfa_y<T>(stream, pfa, tw, spec_p, 1); }
    { TIMED("dft_z_c2r"); launch_pfa_z<T>(stream, pfa, tw, mesh_p, spec_p, 1); }
    return false;
  }
  if (direct()) {
    const T* tw = dft_tw.as<T>();
    const bool planes = plane_kernels();            // z and y lines of a plane in one workgroup (dft_kernels.hip)
    ARG_CHECK(!sp || planes, "internal: plane spread without the plane kernels");
    int mf = 0;
    if (planes && sp) { TIMED("dft_spread_zy_fwd"); launch_dft_zy<T>(stream, K, tw, mesh_p, spec_p, 0, 1, 0, 0, nullptr, sp, &mf); }
    else if (planes) { TIMED("dft_zy_fwd"); launch_dft_zy<T>(stream, K, tw, mesh_p, spec_p, 0, 1, 0, 0, nullptr, nullptr, &mf); }
    if (planes) { ++stats->plane_mfma[mf ? 0 : 1]; ++stats->plane_mfma4[mf ? 0 : 1]; }
    else {
      { TIMED("dft_z_r2c"); launch_dft_z<T>(stream, K, tw, mesh_p, spec_p, 0); }
      { TIMED("dft_y_fwd"); launch_dft_y<T>(stream, K, tw, spec_p, 0); }
    }
    DftTabs<T> tabs;
    tabs.p[0] = gtab;
    // G table of slot 0 even along x (every orthorhombic cell): one circulant product per line instead of two transforms
    const T* ct = xctab_ok && gtab == gtabs[0].template as<T>() ? xctab.template as<T>() : nullptr;
    ++stats->xpass[ct ? 0 : 1];
    { TIMED("dft_x_kspace"); launch_dft_x_pass<T>(stream, K, tw, spec_p, tabs, Ed, slot, ct, rider, prider); }
    bool added;
    if (planes) {
      TIMED("dft_yz_inv");
      added = launch_dft_zy<T>(stream, K, tw, mesh_p, spec_p, 1, 1, 0, 0, accum, nullptr, &mf);
      ++stats->plane_mfma[1];                       // (word [1] counts the inverse launches of either form)
      ++stats->plane_mfma4[mf ? 2 : 3];
    }
    else {
      { TIMED("dft_y_inv"); launch_dft_y<T>(stream, K, tw, spec_p, 1); }
      { TIMED("dft_z_c2r"); added = launch_dft_z<T>(stream, K, tw, mesh_p, spec_p, 1, 1, 0, 0, accum); }
    }
    return added;
  }
  if (path_ == MeshPath::FusedX) {      // rocFFT for the y-z planes, one fused kernel for x forward * G * x inverse
    run_plan("rocfft_r2c_yz", plan2_f, mesh_p, spec_p);
    { TIMED("fftx_kspace"); launch_fftx_conv<T>(stream, K, fx_tw.as<T>(), spec_p, gtab, Ed, slot, fx_khp); }
    run_plan("rocfft_c2r_yz", plan2_b, spec_p, mesh_o);
    return false;
  }
  fft_forward(mesh_p, spec_p);
  { TIMED("kspace"); launch_kspace<T>(stream, K, nyown(), gtab, spec_p, Ed, slot); }
  fft_inverse(spec_p, mesh_o);
  return false;
}

// Batched y-z plans of the fused-x path for nb meshes at once (dispersion PME: C6 / C8 / C10): the same 2-D r2c / c2r
// plans with batch nb * K0 over meshes / spectra stored back to back -- two rocFFT executions per call instead of 2 nb.
template <class T>
void MeshConv<T>::ensure_batched_plans(int nb) {
  ARG_CHECK(nb >= 2 && nb <= 3 && path_ == MeshPath::FusedX, "internal: batched y-z plans");
  if (plan2n_f[nb]) return;
  make_yz_plans((size_t)nb * K[0], &plan2n_f[nb], &plan2n_b[nb]);
  size_t w = 0, wmax = 0;
  FFT_TRY(rocfft_plan_get_work_buffer_size(plan2n_f[nb], &w)); if (w > wmax) wmax = w;
  FFT_TRY(rocfft_plan_get_work_buffer_size(plan2n_b[nb], &w)); if (w > wmax) wmax = w;
  if (wmax + 16 > fft_work.bytes) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    fft_work.need(wmax + 16);
  }
  if (fft_work.bytes > 16) FFT_TRY(rocfft_execution_info_set_work_buffer(info_f, fft_work.p, fft_work.bytes - 16));
}

template <class T>
void MeshConv<T>::convolve_batch(T* mesh_p, const DftTabs<T>& tabs, int nb, size_t nspec, double* Ed, int slot) {
  MC_CTX;
  (void)snranks;
  T* spec_p = spectrum();
  ensure_batched_plans(nb);
  run_plan("rocfft_r2c_yz", plan2n_f[nb], mesh_p, spec_p);
  { TIMED("fftx_kspace");
    launch_fftx_conv_batch<T>(stream, K, fx_tw.as<T>(), spec_p, tabs, nb, (long)nspec, Ed, slot, fx_khp); }
  run_plan("rocfft_c2r_yz", plan2n_b[nb], spec_p, mesh_p);
}

template <class T>
void MeshConv<T>::convolve_mix(T* mesh_p, const DftTabs<T>& tabs, const MixTab& mix, int nt, size_t nspec, double* Ed, int slot) {
  MC_CTX;
  (void)snranks;
  T* spec_p = spectrum();
  if (nt >= 2) ensure_batched_plans(nt);
  run_plan("rocfft_r2c_yz", nt >= 2 ? plan2n_f[nt] : plan2_f, mesh_p, spec_p);
  { TIMED("fftx_kspace");
    launch_fftx_mix<T>(stream, K, fx_tw.as<T>(), spec_p, tabs, mix, (long)nspec, Ed, slot, fx_khp); }
  run_plan("rocfft_c2r_yz", nt >= 2 ? plan2n_b[nt] : plan2_b, spec_p, mesh_p);
}

template <class T>
void MeshConv<T>::convolve_dft_batch(T* mesh_p, const DftTabs<T>& tabs, int nb, size_t nreal, size_t nspec, double* Ed, int slot,
                                     const MixTab* mix) {
  MC_CTX;
  (void)snranks;
  T* spec_p = spectrum();
  if (path_ == MeshPath::TwoLevel) {
    const T* tw = pfa_tw.as<T>();
    { TIMED("dft_z_r2c"); launch_pfa_z<T>(stream, pfa, tw, mesh_p, spec_p, 0, nb, (long)nreal, (long)nspec); }
    { TIMED("dft_y_fwd"); launch_pfa_y<T>(stream, pfa, tw, spec_p, 0, nb, (long)nspec); }
    { TIMED("dft_x_kspace"); launch_pfa_x_conv<T>(stream, pfa, tw, spec_p, tabs, Ed, slot, nb, (long)nspec); }
    { TIMED("dft_y_inv"); launch_pfa_y<T>(stream, pfa, tw, spec_p, 1, nb, (long)nspec); }
    { TIMED("dft_z_c2r"); launch_pfa_z<T>(stream, pfa, tw, mesh_p, spec_p, 1, nb, (long)nreal, (long)nspec); }
    return;
  }
  const T* tw = dft_tw.as<T>();
  { TIMED("dft_z_r2c"); launch_dft_z<T>(stream, K, tw, mesh_p, spec_p, 0, nb, (long)nreal, (long)nspec); }
  { TIMED("dft_y_fwd"); launch_dft_y<T>(stream, K, tw, spec_p, 0, nb, (long)nspec); }
  { TIMED("dft_x_kspace");
    if (mix) launch_dft_x_mix<T>(stream, K, tw, spec_p, tabs, *mix, (long)nspec, Ed, slot);
    else launch_dft_x_conv<T>(stream, K, tw, spec_p, tabs, Ed, slot, nb, (long)nspec); }
  { TIMED("dft_y_inv"); launch_dft_y<T>(stream, K, tw, spec_p, 1, nb, (long)nspec); }
  { TIMED("dft_z_c2r"); launch_dft_z<T>(stream, K, tw, mesh_p, spec_p, 1, nb, (long)nreal, (long)nspec); }
}

template <class T>
void MeshConv<T>::convolve_virial(T* mesh_p, const T* gtab, double* Ed, int slot, int which, double vol, double kappa,
                                  int ref_korder, double* acc_tk) {
  MC_CTX;
  (void)snranks;
  T* spec_p = spectrum();
  fft_forward(mesh_p, spec_p);
  launch_kspace_virial<T>(stream, K, binv_d.as<double>(), std::fabs(vol), kappa, which, ref_korder, spec_p, acc_tk);
  if (path_ == MeshPath::TwoLevel) {   // this pass goes through rocFFT: it needs the table in the natural layout, not the slot-ordered one
    gtab_nat.need((size_t)K[0] * K[1] * (K[2] / 2 + 1) * sizeof(T));
    launch_gtab<T>(stream, K, 0, K[1], binv_d.as<double>(), std::fabs(vol), kappa, which, gtab_nat.as<T>(), ref_korder);
    gtab = gtab_nat.as<T>();
  }
  { TIMED("kspace"); launch_kspace<T>(stream, K, nyown(), gtab, spec_p, Ed, slot); }
  fft_inverse(spec_p, mesh_p);
}

template <class T>
void MeshConv<T>::convolve_slab_virial(T* mesh_p, const T* gtab, double* Ed, int slot, int which, double vol, double kappa,
                                       int ref_korder, double* acc_tk) {
  slab_convolve(mesh_p, mesh_p, XPass::Virial, XArgs{gtab, Ed, slot, which, vol, kappa, ref_korder, acc_tk});
}

template struct MeshConv<float>;
template struct MeshConv<double>;

}  // namespace admp
