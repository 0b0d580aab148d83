// SlabDecomp<T> (slab_decomp.h): the host side of a slab rank's decomposition -- the column plan of slab_plan.h bound to the
// device buffers, the launches of slab_kernels.hip, the one host read of the totals, and the halo exchanges by the lists.
#include "slab_decomp.h"

#include <algorithm>
#include <string>

#include "env.h"

namespace admp {

// what TIMED names in a member function: the handle's profiler and its stream as it is at this call
#define SD_CTX                     \
  Profiler& prof = ctx->prof;      \
  const hipStream_t stream = ctx->stream

template <class T>
void SlabDecomp<T>::decompose(const In& in) {
  SD_CTX;
  const int na = in.na;
  // Atoms that changed hands since the previous evaluation (the home rule follows the positions): their dipoles are valid on
  // the PREVIOUS owner only when the caller keeps home rows (outputs of a decomposed call), so they travel with the atom.
  const bool track = in.with_dipoles && prev_na == na && owner_prev.p;
  static const bool bins_on = env_flag("ADMP_SLAB_BINS", true);
  SlabColumnPlan plan = slab_column_plan(ctx->snranks, ctx->srank, track, bins_on);
  if (plan.refused) throw Err{ADMP_E_ARG, plan.refused};
  owner.need(sizeof(int) * (size_t)na);
  bits_.need(sizeof(int) * (size_t)na);
  owner_prev.need(sizeof(int) * (size_t)na);
  if (track) mig.need(sizeof(int) * (size_t)na);
  plan.bind(na, in.order, mig.as<int>());
  const int ncols = plan.cs.ncols;
  counts.need(sizeof(int) * (size_t)ncols * (size_t)std::max(1, slab_compact_blocks(na)));
  totals.need(sizeof(int) * (kSlabMaxCols + 1));
  lists.need(sizeof(int) * (size_t)ncols * (size_t)na);
  {
    TIMED("slab_decompose");
    int rc = launch_slab_decompose(stream, na, *in.nbr, *in.top, in.bases, in.pol, (int)sizeof(T), in.X1v - in.X0v, in.K0v, in.X0v,
                                   ctx->snranks, ctx->srank, owner.as<int>(), bits_.as<int>(), plan.cs, plan.sb, counts.as<int>(),
                                   totals.as<int>(), lists.as<int>(), track ? owner_prev.as<int>() : nullptr,
                                   track ? mig.as<int>() : nullptr);
    if (rc != 0) throw Err{ADMP_E_HIP, std::string("slab decomposition: ") + hipGetErrorString((hipError_t)rc)};
  }
  int tot[kSlabMaxCols + 1];
  HIP_TRY(hipMemcpyAsync(tot, totals.p, sizeof(int) * (ncols + 1), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (tot[ncols])
    throw Err{ADMP_E_STATE, "an atom entered this rank's slab whose row the neighbour table does not hold: the table of a slab "
                            "rank covers its slab plus a margin of half the list cutoff (admp_set_pairs_from_positions) -- "
                            "rebuild the pair list"};
  seg = slab_segments(plan, tot);
  const int* L = lists.as<int>();
  home_ = L + (size_t)plan.sb.c_home * na;
  rows_ = L + (size_t)plan.c_rows * na;
  act_ = L + (size_t)plan.sb.c_act * na;
  if (tot[plan.c_rows] != seg.n_home) throw Err{ADMP_E_STATE, "slab decomposition: row order and home list disagree"};
  auto joined = [&](const SlabSegs& s, int n, DevBuf& out) {
    out.need(sizeof(int) * (size_t)std::max(1, n));
    launch_slab_concat(stream, s, L, (long)na, out.as<int>());
  };
  joined(seg.imp, seg.n_imp, imp);
  joined(seg.exp, seg.n_exp, exp);
  tracked_ = track;
  if (track) {
    joined(seg.min, seg.n_min, mig_in);
    joined(seg.mout, seg.n_mout, mig_out);
  }
  // the owners of this evaluation are the "previous owners" of the next one
  HIP_TRY(hipMemcpyAsync(owner_prev.p, owner.p, sizeof(int) * (size_t)na, hipMemcpyDeviceToDevice, stream));
  prev_na = in.with_dipoles ? na : -1;
  const size_t w = 9 * sizeof(T) * (size_t)seg.buf_rows;
  sendb.need(w); recvb.need(w);
}

template <class T>
void SlabDecomp<T>::exchange(int what, int w, const char* label, int tag, const DevBuf& out, int n_out, const int64_t* send_cnt,
                             const DevBuf& in, int n_in, const int64_t* recv_cnt, T* data, Site<T>* sites) {
  SD_CTX;
  TIMED(label);                                          // (every rank takes part: the callers' conditions are rank-uniform)
  int64_t sc[kSlabMaxRanks], rc[kSlabMaxRanks];
  for (int t = 0; t < ctx->snranks; ++t) { sc[t] = w * send_cnt[t]; rc[t] = w * recv_cnt[t]; }
  if (what == kPlainRows) launch_rows_gather<T>(stream, n_out, w, out.as<int>(), data, sendb.as<T>());
  else launch_halo_u_pack<T>(stream, n_out, what, out.as<int>(), data, sites, sendb.as<T>());
  comm->all_to_all_v(stream, sendb.p, sc, recvb.p, rc, real_dtype(), tag);
  if (what == kPlainRows) launch_rows_scatter<T>(stream, 1, n_in, w, in.as<int>(), recvb.as<T>(), data);
  else launch_halo_u_unpack<T>(stream, n_in, what, in.as<int>(), recvb.as<T>(), data, sites);
}

template <class T>
void SlabDecomp<T>::exchange_migrants(T* U, Site<T>* sites) {
  exchange(0, 3, "comm_halo_dipoles", ADMP_TAG_HALO_DIPOLES, mig_out, seg.n_mout, seg.mout_cnt, mig_in, seg.n_min, seg.min_cnt, U,
           sites);
}
// owners -> readers: exports out, imports in
template <class T>
void SlabDecomp<T>::exchange_dipoles(int what, T* U, Site<T>* sites) {
  exchange(what, 3, "comm_halo_dipoles", ADMP_TAG_HALO_DIPOLES, exp, seg.n_exp, seg.exp_cnt, imp, seg.n_imp, seg.imp_cnt, U, sites);
}
// ... and back: the imported atoms' rows out, added to the exported atoms' rows
template <class T>
void SlabDecomp<T>::return_gradient(T* grad) {
  exchange(kPlainRows, 3, "comm_halo_gradient", ADMP_TAG_HALO_GRADIENT, imp, seg.n_imp, seg.imp_cnt, exp, seg.n_exp, seg.exp_cnt,
           grad, nullptr);
}

template <class T>
void SlabDecomp<T>::home_to(int32_t* out, int* n_home, int* n_import) const {
  ARG_CHECK(ctx->snranks > 1 && home_, "no decomposed evaluation has run on this handle");
  if (out) HIP_TRY(hipMemcpyAsync(out, home_, sizeof(int) * (size_t)seg.n_home, hipMemcpyDeviceToDevice, ctx->stream));
  if (n_home) *n_home = seg.n_home;
  if (n_import) *n_import = seg.n_imp;
}

template <class T>
void SlabDecomp<T>::lists_to_host(int na, int top_na, int nranks, int32_t* owner_o, int32_t* bits_o, int32_t* home_o,
                                  int32_t* rows_o, int32_t* act_o, int32_t* imp_o, int32_t* exp_o, int32_t* mig_in_o,
                                  int32_t* mig_out_o, int64_t* cnt) const {
  const int N = ctx->snranks;
  const hipStream_t stream = ctx->stream;
  ARG_CHECK(N > 1, "admp_slab_lists works on a slab-decomposed handle only");
  ARG_CHECK(home_, "no decomposed evaluation has run on this handle");
  ARG_CHECK(na == top_na && nranks == N, "n_atoms / nranks are not those of the handle");
  ARG_CHECK(owner_o && bits_o && home_o && rows_o && act_o && imp_o && exp_o && mig_in_o && mig_out_o && cnt, "null argument");
  auto back = [&](int32_t* dst, const void* src, int n) {
    if (n > 0) HIP_TRY(hipMemcpyAsync(dst, src, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, stream));
  };
  back(owner_o, owner.p, na);
  back(bits_o, bits_.p, na);
  back(home_o, home_, seg.n_home);
  back(rows_o, rows_, seg.n_home);
  back(act_o, act_, seg.n_act);
  back(imp_o, imp.p, seg.n_imp);
  back(exp_o, exp.p, seg.n_exp);
  back(mig_in_o, mig_in.p, seg.n_min);
  back(mig_out_o, mig_out.p, seg.n_mout);
  HIP_TRY(hipStreamSynchronize(stream));
  cnt[0] = seg.n_home; cnt[1] = seg.n_act; cnt[2] = seg.n_imp; cnt[3] = seg.n_exp;
  cnt[4] = tracked_ ? 1 : 0; cnt[5] = seg.n_min; cnt[6] = seg.n_mout; cnt[7] = 0;
  for (int t = 0; t < N; ++t) {
    cnt[8 + t] = seg.imp_cnt[t];
    cnt[8 + N + t] = seg.exp_cnt[t];
    cnt[8 + 2 * N + t] = seg.min_cnt[t];
    cnt[8 + 3 * N + t] = seg.mout_cnt[t];
  }
}

template struct SlabDecomp<float>;
template struct SlabDecomp<double>;

}  // namespace admp
