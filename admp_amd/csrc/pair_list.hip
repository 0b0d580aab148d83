// PairList (pair_list.h): the host side of a handle's neighbour table.  The kernels are in nbr_kernels.hip (table from a pair
// list, row order, class partition, pruning) and cell_kernels.hip (cell-list search, table from positions).
#include "pair_list.h"

#include <mutex>
#include <set>
#include <string>

#include "env.h"

namespace admp {

namespace {

std::set<PairList*>& live() { static std::set<PairList*> s; return s; }
std::mutex& live_mu() { static std::mutex m; return m; }
bool is_live(PairList* p) { std::lock_guard<std::mutex> g(live_mu()); return live().count(p) != 0; }

void hip_rc(int rc, const char* what) {
  if (rc != 0) throw Err{ADMP_E_HIP, std::string(what) + ": " + hipGetErrorString((hipError_t)rc)};
}

}  // namespace

// what TIMED names in a member function: the handle's profiler and its stream as it is at this call
#define PL_CTX                \
  Profiler& prof = ctx->prof; \
  const hipStream_t stream = ctx->stream

void PairList::register_live(PairList* p) { std::lock_guard<std::mutex> g(live_mu()); live().insert(p); }
void PairList::unregister_live(PairList* p) { std::lock_guard<std::mutex> g(live_mu()); live().erase(p); }

// ---- the two rules ------------------------------------------------------------------------------------------------------------
void PairList::unprune() {
  if (!pruned) return;
  t = full;
  full = NbrTable();
  pruned = false;
  ++gen_;
}

NbrTable* PairList::built() {
  if (lender) return nullptr;   // the lender's buffers
  unprune();
  return &t;
}

// ---- loans --------------------------------------------------------------------------------------------------------------------
void PairList::end_loan() {
  if (!lender) return;
  t = NbrTable();               // forget the lender's pointers
  lender = nullptr; lender_gen = -1;
  have_ = false;
  ++gen_;
}

void PairList::adopt(int na) {
  if (!lender) return;
  if (!is_live(lender)) {
    t = NbrTable(); lender = nullptr; have_ = false;
    throw Err{ADMP_E_ARG, "the handle the neighbour table was borrowed from has been destroyed"};
  }
  if (!lender->have_ || lender->na_ != na) { t = NbrTable(); have_ = false; return; }
  if (lender_gen != lender->gen_ || t.col != lender->t.col || t.order != lender->t.order || t.order_plain != lender->t.order_plain) {
    if (lender->ctx->stream != ctx->stream) HIP_TRY(hipStreamSynchronize(lender->ctx->stream));   // built / ordered on the lender's stream
    t = lender->t;
    lender_gen = lender->gen_;
    ++gen_;
  }
  have_ = true; na_ = na;       // (this list may lend in turn)
}

void PairList::borrow(PairList* lender_, int na) {
  if (NbrTable* nb = built()) nb->free_all();   // drop the table this list owns
  t = NbrTable();
  lender = lender_; lender_gen = -1;
  have_ = false;
  adopt(na);
}

void PairList::drop() {
  if (NbrTable* nb = built()) nb->free_all();
  t = NbrTable();
  lender = nullptr; lender_gen = -1;
  cls_pending = false; cls_quiet = 1 << 20;
  have_ = false; na_ = 0;
  ++gen_;
}

// ---- builds -------------------------------------------------------------------------------------------------------------------
// row order of the freshly built table (see launch_row_order); ADMP_PAIR_SORT=0 keeps the natural order
void PairList::order_rows(NbrTable& nb, int na) {
  static const bool off = !env_flag("ADMP_PAIR_SORT", true);
  const hipStream_t stream = ctx->stream;
  if (off) {
    if (nb.order) { (void)hipFree(nb.order); nb.order = nullptr; }
    if (nb.order_plain) { (void)hipFree(nb.order_plain); nb.order_plain = nullptr; }
    return;
  }
  if (!nb.order) HIP_TRY(hipMalloc(&nb.order, sizeof(int) * (size_t)na));
  launch_row_order(stream, na, nb.rowptr, nb.order, nb.cls);
  if (nb.cls) {
    if (!nb.order_plain) HIP_TRY(hipMalloc(&nb.order_plain, sizeof(int) * (size_t)na));
    launch_row_order(stream, na, nb.rowptr, nb.order_plain, nullptr);
  }
}

// after a table build or a class compile: part the rows by the classes the table knows, then order them
void PairList::rebuilt(NbrTable& nb, int na) {
  if (nb.cls) hip_rc(launch_class_partition(ctx->stream, na, nb), "class partition");
  order_rows(nb, na);
}

void PairList::set_pairs(const Topology& top, int64_t n_rows, const int32_t* pairs, int on_device) {
  PL_CTX;
  ARG_CHECK(n_rows >= 0, "negative pair count");
  end_loan();                   // a pair list of its own ends a borrowed table
  NbrTable& nb = *built();
  DevBuf staged;
  const int* dev = pairs;
  if (!on_device && n_rows > 0) {
    staged.need(sizeof(int) * 2 * (size_t)n_rows);
    HIP_TRY(hipMemcpyAsync(staged.p, pairs, sizeof(int) * 2 * (size_t)n_rows, hipMemcpyHostToDevice, stream));
    dev = staged.as<int>();
  }
  {
    TIMED("nbr_build");
    if (nb.built) { (void)hipFree(nb.built); nb.built = nullptr; }      // (a table from an explicit list holds every row)
    hip_rc(build_neighbour_table(stream, top, n_rows, dev, nb, &scan_scratch.p, &scan_bytes), "build_neighbour_table");
    rebuilt(nb, top.na);
  }
  HIP_TRY(hipStreamSynchronize(stream));      // `staged` is freed on the way out, and on the way out of a throw above
  have_ = true; na_ = top.na;
  ++gen_;
}

template <class T>
void PairList::build_from_positions(const Topology& top, const T* pos, const Box<T>& box, const double* heights, double rc,
                                    const RowFilter& rf) {
  PL_CTX;
  end_loan();
  NbrTable& nb = *built();
  TIMED("neighbor_table");
  hip_rc(cell_build_table<T>(stream, top, pos, box, heights, rc, cells, nb, rf), "cell_build_table");
  rebuilt(nb, top.na);
  have_ = true; na_ = top.na;
  ++gen_;
}

void PairList::require_own_table() const {
  ARG_CHECK(have_, "a pair list must be set before it can be pruned");
  ARG_CHECK(!lender, "prune the lender's table: a borrowed one follows it");
}

template <class T>
void PairList::prune(int na, const T* pos, const Box<T>& box, double rc) {
  PL_CTX;
  require_own_table();
  NbrTable* nb = built();       // (always from the table as built)
  if (rc <= 0) return;
  const size_t entries = 2 * (size_t)nb->n_half;
  prune_rowptr.need(sizeof(int) * ((size_t)na + 1));
  prune_cnt.need(sizeof(int) * ((size_t)na + 1));
  prune_col.need(sizeof(int) * (entries + 1));
  int64_t total = 0;
  TIMED("prune_pairs");
  hip_rc(prune_table<T>(stream, na, *nb, pos, box, rc, prune_rowptr.as<int>(), prune_cnt.as<int>(), prune_col.as<int>(),
                        &scan_scratch.p, &scan_bytes, &total), "prune_table");
  full = t;
  t.rowptr = prune_rowptr.as<int>();
  t.col = prune_col.as<int>();
  t.n_half = total / 2;
  t.cap = (int64_t)entries + 1;
  t.col_alt = nullptr; t.cap_alt = 0;      // (build scratch of the full table: not this one's)
  t.deg = nullptr; t.deg_na = 0;
  pruned = true;
  ++gen_;
}

template <class T>
void PairList::compile_classes(int na, const Site<T>* sites) {
  if (!have_) return;
  NbrTable* nb = built();       // (classes are compiled into the table as built)
  if (!nb) return;
  if (!nb->cls) HIP_TRY(hipMalloc(&nb->cls, sizeof(int) * (size_t)na));
  launch_site_classes<T>(ctx->stream, na, sites, nb->cls);
  rebuilt(*nb, na);
}

// ---- neighbour search (cell list) ---------------------------------------------------------------------------------------------
template <class T>
void PairList::count(int na, const T* pos, const Box<T>& box, const double* heights, double rc, int64_t* n_pairs) {
  PL_CTX;
  for (int k = 0; k < 9; ++k) { nb_box.h[k] = box.h[k]; nb_box.hinv[k] = box.hinv[k]; }
  nb_na = na; nb_pos = pos; nb_rc = rc;
  long long n = 0;
  TIMED("neighbor_count");
  hip_rc(cell_count_pairs<T>(stream, na, pos, box, heights, rc, cells, &n), "cell_count_pairs");
  nb_found = n;
  *n_pairs = (int64_t)n;
}

template <class T>
void PairList::fill(int32_t* pairs) {
  PL_CTX;
  ARG_CHECK(nb_pos, "admp_neighbor_count must precede admp_neighbor_fill");
  // no pair within rc (one atom, a dilute gas) is a valid answer: nothing to write, the output may be NULL
  ARG_CHECK(pairs || nb_found == 0, "null output for a non-empty pair list");
  const T* pos = static_cast<const T*>(nb_pos);
  nb_pos = nullptr;                            // the pending count is spent, whatever the fill returns
  if (nb_found == 0) return;
  Box<T> box;
  for (int k = 0; k < 9; ++k) { box.h[k] = (T)nb_box.h[k]; box.hinv[k] = (T)nb_box.hinv[k]; }
  TIMED("neighbor_fill");
  hip_rc(cell_fill_pairs<T>(stream, nb_na, pos, box, nb_rc, cells, pairs), "cell_fill_pairs");
}

#define PL_INSTANTIATE(T)                                                                                                      \
  template void PairList::build_from_positions<T>(const Topology&, const T*, const Box<T>&, const double*, double,             \
                                                  const RowFilter&);                                                           \
  template void PairList::prune<T>(int, const T*, const Box<T>&, double);                                                      \
  template void PairList::compile_classes<T>(int, const Site<T>*);                                                             \
  template void PairList::count<T>(int, const T*, const Box<T>&, const double*, double, int64_t*);                             \
  template void PairList::fill<T>(int32_t*)
PL_INSTANTIATE(float);
PL_INSTANTIATE(double);

}  // namespace admp
