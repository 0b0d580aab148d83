// The neighbour table of a handle and everything that happens to it between two evaluations: compiled from a pair list or from
// positions, parted by site classes, pruned to an inner table, lent to and borrowed from other handles, dropped with the
// topology; and the cell-list search behind admp_neighbor_count / admp_neighbor_fill.  One PairList per EngineBase (engine.hip),
// defined in pair_list.hip.  It knows the handle as a HandleCtx and is told the atom count or the Topology view by argument;
// nothing of sites, meshes, SCF or slabs beyond the RowFilter it is handed.  The engine reads the table through table(),
// gen(), have(), owned() and num_pairs(): nothing outside this class assigns to the table or frees it.
//
// Two rules, each kept in one private function, and every operation that frees, rebuilds or recompiles goes through built():
//   unprune()   such an operation works on the table AS BUILT: an inner table ends first (built() calls it, nothing else does)
//   built()     a borrowed table is a copy of the lender's struct, never freed or modified here: it yields no table to work on
#pragma once
#include <cstdint>

#include "dev_buf.h"
#include "handle.h"
#include "launch.h"

namespace admp {

struct PairList {
  explicit PairList(HandleCtx* c) : ctx(c) {}
  PairList(const PairList&) = delete;
  PairList& operator=(const PairList&) = delete;
  ~PairList() { drop(); cells.release(); }

  // ---- what the engine reads ---------------------------------------------------------------------------------------------
  const NbrTable& table() const { return t; }          // the table the calculators walk: owned, pruned or borrowed
  long gen() const { return gen_; }                    // bumped whenever table() changes
  bool have() const { return have_; }
  bool owned() const { return !lender; }
  int64_t num_pairs() const { return t.n_half; }

  // ---- the handles alive in this process (a borrower asks whether its lender still is) -----------------------------------
  static void register_live(PairList* p);
  static void unregister_live(PairList* p);

  // ---- between evaluations -----------------------------------------------------------------------------------------------
  // refresh a borrowed table from its lender; at the head of every call of a handle of na atoms.  Throws when the lender is gone.
  void adopt(int na);
  // admp_set_pairs: the table of n_rows (i, j) rows, host or device; ends a loan
  void set_pairs(const Topology& top, int64_t n_rows, const int32_t* pairs, int on_device);
  // admp_set_pairs_from_positions: the table of all pairs below rc (rows of rf only); ends a loan
  template <class T>
  void build_from_positions(const Topology& top, const T* pos, const Box<T>& box, const double* heights, double rc,
                            const RowFilter& rf);
  // admp_prune_pairs: from now on table() holds the entries of the table as built that lie below rc (own rowptr / col, everything
  // else shared with it), until the next prune, list build, class compile or drop; rc <= 0: the table as built again
  template <class T>
  void prune(int na, const T* pos, const Box<T>& box, double rc);
  void require_own_table() const;      // ... refused, with admp_prune_pairs' messages, without a table or on a borrowed one
  // admp_share_neighbors: walk lender's table (a handle of the same system that owns its table) / walk none until a list is set
  void borrow(PairList* lender_, int na);
  void end_loan();
  // the topology goes: no table, no loan, no pending classes (the pending count of the search stays: it has its own positions)
  void drop();

  // ---- site classes (NbrTable::cls) --------------------------------------------------------------------------------------
  // k_prepare_sites compares them with the sites of every evaluation and leaves CLS_STALE / CLS_BETTER next to E_NACT;
  // read_energies hands the word to classes_seen, and the next evaluation recompiles the table (part the rows, regroup the row
  // order) before it starts.  A table that is merely not as good as it could be (CLS_BETTER) is left alone for a while after a
  // CLS_STALE, so that a caller alternating between parameter sets does not pay a recompilation per call.
  void classes_seen(int flags) {
    if (flags & CLS_STALE) { cls_pending = true; cls_quiet = 0; }
    else if ((flags & CLS_BETTER) && cls_quiet > 8) cls_pending = true;
  }
  bool classes_pending() const { return cls_pending; }
  void evaluation_begins() { cls_pending = false; ++cls_quiet; }      // (after compile_classes, where one was due)
  // once per handle: an owned table without classes whose first evaluation should look at the flags right away
  bool first_look() {
    if (t.cls || !have_ || lender || cls_first_done) return false;
    return cls_first_done = true;
  }
  // the classes of these sites into the table as built, rows parted and reordered; nothing on a borrowed or missing table
  template <class T>
  void compile_classes(int na, const Site<T>* sites);

  // ---- neighbour search (cell list): two phases so that the caller can size `pairs` --------------------------------------
  template <class T>
  void count(int na, const T* pos, const Box<T>& box, const double* heights, double rc, int64_t* n_pairs);
  template <class T>
  void fill(int32_t* pairs);

 private:
  HandleCtx* ctx;
  DevBuf scan_scratch;          // hipcub's, grown by the builders (scan_bytes)
  size_t scan_bytes = 0;
  NbrTable t;                   // what table() shows
  NbrTable full;                // while pruned: the table as built (t then holds prune_rowptr / prune_col)
  bool pruned = false;
  PairList* lender = nullptr;   // t is a copy of lender->t, refreshed by adopt()
  long lender_gen = -1;
  long gen_ = 0;
  bool have_ = false;
  int na_ = 0;                  // atoms of the table (a borrower compares its own count with its lender's)
  bool cls_pending = false;
  int cls_quiet = 1 << 20;      // evaluations since the last CLS_STALE
  bool cls_first_done = false;  // the flags of the first evaluation have been looked at
  CellScratch cells;
  DevBuf prune_rowptr, prune_cnt, prune_col;
  // the pending count of admp_neighbor_count: its arguments, kept for the fill
  int nb_na = 0;
  const void* nb_pos = nullptr;
  Box<double> nb_box;           // (the words of the Box<T> the count received: exact in a double)
  double nb_rc = 0;
  long long nb_found = 0;

  void unprune();
  NbrTable* built();            // the table as built if this list owns one, else nullptr (see the head of this file)
  void rebuilt(NbrTable& nb, int na);      // after a build or a class compile of *built(): rows parted by class, then ordered
  void order_rows(NbrTable& nb, int na);
};

}  // namespace admp
