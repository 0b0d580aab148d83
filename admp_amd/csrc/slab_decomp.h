// The decomposition of one evaluation on a slab rank (snranks > 1) and the halo exchanges that go by its lists: who owns what,
// derived by every rank from the replicated inputs, and the three all-to-all-v exchanges between owners and readers.  One
// SlabDecomp per Engine<T> (engine.hip); defined in slab_decomp.hip.  The planning is slab_plan.h's, the kernels are
// slab_kernels.hip's.  It knows the handle as a HandleCtx, the communicator and the arguments of each call, nothing of the
// engine's evaluation record.
#pragma once
#include <cstdint>

#include "comm.h"
#include "dev_buf.h"
#include "handle.h"
#include "launch.h"
#include "slab_plan.h"

namespace admp {

template <class T>
struct SlabDecomp {
  SlabDecomp(HandleCtx* c, const Comm* cm) : ctx(c), comm(cm) {}
  SlabDecomp(const SlabDecomp&) = delete;
  SlabDecomp& operator=(const SlabDecomp&) = delete;

  // K0v / X0v / X1v: the planes the ownership rule works on (the PME mesh's; a handle without a mesh takes a virtual one);
  // bases: the stencil base planes of all atoms; pol: polarizabilities (nullptr: no atom is polarizable); order: the row order
  // of the table to filter (nullptr: natural order); with_dipoles: the evaluation carries induced dipoles from call to call
  // (atoms that change hands take theirs along)
  struct In {
    int na = 0;
    const NbrTable* nbr = nullptr;
    const Topology* top = nullptr;
    const int4* bases = nullptr;
    const T* pol = nullptr;
    int K0v = 0, X0v = 0, X1v = 0;
    const int* order = nullptr;
    bool with_dipoles = false;
  };
  // Who owns what in this evaluation (no communication): home atoms, home rows in pair-kernel order, polarizable home atoms,
  // imports per owner, exports per reader, and -- tracked -- the atoms that changed hands.  One host read (the counts).
  void decompose(const In& in);
  // whether the next decompose() of na atoms will list the atoms that changed hands (the caller then moves their dipoles)
  bool will_track(int na, bool lpol) const { return lpol && prev_na == na; }
  // the owners on record belong to a system that is gone (admp_set_topology)
  void forget() { prev_na = -1; tracked_ = false; }

  const int* home() const { return home_; }      // home atoms, ascending
  const int* rows() const { return rows_; }      // home rows in the pair kernels' order (the table's class-grouped order, filtered)
  const int* act() const { return act_; }        // polarizable home atoms, ascending
  const int* imports() const { return imp.as<int>(); }
  const int* bits() const { return bits_.as<int>(); }
  int n_home() const { return seg.n_home; }
  int n_act() const { return seg.n_act; }
  int n_imp() const { return seg.n_imp; }
  bool tracked() const { return tracked_; }      // the last decomposition compared its owners with the previous one's
  bool decomposed() const { return home_ != nullptr; }

  // the dipoles of the atoms that changed hands: previous owner -> new owner
  void exchange_migrants(T* U, Site<T>* sites);
  // what 0: the Cartesian dipoles of the atoms this rank reads <- their owners' values (start of an evaluation: the result
  // must not depend on rows of U the rank does not own); what 1: the last Jacobi step's change of those dipoles
  void exchange_dipoles(int what, T* U, Site<T>* sites);
  // what the closing kernel added to atoms of other ranks (frame adjoint of molecules across a slab face) goes to the owners
  void return_gradient(T* grad);

  // admp_slab_home / admp_slab_lists: what decompose() left on the device (no kernel runs)
  void home_to(int32_t* out, int* n_home, int* n_import) const;
  void lists_to_host(int na, int top_na, int nranks, int32_t* owner, int32_t* bits, int32_t* home, int32_t* rows, int32_t* act,
                     int32_t* imp, int32_t* exp, int32_t* mig_in, int32_t* mig_out, int64_t* counts) const;

 private:
  HandleCtx* ctx;
  const Comm* comm;
  DevBuf owner, owner_prev, mig, bits_, counts, totals, lists, imp, exp, mig_in, mig_out, sendb, recvb;
  int prev_na = -1;             // owner_prev holds the owners of this handle's previous decomposed evaluation of prev_na atoms
  bool tracked_ = false;        // (mig_in / mig_out are lists)
  SlabSegments seg;             // counts per rank and in all (slab_plan.h)
  const int* home_ = nullptr;
  const int* rows_ = nullptr;
  const int* act_ = nullptr;

  static constexpr int real_dtype() { return sizeof(T) == 4 ? ADMP_T_F32 : ADMP_T_F64; }
  // The one body of the three exchanges: the n_out rows of width w listed in `out` are packed, travel by one all-to-all-v
  // (send_cnt / recv_cnt: rows per rank) and land on the n_in rows listed in `in`.  what 0 / 1: dipoles / dipole steps of
  // (data, sites), set on arrival; kPlainRows: rows of data, added on arrival.
  static constexpr int kPlainRows = -1;
  void exchange(int what, int w, const char* label, int tag, const DevBuf& out, int n_out, const int64_t* send_cnt,
                const DevBuf& in, int n_in, const int64_t* recv_cnt, T* data, Site<T>* sites);
};

}  // namespace admp
