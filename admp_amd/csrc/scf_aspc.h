// Always-stable predictor-corrector dipoles (J. Kolafa, J. Comput. Chem. 25, 335, 2004) for consecutive polarizable calls:
// the coefficient table, omega(k), the argument checks and the arithmetic of the ring that holds the dipole history.
// Host arithmetic only (no HIP include): the engine keeps one AspcRing per handle, tests/aspc_shim drives it on the CPU.
//
//   U_p = sum_{j=1..k+2} B_j U(n-j),   B_j = (-1)^(j+1) j C(2k+4, k+2-j) / C(2k+2, k+1),   omega = (k+2) / (2k+3)
#pragma once
#include "scf_policy.h"      // kScfChainSteps: the most corrector steps one call enqueues

constexpr int kAspcMaxOrder = 4;
constexpr int kAspcMaxSets = kAspcMaxOrder + 2;      // dipole sets an order-4 history holds

struct AspcFrac { int num, den; };

// B_1 .. B_{k+2} of order k as exact fractions (row k; unused entries 0/1)
constexpr AspcFrac kAspcB[kAspcMaxOrder + 1][kAspcMaxSets] = {
    {{2, 1}, {-1, 1}, {0, 1}, {0, 1}, {0, 1}, {0, 1}},
    {{5, 2}, {-2, 1}, {1, 2}, {0, 1}, {0, 1}, {0, 1}},
    {{14, 5}, {-14, 5}, {6, 5}, {-1, 5}, {0, 1}, {0, 1}},
    {{3, 1}, {-24, 7}, {27, 14}, {-4, 7}, {1, 14}, {0, 1}},
    {{22, 7}, {-55, 14}, {55, 21}, {-22, 21}, {5, 21}, {-1, 42}}};

inline int aspc_sets(int order) { return order + 2; }
inline AspcFrac aspc_coef_frac(int order, int j) { return kAspcB[order][j - 1]; }                       // 1 <= j <= order + 2
inline double aspc_coef(int order, int j) { return (double)kAspcB[order][j - 1].num / kAspcB[order][j - 1].den; }
inline AspcFrac aspc_omega_frac(int order) { return AspcFrac{order + 2, 2 * order + 3}; }
inline double aspc_omega(int order) { return (double)(order + 2) / (2 * order + 3); }

// the arguments of admp_scf_aspc: order -1 (off) .. 4, n_corrector 1 .. kScfChainSteps, omega <= 0 (Kolafa's) or in (0, 1];
// a NaN fails every comparison and is refused
inline bool aspc_args_ok(int order, int n_corrector, double omega) {
  if (order == -1) return true;
  if (order < 0 || order > kAspcMaxOrder) return false;
  if (n_corrector < 1 || n_corrector > kScfChainSteps) return false;
  return omega <= 1.0;      // (false for a NaN)
}
inline double aspc_omega_in_effect(int order, double omega) { return omega > 0.0 ? omega : aspc_omega(order); }

// Which slot of the ring holds U(n-j), how many sets are stored, push and drop.  The ring has order + 2 slots; a new set
// goes to next_slot() and counts only once push() is called, so a call that fails before then leaves the history as it was
// as long as fewer than order + 2 sets are stored (a full ring's next slot is its oldest set: see the engine's dirty mark).
class AspcRing {
  int order_ = -1, n_corr_ = 1;
  double omega_ = 0.0;
  int head_ = 0;       // slot of U(n-1)
  int count_ = 0;

 public:
  bool on() const { return order_ >= 0; }
  int order() const { return order_; }
  int n_corrector() const { return n_corr_; }
  double omega() const { return on() ? aspc_omega_in_effect(order_, omega_) : 0.0; }
  int slots() const { return on() ? aspc_sets(order_) : 0; }
  int count() const { return count_; }
  bool full() const { return on() && count_ == slots(); }
  // false: refused, nothing changes.  Otherwise the mode is (re)set and the history dropped, same values or not.
  bool configure(int order, int n_corrector, double omega) {
    if (!aspc_args_ok(order, n_corrector, omega)) return false;
    order_ = order;
    n_corr_ = order >= 0 ? n_corrector : 1;
    omega_ = order >= 0 ? omega : 0.0;
    drop();
    return true;
  }
  void drop() { head_ = 0; count_ = 0; }
  int slot(int j) const { return ((head_ - (j - 1)) % slots() + slots()) % slots(); }      // 1 <= j <= count()
  int next_slot() const { return count_ == 0 ? head_ : (head_ + 1) % slots(); }
  void push() {
    head_ = next_slot();
    if (count_ < slots()) ++count_;
  }
};
