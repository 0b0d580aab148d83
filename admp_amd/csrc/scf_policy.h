// Which form of the SCF a polarizable call takes, decided from the residual history of the calls before it.
// Host arithmetic only (no HIP include): the engine keeps one ScfHistory per handle, tests/hostshim drives it on the CPU.
#pragma once
#include <algorithm>
#include <cmath>

constexpr int kScfChainSteps = 6;      // most Jacobi steps one chained call enqueues (= E_CHAIN residual words, launch.h)

enum class ScfForm { plain = 0, speculative = 1, chained = 2 };

// spec_mode: ADMP_SPECULATE, 0 / 1 forces the plain / the speculative first cycle (A/B, tests), -1 unset
// chain_max: ADMP_SCF_CHAIN_MAX, atom count up to which a call may be chained
struct ScfSwitches { int spec_mode = -1, chain_max = 200000; };

// nhat: number of Jacobi steps the history predicts (0: no prediction, or the first check will pass)
// pred: predicted residual of the first check (< 0: no prediction)
struct ScfPlan { ScfForm form = ScfForm::plain; int nhat = 0; double pred = -1.0; };

// Residual history of consecutive polarizable calls (MD: every call starts from the previous call's dipoles): the residual
// of a call's first check is the previous call's last residual plus what one step of motion adds.  growth = that
// increase as last observed after a call of the same kind, last = the residual the previous call ended with (< 0: no history).  The first cycle is
// evaluated speculatively with the full kernels only when last + growth predicts that its check will pass.
class ScfHistory {
  bool warm = false;           // previous polarizable call converged at its first SCF check
  double last = -1.0;
  double growth[2][2] = {{0.0, 0.0}, {0.0, 0.0}};    // the last two observed increases after a call without / with a Jacobi
  int nobs[2] = {0, 0};                              // step (they differ: the residual is a maximum norm, not additive);
  int state = 0;                                     // a prediction needs two observations of the current kind
  double contract = -1.0;      // factor by which one Jacobi step shrank the residual in the last call that took steps
                               // ((last / first residual)^(1 / steps); < 0: never observed)

 public:
  // can_chain: the polarizable rows of the call are known to the host (every input of these decisions is the same on every
  // rank of a decomposed handle: the residuals are global maxima)
  ScfPlan plan(double thresh, int na, int max_cycle, bool can_chain, const ScfSwitches& sw) const {
    ScfPlan p;
    // a failed speculation wastes the full pair kernel, the gather and the closing kernel; a successful one saves the field
    // kernels and one synchronisation: at 3072 atoms that is 30 against 45 us, at 98k atoms about even, at 1M atoms 0.55
    // against 0.18 ms -- very large systems speculate only on a clear prediction
    const double spec_infl = na <= 200000 ? 1.0 : 1.5;    // weight of the observed growth (0 on a static geometry)
    const bool have_pred = last >= 0.0 && nobs[state] >= 2;
    const double g_hi = std::max(growth[state][0], growth[state][1]);
    const double g_lo = std::min(growth[state][0], growth[state][1]);
    const bool speculate = sw.spec_mode >= 0 ? sw.spec_mode != 0
                                             : (have_pred ? last + spec_infl * g_hi < thresh : (last < 0.0 && warm));
    p.pred = have_pred ? last + 0.5 * (g_hi + g_lo) : -1.0;
    // number of Jacobi steps the history predicts: the residual contracts by `contract` per step
    if (have_pred && last + g_lo >= 1.1 * thresh && contract > 0.0 && contract < 0.95 && thresh > 0.0) {
      double r = p.pred;
      while (p.nhat <= kScfChainSteps && r >= thresh) { r *= contract; ++p.nhat; }
    }
    const bool chain = sw.spec_mode < 0 && !speculate && na <= sw.chain_max && p.nhat >= 1 && p.nhat <= kScfChainSteps &&
                       p.nhat + 2 <= max_cycle && can_chain;
    p.form = chain ? ScfForm::chained : (speculate ? ScfForm::speculative : ScfForm::plain);
    return p;
  }
  // after a polarizable call: residuals of its first and of its last check (< 0: it made none), Jacobi steps taken
  void observe(double f_first, double f_final, int cyc) {
    warm = (cyc == 0);
    if (f_first < 0.0) return;
    if (last >= 0.0) {
      growth[state][1] = growth[state][0];
      growth[state][0] = f_first - last;
      ++nobs[state];
    }
    last = f_final;
    state = cyc > 0 ? 1 : 0;
    if (cyc >= 1 && f_first > 0.0 && f_final > 0.0 && f_final < f_first) contract = std::pow(f_final / f_first, 1.0 / cyc);
  }
  // an evaluation at dipoles of the caller's choice came between: the next call's first residual continues nothing
  // (growth, state and contract stay; whether a stale contract should survive is a question of behaviour, not decided here)
  void forget() {
    warm = false;
    last = -1.0;
    nobs[0] = nobs[1] = 0;
  }
};
