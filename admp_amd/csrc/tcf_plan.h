// Host-side plan of an admp_md_tcf call (tcf_kernels.hip): the refusals, which lags a frame reaches, where the ring keeps them,
// the grid of the lag kernel and the driver's scratch.  Plain C++ (no HIP), so that tests/tcf_shim compiles it for the host and
// tests/test_tcf_cpu.py can check it without a GPU.
//
//   ring     frame f lives in ring slot f mod L; the lag k of frame f pairs it with frame f - k, slot (f - k) mod L.
//   lags     frame f reaches the lags 0 .. min(f, L - 1): lags_now = min(f, L - 1) + 1 of them.
//   grid     tiles x ceil(lags_now / kTcfLagsPerWg) workgroups of min(256, tile_atoms) lanes; a lane holds
//            ceil(tile_atoms / 256) slots of its tile, 256 apart.
//   scratch  one double per (quantity, tile, lag): 2 n_tiles L of them, whatever the frame.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

namespace admp {

constexpr int kTcfLagsPerWg = 16;     // lags a workgroup walks with its tile's current frame in registers
constexpr int kTcfThreads = 256;      // lanes of a workgroup at most
constexpr int kTcfMaxTileAtoms = 1024;
constexpr int kTcfPlanMaxTypes = 8;   // (= kTcfMaxTypes of tcf_math.h)

struct TcfPlan {
  const char* error = nullptr;        // set: the call is refused with this text
  int threads = 0;                    // lanes of a workgroup of the lag kernel
  int slots_per_lane = 0;
  int lags_now = 0;                   // lags this frame reaches
  int lag_blocks = 0;
  long workgroups = 0;                // of the lag kernel; 0: nothing to launch
  int ring_slot = 0;                  // where this frame goes
  size_t scratch_bytes = 0;
};

inline int tcf_lags_reached(int64_t frame, int n_lags) { return (int)(frame < n_lags - 1 ? frame : n_lags - 1) + 1; }
// the ring slot of the frame `lag` records before `frame` (0 <= lag <= frame)
inline int tcf_ring_slot(int64_t frame, int lag, int n_lags) { return (int)((frame - lag) % n_lags); }
inline size_t tcf_ring_bytes(int n_slots, int n_lags, size_t real_bytes) { return (size_t)n_lags * 6 * (size_t)n_slots * real_bytes; }

inline TcfPlan tcf_make_plan(int n_atoms, int n_slots, int n_tiles, int tile_atoms, int n_types, int n_lags, int64_t frame) {
  TcfPlan p;
  if (n_atoms < 0 || n_slots < 0 || n_tiles < 0) { p.error = "n_atoms, n_slots and n_tiles must not be negative"; return p; }
  if (tile_atoms < 64 || tile_atoms > kTcfMaxTileAtoms || tile_atoms % 64 != 0) { p.error = "tile_atoms must be a multiple of 64 in 64..1024"; return p; }
  if ((long)n_tiles * tile_atoms != (long)n_slots) { p.error = "n_slots must equal n_tiles * tile_atoms"; return p; }
  if (n_types < 1 || n_types > kTcfPlanMaxTypes) { p.error = "n_types must lie in 1..8"; return p; }
  if (n_lags < 1) { p.error = "n_lags must be at least 1"; return p; }
  if (frame < 0) { p.error = "frame must not be negative"; return p; }
  p.threads = tile_atoms < kTcfThreads ? tile_atoms : kTcfThreads;
  p.slots_per_lane = (tile_atoms + kTcfThreads - 1) / kTcfThreads;
  p.lags_now = tcf_lags_reached(frame, n_lags);
  p.lag_blocks = (p.lags_now + kTcfLagsPerWg - 1) / kTcfLagsPerWg;
  p.ring_slot = tcf_ring_slot(frame, 0, n_lags);
  if ((long)n_tiles * p.lag_blocks > (long)INT_MAX) { p.error = "n_tiles * ceil(n_lags / 16) exceeds 2^31 - 1 workgroups"; return p; }
  p.workgroups = (long)n_tiles * p.lag_blocks;
  p.scratch_bytes = 2 * (size_t)n_tiles * (size_t)n_lags * sizeof(double);
  return p;
}

}  // namespace admp
