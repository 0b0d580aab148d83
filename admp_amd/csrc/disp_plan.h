// Which reciprocal-space path a dispersion PME call takes (engine.hip Engine::disp switches on the result): a pure function of
// the handle's mesh plans, the brick rule of the spread, the precision, the number of powers and the type table.  Host-only,
// no HIP header: tests/disp_shim/main.cpp compiles it alone and tests/test_disp_plan_cpu.py walks its whole input space.
#pragma once

namespace admp {

enum class DispPath {
  BricksTyped,      // brick spread of one mesh per TYPE, batched y-z plans, the x pass mixes the types into the powers, one gather
  BricksBatched,    // brick spread of one mesh per power, batched y-z plans, one x pass, interleave, one gather
  BricksPerPower,   // brick spread of one mesh per power, then convolve() and a gather per power
  DftTyped,         // direct-DFT mesh: one-hot site rows per type, one batch of line transforms, the x pass mixes
  DftBatched,       // direct-DFT / two-level mesh: site rows per power, one batch of line transforms
  PerPower          // site rows, spread, convolve(), gather, scale-add per power
};

struct DispPathIn {
  int snranks;             // ranks of the slab decomposition (1: the whole mesh is local)
  bool use_dft, use_pfa;   // the mesh convolution runs on the direct-DFT / on the two-level kernels
  bool use_fx;             // ... on rocFFT y-z plans around the fused x pass
  bool bricks;             // spread_uses_bricks(na, g)
  bool single_precision;
  int nch;                 // powers: (pmax - 4) / 2
  int disp_nt;             // types of admp_disp_set_types (0: none)
  bool have_types;         // ... and their index array
  bool types_on, batch_on; // ADMP_DISP_TYPES, ADMP_DISP_BATCH
};

inline DispPath disp_path(const DispPathIn& in) {
  // at scale (brick regime) and on every slab rank: ONE binning, ONE spread straight from the caller's arrays
  const bool fused = !(in.use_dft || in.use_pfa) && (in.snranks > 1 || in.bricks);
  if (fused) {
    // (more types than powers would mean more transforms than the per-power form: pmax 6 with two types keeps its one mesh)
    const bool typed = in.types_on && in.batch_on && in.snranks == 1 && in.use_fx && in.single_precision && in.disp_nt >= 1 &&
                       in.disp_nt <= in.nch && in.have_types;
    if (typed) return DispPath::BricksTyped;
    if (in.batch_on && in.snranks == 1 && in.use_fx && in.nch >= 2) return DispPath::BricksBatched;
    return DispPath::BricksPerPower;
  }
  // small direct-DFT meshes: the types take the place of the powers in the batch only where they are FEWER
  if (in.types_on && in.disp_nt >= 1 && in.disp_nt < in.nch && in.have_types && in.use_dft && !in.use_pfa && in.snranks == 1 &&
      !in.bricks)
    return DispPath::DftTyped;
  if ((in.use_dft || in.use_pfa) && in.nch > 1) return DispPath::DftBatched;
  return DispPath::PerPower;
}

inline const char* disp_path_name(DispPath p) {
  switch (p) {
    case DispPath::BricksTyped: return "BricksTyped";
    case DispPath::BricksBatched: return "BricksBatched";
    case DispPath::BricksPerPower: return "BricksPerPower";
    case DispPath::DftTyped: return "DftTyped";
    case DispPath::DftBatched: return "DftBatched";
    case DispPath::PerPower: return "PerPower";
  }
  return "?";
}

}  // namespace admp
