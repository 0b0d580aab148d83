#!/usr/bin/env python
"""Velocity-Verlet NVE loop on the full MPID-style water potential: multipolar (optionally polarizable) PME +
dispersion PME + Tang-Toennies damping from libadmp_hip, harmonic bonds / angles (examples' mpidwater.xml:16-21)
and the integrator as HIP kernels too (admp_amd/md.py: one kernel for the bonded terms, one per half step; round 3 spent
~60 torch launches per step on them).  The reference has no integrator; this driver turns the hot
path into a real MD loop: it reports the energy drift (a direct check that the hand-coded adjoints are the gradient of the
energies) and the achieved ns/day including neighbour rebuilds.  Per step the host waits only where the calculators
themselves do (each returns its energy as a number, like the reference's get_forces); the bonded and kinetic energies
stay on the device until a line is logged.

    python examples/md/nve_water.py [--waters 1024] [--steps 200] [--dt 0.5] [--pol] [--single] [--mesh K] [--log 10] [--prune M] [--predict k | --aspc K [--aspc-corr N]] [--dipoles N] [--rdf N [--rdf-out FILE]]
                                    [--msd N [--msd-lags L] [--msd-out FILE]]

--dipoles N records the molecular and cell dipoles every N steps on the device (admp_amd.md.DipoleRecorder) and prints, when the
run ends, the mean molecular dipole in Debye, its permanent and induced shares, and the dielectric constant of the run.
--mesh K: K1 = K2 = K3 = K instead of the reference's rule (admp/pme.py:146-172), e.g. 128 for the 98 304-atom box of
BASELINE configs[2] (the rule gives 305 = 5 * 61 there: every convolution then runs on the two-level DFT kernels, 0.7 ms
each -- with a tight SCF that, not the host, is most of a step).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from water_md import KB, MASS, K_BOND, R0, K_ANG, TH0, bonded, add_arguments, setup, minimize      # noqa: E402,F401
from admp_amd import settings                                                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    add_arguments(ap)
    opt = ap.parse_args()
    w = setup(opt)
    from admp_amd.md import VelocityVerlet
    n_mol, pos, mass, dt, dev, pme = w.n_mol, w.pos, w.mass, w.dtype, 'cuda', w.pme
    nbl, forces, epot_now, state = w.nbl, w.forces, w.epot_now, w.state

    g = torch.Generator(device=dev).manual_seed(1)
    # units: A, fs, amu, kJ/mol.  1 kJ/mol/amu = (1e-2 A/fs)^2;  1 (kJ/mol/A)/amu = 1e-4 A/fs^2
    vel = torch.randn(pos.shape, generator=g, device=dev, dtype=dt) * torch.sqrt(KB * opt.temp / mass) * 1e-2
    h = opt.dt
    vv = VelocityVerlet(pme, np.tile(MASS, n_mol), h)
    pos, pairs, e123, grad = minimize(w, opt, pos)
    w.start_aspc()                                                     # --aspc: every polarizable call is a time step from here
    vel = vel.contiguous()
    log = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(opt.steps):
        vv.kick_drift(pos, vel, grad)                                  # v(t + h/2), r(t + h): in place, one kernel
        if (step + 1) % opt.rebuild == 0:
            pairs = nbl.allocate(pos)
        if opt.prune and (step + 1) % opt.prune == 0:
            nbl.prune(pos)
        e123, grad = forces(pos, pairs)
        w.record_dipoles(step, pos)                                    # --dipoles: two small kernels, nothing read back
        w.record_rdf(step, pos)                                        # --rdf: one C call, integer counters, nothing read back
        w.record_msd(step, pos, vel)                                   # --msd: one C call, sums in double on the device, nothing read back
        rec = step % opt.log == 0 or step == opt.steps - 1
        vv.kick(pos, vel, grad, want_ekin=rec)                         # v(t + h)
        if rec:
            epot, ekin = epot_now(e123), vv.kinetic_energy()
            log.append((step, epot, ekin, epot + ekin))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    e0 = log[0][3]
    for (s, ep, ek, et) in log:
        print('step %5d  Epot %14.4f  Ekin %12.4f  Etot %14.4f  drift %+.3e' % (s, ep, ek, et, (et - e0) / abs(e0)))
    ns_day = opt.steps * h * 1e-6 / wall * 86400.0
    if opt.pol:
        print('\n'.join(w.scf_lines()))
        # which form the library chose for every polarizable call (residual history, engine.hip pme()) and what wrong guesses cost
        print('# SCF forms over the run (real dynamics): %s' % pme.scf_stats())
    for line in w.dipole_lines() + w.rdf_lines() + w.msd_lines():
        print(line)
    print('# %d waters, %s, %s, dt %.2f fs: %.3f ms/step, %.2f ns/day (all terms, list rebuilt every %d steps); '
          'relative energy drift %.2e, T_final %.1f K' % (n_mol, 'polarizable' if opt.pol else 'fixed multipoles',
                                                         settings.PRECISION, h, wall / opt.steps * 1e3, ns_day, opt.rebuild,
                                                         (log[-1][3] - e0) / abs(e0), 2 * log[-1][2] / (3 * 3 * n_mol * KB)))


if __name__ == '__main__':
    main()
