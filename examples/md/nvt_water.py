#!/usr/bin/env python
"""Langevin NVT loop (BAOAB) on the full MPID-style water potential: the calculators, lists and forces of nve_water.py
(water_md.py) under the thermostat of admp_amd/md.py.  The first half of a step -- kick, half drift, friction + noise, half
drift -- is ONE elementwise HIP kernel (admp_md_langevin) that draws its noise in registers from a counter-based generator
(Philox-4x32-10: a function of (seed, step, atom) alone, so a run restarted at any step repeats its noise); the second half
is the kick of velocity Verlet.  The velocities start from a Maxwell-Boltzmann draw of the same generator
(admp_amd.md.maxwell_boltzmann), and the driver logs the kinetic temperature: after the minimised box has heated up
(friction * time of a few units) it fluctuates around --temp with the relative width sqrt(2 / 3N).

    python examples/md/nvt_water.py [--waters 1024] [--steps 200] [--dt 0.5] [--temp 300] [--friction 0.05] [--seed 1] [--pol]
                                    [--single] [--mesh K] [--log 10] [--prune M] [--predict k | --aspc K [--aspc-corr N]]
                                    [--thermostat {langevin,vrescale}] [--tau-t 100] [--dipoles N] [--rdf N [--rdf-out FILE]]
                                    [--msd N [--msd-lags L] [--msd-out FILE]]

--thermostat vrescale runs velocity Verlet (the same first-half kernel at friction 0) under stochastic velocity rescaling
(admp_amd.md.VRescale, relaxation time --tau-t fs): the closing half kick and the thermostat are one C call, and the log gains
the conserved quantity E_pot + E_kin - heat, whose drift the final line reports.  The other arguments are those of nve_water.py.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from water_md import MASS, add_arguments, add_thermostat_arguments, drift_of, setup, minimize      # noqa: E402
from admp_amd import settings                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    add_arguments(ap)
    ap.add_argument('--friction', type=float, default=0.05, help='1/fs')
    ap.add_argument('--seed', type=int, default=1, help='of the initial velocities and of the thermostat\'s noise')
    add_thermostat_arguments(ap)
    opt = ap.parse_args()
    w = setup(opt)
    from admp_amd.md import Langevin, VRescale, maxwell_boltzmann
    n_mol, pme, nbl, forces, epot_now, state = w.n_mol, w.pme, w.nbl, w.forces, w.epot_now, w.state
    masses = np.tile(MASS, n_mol)
    h = opt.dt
    # units: A, fs, amu, kJ/mol
    vel = maxwell_boltzmann(pme, masses, opt.temp, opt.seed)
    vr = opt.thermostat == 'vrescale' and VRescale(pme, masses, h, opt.temp, opt.tau_t, opt.seed, n_dof=3 * len(masses) - 3)
    lv = Langevin(pme, masses, h, opt.temp, 0.0 if vr else opt.friction, opt.seed)
    pos, pairs, e123, grad = minimize(w, opt, w.pos)
    w.start_aspc()                                                     # --aspc: every polarizable call is a time step from here
    log = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(opt.steps):
        lv.kick_drift(pos, vel, grad)                                  # B, A, O, A: in place, one kernel
        if (step + 1) % opt.rebuild == 0:
            pairs = nbl.allocate(pos)
        if opt.prune and (step + 1) % opt.prune == 0:
            nbl.prune(pos)
        e123, grad = forces(pos, pairs)
        w.record_dipoles(step, pos)                                    # --dipoles: two small kernels, nothing read back
        w.record_rdf(step, pos)                                        # --rdf: one C call, integer counters, nothing read back
        w.record_msd(step, pos, vel)                                   # --msd: one C call, sums in double on the device, nothing read back
        rec = step % opt.log == 0 or step == opt.steps - 1
        if vr:
            vr.kick(vel, grad)                                         # B: v(t + h), then the thermostat: one call
            if rec:
                i = vr.info()
                log.append((step, epot_now(e123), i['k_after'], vr.temperature(), i['heat']))
            continue
        lv.kick(pos, vel, grad, want_ekin=rec)                         # B: v(t + h)
        if rec:
            log.append((step, epot_now(e123), lv.kinetic_energy(), lv.temperature()))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    for (s, ep, ek, tk, *heat) in log:
        print('step %5d  Epot %14.4f  Ekin %12.4f  T_kin %8.2f' % (s, ep, ek, tk)
              + ('  conserved %14.4f' % (ep + ek - heat[0]) if heat else ''))
    ns_day = opt.steps * h * 1e-6 / wall * 86400.0
    if opt.pol:
        print('\n'.join(w.scf_lines()))
        print('# SCF forms over the run (real dynamics): %s' % pme.scf_stats())
    for line in w.dipole_lines() + w.rdf_lines() + w.msd_lines():
        print(line)
    tk = np.array([r[3] for r in log if r[0] >= opt.steps // 2])
    if vr:
        print('# %d waters, %s, %s, dt %.2f fs, velocity rescaling %.1f K, tau %g fs, seed %d: T_kin over the second half mean '
              '%.1f K std %.1f K (%d records); conserved quantity drift %s; %.3f ms/step, %.2f ns/day (all terms, list rebuilt '
              'every %d steps)'
              % (n_mol, 'polarizable' if opt.pol else 'fixed multipoles', settings.PRECISION, h, opt.temp, opt.tau_t, opt.seed,
                 tk.mean(), tk.std(), len(tk), drift_of(log), wall / opt.steps * 1e3, ns_day, opt.rebuild))
        return
    print('# %d waters, %s, %s, dt %.2f fs, Langevin %.1f K, friction %g /fs, seed %d: T_kin over the second half mean %.1f K '
          'std %.1f K (%d records); %.3f ms/step, %.2f ns/day (all terms, list rebuilt every %d steps)'
          % (n_mol, 'polarizable' if opt.pol else 'fixed multipoles', settings.PRECISION, h, opt.temp, opt.friction, opt.seed,
             tk.mean(), tk.std(), len(tk), wall / opt.steps * 1e3, ns_day, opt.rebuild))


if __name__ == '__main__':
    main()
