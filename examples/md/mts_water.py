#!/usr/bin/env python
"""Multiple-time-step loop (impulse r-RESPA with two levels, OpenMM's MTSLangevinIntegrator) on the potential of nve_water.py:
the harmonic bonds and angles, whose O-H stretch (period about 10 fs) is what holds nve_water.py at 0.5 fs, advance by --inner
BAOAB steps of --dt / --inner inside ONE kernel with whole molecules resident in LDS (admp_amd.md.MTSLangevin, admp_md_mts_step);
the multipolar PME, the dispersion PME and the Tang-Toennies pairs are evaluated once per outer step --dt.  An outer step
launches what a step of nve_water.py launches, less the bonded kernel.  --friction 0 (the default) is NVE; with --friction the
inner steps carry the Langevin thermostat at --temp with the noise of --seed.

    python examples/md/mts_water.py [--dt 2] [--inner 4] [--friction 0] [--seed 1] [the arguments of nve_water.py]
                                    [--thermostat {langevin,vrescale}] [--tau-t 100]

--thermostat vrescale keeps the friction at 0 and makes the closing outer half kick and stochastic velocity rescaling
(admp_amd.md.VRescale) one C call per outer step; the log then carries the conserved quantity E_pot + E_kin - heat.

The same minimisation, start velocities and summary line as nve_water.py, so the two can be compared run for run."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from water_md import KB, MASS, add_arguments, add_thermostat_arguments, drift_of, setup, minimize      # noqa: E402
from admp_amd import settings                                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    add_arguments(ap)
    ap.set_defaults(dt=2.0, rebuild=5)      # outer steps: the lists are rebuilt every 10 fs (nve_water.py: 10 steps of 0.5 fs)
    ap.add_argument('--inner', type=int, default=4, help='inner steps on the bonded terms per outer step --dt')
    ap.add_argument('--friction', type=float, default=0.0, help='1/fs (0: constant energy)')
    ap.add_argument('--seed', type=int, default=1, help='of the thermostat\'s noise')
    add_thermostat_arguments(ap)
    opt = ap.parse_args()
    if opt.thermostat == 'vrescale' and opt.friction != 0.0:
        ap.error('--thermostat vrescale runs at --friction 0')
    w = setup(opt)
    from admp_amd.md import MTSLangevin, VRescale
    n_mol, pos, mass, dt, dev, pme, bond, box = w.n_mol, w.pos, w.mass, w.dtype, 'cuda', w.pme, w.bond, w.box
    nbl, forces, epot_now, state = w.nbl, w.forces, w.epot_now, w.state

    g = torch.Generator(device=dev).manual_seed(1)
    vel = torch.randn(pos.shape, generator=g, device=dev, dtype=dt) * torch.sqrt(KB * opt.temp / mass) * 1e-2
    h = opt.dt
    mts = MTSLangevin(bond, np.tile(MASS, n_mol), h, opt.inner, opt.temp, opt.friction, opt.seed)
    vr = opt.thermostat == 'vrescale' and VRescale(bond, np.tile(MASS, n_mol), h, opt.temp, opt.tau_t, opt.seed)
    pos, pairs, e123, grad = minimize(w, opt, pos)
    w.start_aspc()                                                     # --aspc: every polarizable call is a time step from here
    e123, grad = forces(pos, pairs, bonded=False)                      # the slow gradient: the calculators alone
    vel = vel.contiguous()
    log = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(opt.steps):
        bond.reset_energy()
        mts.kick_drift(pos, vel, grad, box)                            # the slow half kick and the whole inner loop: one kernel
        if (step + 1) % opt.rebuild == 0:
            pairs = nbl.allocate(pos)
        if opt.prune and (step + 1) % opt.prune == 0:
            nbl.prune(pos)
        e123, grad = forces(pos, pairs, bonded=False)
        w.record_dipoles(step, pos)                                    # --dipoles: two small kernels, nothing read back
        w.record_rdf(step, pos)                                        # --rdf: one C call, integer counters, nothing read back
        w.record_msd(step, pos, vel)                                   # --msd: one C call, sums in double on the device, nothing read back
        rec = step % opt.log == 0 or step == opt.steps - 1
        if vr:
            vr.kick(vel, grad)                                         # v(t + h), then the thermostat: one call
            if rec:
                i = vr.info()
                epot = epot_now(e123)
                log.append((step, epot, i['k_after'], epot + i['k_after'] - i['heat'], i['heat']))
            continue
        mts.kick(pos, vel, grad, want_ekin=rec)                        # v(t + h)
        if rec:
            epot, ekin = epot_now(e123), mts.kinetic_energy()          # (the bonded words are the kernel's, at the new positions)
            log.append((step, epot, ekin, epot + ekin))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    e0 = log[0][3]
    for (s, ep, ek, et, *heat) in log:
        print('step %5d  Epot %14.4f  Ekin %12.4f  %s %14.4f  drift %+.3e' % (s, ep, ek, 'conserved' if heat else 'Etot', et, (et - e0) / abs(e0)))
    ns_day = opt.steps * h * 1e-6 / wall * 86400.0
    if opt.pol:
        print('\n'.join(w.scf_lines()))
        print('# SCF forms over the run (real dynamics): %s' % pme.scf_stats())
    for line in w.dipole_lines() + w.rdf_lines() + w.msd_lines():
        print(line)
    info = mts.plan_info()
    print('# multiple time steps: %d tiles of at most %d atoms, %d B of LDS per workgroup' % (info['tiles'], info['tile_atoms'],
                                                                                           info['lds_bytes']))
    print('# %d waters, %s, %s, dt %.2f fs: %.3f ms/step, %.2f ns/day (all terms, list rebuilt every %d steps); '
          'relative energy drift %.2e, T_final %.1f K; inner step %.3f fs (%d per outer step)'
          % (n_mol, 'polarizable' if opt.pol else 'fixed multipoles', settings.PRECISION, h, wall / opt.steps * 1e3, ns_day,
             opt.rebuild, (log[-1][3] - e0) / abs(e0), 2 * log[-1][2] / (3 * 3 * n_mol * KB), h / opt.inner, opt.inner)
          + ('; velocity rescaling %.1f K, tau %g fs: conserved quantity drift %s, heat %+.4f kJ/mol'
             % (opt.temp, opt.tau_t, drift_of(log, lambda r: r[3]), log[-1][4]) if vr else ''))


if __name__ == '__main__':
    main()
