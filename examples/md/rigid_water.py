#!/usr/bin/env python
"""Rigid-water loop on the potential of nve_water.py: the O-H stretch (period about 10 fs), which holds nve_water.py at 0.5 fs,
is removed by distance constraints -- O-H, O-H and H-H = 2 r0 sin(theta0 / 2), no bonded terms at all -- so that --dt 2 needs no
force split (mts_water.py).  Constrained BAOAB (admp_amd.md.Constraints / ConstrainedLangevin: SHAKE on the step's displacement
and RATTLE on the velocities, one kernel per half step, whole molecules resident in LDS), so a step launches what a step of
nve_water.py launches, with the two half-step kernels replaced by the two constrained ones and without the bonded kernel.
--friction 0 (the default) is RATTLE velocity Verlet; with --friction the O step carries the Langevin thermostat at --temp with
the noise of --seed.  --bonds-only constrains the two O-H bonds only and keeps the harmonic angle (admp_amd.md.HarmonicBonded).

    python examples/md/rigid_water.py [--dt 2] [--bonds-only] [--friction 0] [--seed 1] [--tol T] [the arguments of nve_water.py]
                                      [--thermostat {langevin,vrescale}] [--tau-t 100] [--dipoles N] [--rdf N [--rdf-out FILE]]
                                    [--msd N [--msd-lags L] [--msd-out FILE]]

--thermostat vrescale keeps the friction at 0 and applies stochastic velocity rescaling (admp_amd.md.VRescale over the constrained
degrees of freedom) after the RATTLE kick of every step: one factor for all velocities leaves them on the constraints.  The log
then carries the conserved quantity E_pot + E_kin - heat and the final line its drift.

Start: the flexible minimisation of the other drivers, the positions projected onto the constraints, Maxwell-Boltzmann
velocities projected likewise and rescaled to --temp over the constrained degrees of freedom."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from water_md import MASS, add_arguments, add_thermostat_arguments, drift_of, setup, rigid_start      # noqa: E402
from admp_amd import settings                                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    add_arguments(ap)
    ap.set_defaults(dt=2.0, rebuild=5)      # the lists are rebuilt every 10 fs (nve_water.py: 10 steps of 0.5 fs)
    ap.add_argument('--bonds-only', action='store_true', help='constrain the O-H bonds only; the angle stays harmonic')
    ap.add_argument('--friction', type=float, default=0.0, help='1/fs (0: constant energy)')
    ap.add_argument('--seed', type=int, default=1, help='of the start velocities and the thermostat\'s noise')
    ap.add_argument('--tol', type=float, default=0.0, help='relative tolerance of the constraints (0: 1e-8 in double, 1e-6 in single)')
    add_thermostat_arguments(ap)
    opt = ap.parse_args()
    if opt.thermostat == 'vrescale' and opt.friction != 0.0:
        ap.error('--thermostat vrescale runs at --friction 0')
    w = setup(opt)
    n_mol, box = w.n_mol, w.box
    nbl, state, pme = w.nbl, w.state, w.pme
    rs = rigid_start(w, opt, np.tile(MASS, n_mol))      # constraints, integrator, gradient closure; the start on the constraints
    con, integ, tol, gradient, epot_now, constraint_error = rs.con, rs.integ, rs.tol, rs.gradient, rs.epot_now, rs.constraint_error
    pos, vel, pairs_l, e123, grad = rs.pos, rs.vel, rs.pairs, rs.e123, rs.grad
    w.start_aspc()                                                     # --aspc: every polarizable call is a time step from here
    h = opt.dt
    vr = None
    if opt.thermostat == 'vrescale':
        from admp_amd.md import VRescale
        vr = VRescale(con, np.tile(MASS, n_mol), h, opt.temp, opt.tau_t, opt.seed, n_dof=rs.n_dof)
    log = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(opt.steps):
        integ.kick_drift(pos, vel, grad, box)                              # B, A-O-A, SHAKE: one kernel
        if (step + 1) % opt.rebuild == 0:
            pairs_l = nbl.allocate(pos)
        if opt.prune and (step + 1) % opt.prune == 0:
            nbl.prune(pos)
        e123, grad = gradient(pos, pairs_l)
        w.record_dipoles(step, pos)                                        # --dipoles: two small kernels, nothing read back
        w.record_rdf(step, pos)                                            # --rdf: one C call, integer counters, nothing read back
        w.record_msd(step, pos, vel)                                       # --msd: one C call, sums in double on the device, nothing read back
        rec = step % opt.log == 0 or step == opt.steps - 1
        integ.kick(pos, vel, grad, box, want_ekin=rec and not vr)          # B, RATTLE: one kernel
        if vr:
            vr.apply(vel)                                                  # the thermostat: sums, then one factor for all
            if rec:
                i = vr.info()
                epot = epot_now(e123)
                log.append((step, epot, i['k_after'], epot + i['k_after'] - i['heat'], vr.temperature(), constraint_error(pos), i['heat']))
        elif rec:
            epot, ekin = epot_now(e123), integ.kinetic_energy()
            log.append((step, epot, ekin, epot + ekin, integ.temperature(), constraint_error(pos)))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    e0 = log[0][3]
    for (s, ep, ek, et, tk, ce, *heat) in log:
        print('step %5d  Epot %14.4f  Ekin %12.4f  %s %14.4f  drift %+.3e  T %7.2f  constraints %.2e' % (s, ep, ek, 'conserved' if heat else 'Etot', et, (et - e0) / abs(e0), tk, ce))
    ns_day = opt.steps * h * 1e-6 / wall * 86400.0
    if opt.pol:
        print('\n'.join(w.scf_lines()))
        print('# SCF forms over the run (real dynamics): %s' % pme.scf_stats())
    for line in w.dipole_lines() + w.rdf_lines() + w.msd_lines():
        print(line)
    info = con.plan_info()
    print('# constraints: %d tiles of at most %d atoms, %d B of LDS per workgroup, most sweeps of a cluster %d; '
          'largest constraint error %.3e (tolerance %.1e); failures %d' % (info['tiles'], info['tile_atoms'], info['lds_bytes'],
                                                                            con.max_sweeps_seen(), max(x[5] for x in log), tol, con.failures()))
    print('# %d waters, %s, %s, dt %.2f fs: %.3f ms/step, %.2f ns/day (all terms, list rebuilt every %d steps); '
          'relative energy drift %.2e, T_final %.1f K'
          % (n_mol, 'polarizable' if opt.pol else 'fixed multipoles', settings.PRECISION, h, wall / opt.steps * 1e3, ns_day,
             opt.rebuild, (log[-1][3] - e0) / abs(e0), log[-1][4])
          + ('; velocity rescaling %.1f K, tau %g fs: conserved quantity drift %s, heat %+.4f kJ/mol'
             % (opt.temp, opt.tau_t, drift_of(log, lambda r: r[3]), log[-1][6]) if vr else ''))


if __name__ == '__main__':
    main()
