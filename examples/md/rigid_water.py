#!/usr/bin/env python
"""Rigid-water loop on the potential of nve_water.py: the O-H stretch (period about 10 fs), which holds nve_water.py at 0.5 fs,
is removed by distance constraints -- O-H, O-H and H-H = 2 r0 sin(theta0 / 2), no bonded terms at all -- so that --dt 2 needs no
force split (mts_water.py).  Constrained BAOAB (admp_amd.md.Constraints / ConstrainedLangevin: SHAKE on the step's displacement
and RATTLE on the velocities, one kernel per half step, whole molecules resident in LDS), so a step launches what a step of
nve_water.py launches, with the two half-step kernels replaced by the two constrained ones and without the bonded kernel.
--friction 0 (the default) is RATTLE velocity Verlet; with --friction the O step carries the Langevin thermostat at --temp with
the noise of --seed.  --bonds-only constrains the two O-H bonds only and keeps the harmonic angle (admp_amd.md.HarmonicBonded).

    python examples/md/rigid_water.py [--dt 2] [--bonds-only] [--friction 0] [--seed 1] [--tol T] [the arguments of nve_water.py]

Start: the flexible minimisation of the other drivers, the positions projected onto the constraints, Maxwell-Boltzmann
velocities projected likewise and rescaled to --temp over the constrained degrees of freedom."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from water_md import KB, MASS, R0, K_ANG, TH0, add_arguments, setup, minimize      # noqa: E402
from admp_amd import settings                                                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    add_arguments(ap)
    ap.set_defaults(dt=2.0, rebuild=5)      # the lists are rebuilt every 10 fs (nve_water.py: 10 steps of 0.5 fs)
    ap.add_argument('--bonds-only', action='store_true', help='constrain the O-H bonds only; the angle stays harmonic')
    ap.add_argument('--friction', type=float, default=0.0, help='1/fs (0: constant energy)')
    ap.add_argument('--seed', type=int, default=1, help='of the start velocities and the thermostat\'s noise')
    ap.add_argument('--tol', type=float, default=0.0, help='relative tolerance of the constraints (0: 1e-8 in double, 1e-6 in single)')
    opt = ap.parse_args()
    w = setup(opt)
    from admp_amd.md import Constraints, ConstrainedLangevin, HarmonicBonded, maxwell_boltzmann
    n_mol, pos, dt, box = w.n_mol, w.pos, w.dtype, w.box
    nbl, forces, state, pme = w.nbl, w.forces, w.state, w.pme
    tol = opt.tol or (1e-6 if opt.single else 1e-8)

    o = 3 * np.arange(n_mol)
    pairs = [np.stack([o, o + 1], axis=1), np.stack([o, o + 2], axis=1)]
    lengths = [np.full(n_mol, R0), np.full(n_mol, R0)]
    if not opt.bonds_only:
        pairs.append(np.stack([o + 1, o + 2], axis=1))
        lengths.append(np.full(n_mol, 2.0 * R0 * np.sin(0.5 * TH0)))
    pairs = np.stack(pairs, axis=1).reshape(-1, 2)          # a molecule's constraints side by side
    lengths = np.stack(lengths, axis=1).reshape(-1)
    masses = np.tile(MASS, n_mol)
    con = Constraints(3 * n_mol, pairs, lengths, masses, tolerance=tol)
    angle = None
    if opt.bonds_only:
        angle = HarmonicBonded(3 * n_mol, np.zeros((0, 2)), np.zeros((0, 2)), np.stack([o + 1, o, o + 2], axis=1),
                               np.tile([K_ANG, TH0], (n_mol, 1)))
    integ = ConstrainedLangevin(con, opt.dt, opt.temp, opt.friction, opt.seed)
    n_dof = 9 * n_mol - con.n_constraints
    pi, pj = (torch.as_tensor(pairs[:, k], device='cuda') for k in (0, 1))
    d_t = torch.as_tensor(lengths, dtype=torch.float64, device='cuda')

    def gradient(p, prs):
        """the calculators without the bonded terms, plus the harmonic angle of --bonds-only"""
        e, g = forces(p, prs, bonded=False)
        if angle is not None:
            angle.reset_energy()
            angle.add_forces(p, box, g)
        return e, g

    def epot_now(e):
        return float(e) + (angle.energy() if angle is not None else 0.0)

    def constraint_error(p):
        """largest | |x_j - x_i| - d | / d, minimum image, in double on the device"""
        h = torch.as_tensor(np.asarray(box, dtype=np.float64).reshape(3, 3), device='cuda')
        s = (p[pj].double() - p[pi].double()) @ torch.linalg.inv(h)
        d = ((s - torch.round(s)) @ h).norm(dim=1)
        return float(((d - d_t).abs() / d_t).max())

    pos, pairs_l, _, _ = minimize(w, opt, pos)                              # flexible, as the other drivers
    print('# constraint error before the projection %.3e' % constraint_error(pos))
    con.project_positions(pos, box)
    pairs_l = nbl.allocate(pos)
    e123, grad = gradient(pos, pairs_l)
    vel = maxwell_boltzmann(con, masses, opt.temp, opt.seed)
    con.project_velocities(pos, vel, box, opt.dt)
    m_t = torch.as_tensor(masses, dtype=dt, device='cuda')[:, None]
    t_now = float((m_t * vel * vel).sum()) / ConstrainedLangevin.ACC / (n_dof * KB)
    if t_now > 0:
        vel *= float(np.sqrt(opt.temp / t_now))
    print('# %d constraints (%s), tolerance %.1e; start: constraint error %.3e, T %.1f K over %d degrees of freedom, failures %d'
          % (con.n_constraints, 'O-H bonds, harmonic angle' if opt.bonds_only else 'rigid water', tol, constraint_error(pos),
             opt.temp if t_now > 0 else 0.0, n_dof, con.failures()))
    con.reset_failures()
    h = opt.dt
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
        rec = step % opt.log == 0 or step == opt.steps - 1
        integ.kick(pos, vel, grad, box, want_ekin=rec)                     # B, RATTLE: one kernel
        if rec:
            epot, ekin = epot_now(e123), integ.kinetic_energy()
            log.append((step, epot, ekin, epot + ekin, integ.temperature(), constraint_error(pos)))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    e0 = log[0][3]
    for (s, ep, ek, et, tk, ce) in log:
        print('step %5d  Epot %14.4f  Ekin %12.4f  Etot %14.4f  drift %+.3e  T %7.2f  constraints %.2e' % (s, ep, ek, et, (et - e0) / abs(e0), tk, ce))
    ns_day = opt.steps * h * 1e-6 / wall * 86400.0
    if opt.pol:
        print('# mean SCF cycles per evaluation (thresh %g): %.1f' % (settings.POL_CONV, state['cyc'] / state['n']))
        print('# SCF forms over the run (real dynamics): %s' % pme.scf_stats())
    info = con.plan_info()
    print('# constraints: %d tiles of at most %d atoms, %d B of LDS per workgroup, most sweeps of a cluster %d; '
          'largest constraint error %.3e (tolerance %.1e); failures %d' % (info['tiles'], info['tile_atoms'], info['lds_bytes'],
                                                                            con.max_sweeps_seen(), max(x[5] for x in log), tol, con.failures()))
    print('# %d waters, %s, %s, dt %.2f fs: %.3f ms/step, %.2f ns/day (all terms, list rebuilt every %d steps); '
          'relative energy drift %.2e, T_final %.1f K'
          % (n_mol, 'polarizable' if opt.pol else 'fixed multipoles', settings.PRECISION, h, wall / opt.steps * 1e3, ns_day,
             opt.rebuild, (log[-1][3] - e0) / abs(e0), log[-1][4]))


if __name__ == '__main__':
    main()
