#!/usr/bin/env python
"""Langevin NPT loop on the full MPID-style water potential: the loop of nvt_water.py (BAOAB, water_md.py) under the isotropic
barostat of admp_amd/md.py (stochastic cell rescaling, Bernetti and Bussi 2020).  Every --nbaro steps, after the closing kick,
the driver sums dE/dbox over the four calculators (PME, dispersion PME, Tang-Toennies pairs, bonded terms: box_gradient of
water_md.py), reads the two 3x3 sums of the pressure and the barostat's normal from one launch (admp_md_virial), rescales
positions, velocities (admp_md_scale) and the cell, rebuilds the neighbour list and evaluates the forces again, so that the
next kick uses the gradients of the scaled configuration.  The noise is a function of (seed, application) alone (stream 2 of
the thermostat's generator): a run restarted at any step repeats it.

    python examples/md/npt_water.py [--waters 1024] [--steps 200] [--dt 0.5] [--temp 300] [--friction 0.05] [--seed 1]
                                    [--pressure 1] [--tau-p 1000] [--compress 4.5e-5] [--nbaro 10] [--pol] [--single] [--mesh K]
                                    [--molecular | --rigid [--bonds-only] [--tol T]]
                                    [--thermostat {langevin,vrescale}] [--tau-t 100] [--dipoles N] [--rdf N [--rdf-out FILE]]
                                    [--msd N [--msd-lags L] [--msd-out FILE]]

The other arguments are those of nve_water.py.  Without --molecular or --rigid: isotropic scaling of the atoms only (one rank).
--molecular: the same flexible water, but whole molecules are scaled about their centres of mass and the pressure is the
molecular one (admp_amd.md.MolecularCRescaleBarostat: admp_md_mol_sums, admp_md_mol_scale).  --rigid: the rigid water of
rigid_water.py (constrained BAOAB, admp_amd.md.Constraints / ConstrainedLangevin; --bonds-only and --tol as there) under the
molecular barostat, default --dt 2 with the lists rebuilt every 5 steps: a molecule moves rigidly in an application, so the
constraints survive it without a re-projection -- the largest constraint error right after the application is logged with
every record.  --thermostat vrescale replaces the friction (then 0) by stochastic velocity rescaling (admp_amd.md.VRescale,
relaxation time --tau-t), the thermostat the barostat was published with: the closing kick and the thermostat are one C call
(--rigid: the thermostat follows the RATTLE kick).  The log then carries E_pot + E_kin - heat, which the thermostat conserves
and only the barostat's work moves.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from water_md import MASS, add_arguments, add_thermostat_arguments, drift_of, setup, minimize, rigid_start      # noqa: E402
from admp_amd import settings                                               # noqa: E402

G_CM3_PER_AMU_A3 = 1.66053907      # 1 amu/A^3 in g/cm^3


def main():
    ap = argparse.ArgumentParser()
    add_arguments(ap)
    ap.add_argument('--friction', type=float, default=0.05, help='1/fs')
    ap.add_argument('--seed', type=int, default=1, help='of the initial velocities and of the noise of thermostat and barostat')
    ap.add_argument('--pressure', type=float, default=1.0, help='bar')
    ap.add_argument('--tau-p', type=float, default=1000.0, help='relaxation time of the barostat, fs')
    ap.add_argument('--compress', type=float, default=4.5e-5, help='isothermal compressibility, 1/bar')
    ap.add_argument('--nbaro', type=int, default=10, help='steps between applications of the barostat')
    ap.add_argument('--molecular', action='store_true', help='scale whole molecules about their centres of mass; molecular pressure')
    ap.add_argument('--rigid', action='store_true', help='rigid water (constrained BAOAB) under the molecular barostat; default --dt 2')
    ap.add_argument('--bonds-only', action='store_true', help='with --rigid: constrain the O-H bonds only; the angle stays harmonic')
    ap.add_argument('--tol', type=float, default=0.0, help='with --rigid: relative tolerance of the constraints (0: 1e-8 in double, '
                    '1e-6 in single)')
    ap.set_defaults(dt=None, rebuild=None)      # resolved below: they depend on --rigid
    add_thermostat_arguments(ap)
    opt = ap.parse_args()
    if opt.thermostat == 'vrescale':
        opt.friction = 0.0
    if opt.dt is None:
        opt.dt = 2.0 if opt.rigid else 0.5
    if opt.rebuild is None:
        opt.rebuild = 5 if opt.rigid else 10      # as rigid_water.py: the lists are rebuilt every 10 fs
    if opt.nbaro < 1:
        ap.error('--nbaro must be at least 1')
    if opt.molecular and opt.rigid:
        ap.error('--rigid implies molecular scaling: give one of --molecular and --rigid')
    if (opt.bonds_only or opt.tol) and not opt.rigid:
        ap.error('--bonds-only and --tol belong to --rigid')
    w = setup(opt)
    from admp_amd.md import CRescaleBarostat, Langevin, MolecularCRescaleBarostat, VRescale, groups_of, maxwell_boltzmann
    n_mol, pme, nbl, forces, epot_now, state, box = w.n_mol, w.pme, w.nbl, w.forces, w.epot_now, w.state, w.box
    masses = np.tile(MASS, n_mol)
    h = opt.dt
    # units: A, fs, amu, kJ/mol; pressures in bar
    con = angle = constraint_error = None
    if opt.rigid:
        rs = rigid_start(w, opt, masses)      # constraints, integrator, gradient closure; positions and velocities on the constraints
        con, angle, lv, forces, epot_now, constraint_error = rs.con, rs.angle, rs.integ, rs.gradient, rs.epot_now, rs.constraint_error
        pos, vel, pairs, e123, grad = rs.pos, rs.vel, rs.pairs, rs.e123, rs.grad
        baro = MolecularCRescaleBarostat(con, masses, groups_of(3 * n_mol, constraints=con), opt.nbaro * h, opt.temp, opt.pressure,
                                         opt.tau_p, opt.compress, opt.seed)
    else:
        vel = maxwell_boltzmann(pme, masses, opt.temp, opt.seed)
        lv = Langevin(pme, masses, h, opt.temp, opt.friction, opt.seed)
        if opt.molecular:
            baro = MolecularCRescaleBarostat(pme, masses, groups_of(3 * n_mol, bonded=w.bond), opt.nbaro * h, opt.temp, opt.pressure,
                                             opt.tau_p, opt.compress, opt.seed)
        else:
            baro = CRescaleBarostat(pme, masses, opt.nbaro * h, opt.temp, opt.pressure, opt.tau_p, opt.compress, opt.seed)
        pos, pairs, e123, grad = minimize(w, opt, w.pos)
    w.start_aspc()                                                     # --aspc: every polarizable call is a time step from here
    vr = opt.thermostat == 'vrescale' and VRescale(con if opt.rigid else pme, masses, h, opt.temp, opt.tau_t, opt.seed,
                                                   n_dof=rs.n_dof if opt.rigid else 3 * len(masses) - 3)
    log, extra = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(opt.steps):
        if con is not None:
            lv.kick_drift(pos, vel, grad, box)                         # B, A-O-A, SHAKE: in place, one kernel
        else:
            lv.kick_drift(pos, vel, grad)                              # B, A, O, A: in place, one kernel
        if (step + 1) % opt.rebuild == 0:
            pairs = nbl.allocate(pos)
        if opt.prune and (step + 1) % opt.prune == 0:
            nbl.prune(pos)
        e123, grad = forces(pos, pairs)
        w.record_dipoles(step, pos)                                    # --dipoles: two small kernels, nothing read back
        w.record_rdf(step, pos)                                        # --rdf: one C call, integer counters, nothing read back
        w.record_msd(step, pos, vel)                                   # --msd: one C call, sums in double on the device, nothing read back
        baro_now = (step + 1) % opt.nbaro == 0
        rec = baro_now and (step // opt.nbaro % max(opt.log // opt.nbaro, 1) == 0 or step + opt.nbaro >= opt.steps)
        if con is not None:
            lv.kick(pos, vel, grad, box, want_ekin=rec and not vr)     # B, RATTLE: v(t + h)
            if vr:
                vr.apply(vel)                                          # the thermostat: one factor for all velocities
        elif vr:
            vr.kick(vel, grad)                                         # B: v(t + h), then the thermostat: one call
        else:
            lv.kick(pos, vel, grad, want_ekin=rec)                     # B: v(t + h)
        if baro_now:
            if con is not None:                                        # the three calculators, and the angle of --bonds-only
                dbox = w.box_gradient(pos, pairs, bonded=False)
                if angle is not None:
                    dbox = dbox + angle.get_box_gradient(pos, box)
            else:
                dbox = w.box_gradient(pos, pairs)                      # four evaluations at the current positions and list
            if con is not None or opt.molecular:
                kin, rg, xi = baro.sums(pos, vel, grad, box)           # one launch, one host read
            else:
                kin, rg, xi = baro.sums(pos, vel, grad)                # one launch, one host read
            p_inst = baro.pressure(box, dbox, kin, rg)
            if rec:
                log.append((step, epot_now(e123), vr.temperature() if vr else lv.temperature(), p_inst, abs(float(np.linalg.det(box)))))
                if vr:
                    i = vr.info()
                    extra.append((step, log[-1][1], i['k_after'], i['heat']))
            baro.apply(pos, vel, box, p_inst, xi)                      # r, v and the cell (in place: the closures hold `box`)
            if rec and con is not None:                                # the constraints in the scaled cell, not re-projected
                log[-1] += (constraint_error(pos),)
            pairs = nbl.allocate(pos)
            w.aspc_jump()                                              # --aspc: the scaled configuration starts a new history
            e123, grad = forces(pos, pairs)                            # the next kick takes the scaled configuration's gradients
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    m_tot = float(masses.sum())
    for k, rec in enumerate(log):
        (s, ep, tk, p, v) = rec[:5]
        print('step %5d  Epot %14.4f  T_kin %8.2f  P_inst %12.2f  V %14.4f  density %7.4f'
              % (s, ep, tk, p, v, m_tot / v * G_CM3_PER_AMU_A3) + ('  constraints %.2e' % rec[5] if con is not None else '')
              + ('  Epot+Ekin-heat %14.4f' % (extra[k][1] + extra[k][2] - extra[k][3]) if vr else ''))
    ns_day = opt.steps * h * 1e-6 / wall * 86400.0
    if opt.pol:
        print('\n'.join(w.scf_lines()))
        print('# SCF forms over the run (real dynamics): %s' % pme.scf_stats())
    for line in w.dipole_lines() + w.rdf_lines() + w.msd_lines():
        print(line)
    if con is not None or opt.molecular:
        info = baro.plan_info()
        print('# molecular scaling: %d groups in %d tiles of at most %d atoms, %d B of LDS per workgroup'
              % (info['groups'], info['tiles'], info['tile_atoms'], info['lds_bytes']))
    if con is not None:
        print('# constraints: largest constraint error %.3e at a record, %.3e at the end (tolerance %.1e, no re-projection in the '
              'loop); most sweeps of a cluster %d; failures %d'
              % (max(r[5] for r in log), constraint_error(pos), con.tolerance, con.max_sweeps_seen(), con.failures()))
    half = [r for r in log if r[0] >= opt.steps // 2]
    tk, pp, vv = (np.array([r[k] for r in half]) for k in (2, 3, 4))
    if vr:
        print('# velocity rescaling %.1f K, tau %g fs in place of the friction: E_pot + E_kin - heat moved by %s (the barostat\'s '
              'work), heat %+.4f kJ/mol' % (opt.temp, opt.tau_t, drift_of(extra), extra[-1][3]))
    print('# %d waters, %s, %s, dt %.2f fs, Langevin %.1f K, friction %g /fs, seed %d, barostat %.1f bar, tau_p %g fs, every %d '
          'steps: over the second half T_kin mean %.1f K, P mean %.1f bar std %.1f bar, V mean %.2f A^3 std %.2f A^3 (%d records), '
          'V_final %.4f A^3; %.3f ms/step, %.2f ns/day (all terms, list rebuilt every %d steps and after each rescaling)'
          % (n_mol, 'polarizable' if opt.pol else 'fixed multipoles', settings.PRECISION, h, opt.temp, opt.friction, opt.seed,
             opt.pressure, opt.tau_p, opt.nbaro, tk.mean(), pp.mean(), pp.std(), vv.mean(), vv.std(), len(half),
             abs(float(np.linalg.det(box))), wall / opt.steps * 1e3, ns_day, opt.rebuild))


if __name__ == '__main__':
    main()
