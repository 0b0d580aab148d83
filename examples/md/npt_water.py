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

The other arguments are those of nve_water.py.  Isotropic scaling of the atoms only (no molecular scaling, one rank).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from water_md import MASS, add_arguments, setup, minimize      # noqa: E402
from admp_amd import settings                                  # noqa: E402

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
    opt = ap.parse_args()
    if opt.nbaro < 1:
        ap.error('--nbaro must be at least 1')
    w = setup(opt)
    from admp_amd.md import CRescaleBarostat, Langevin, maxwell_boltzmann
    n_mol, pme, nbl, forces, epot_now, state, box = w.n_mol, w.pme, w.nbl, w.forces, w.epot_now, w.state, w.box
    masses = np.tile(MASS, n_mol)
    h = opt.dt
    # units: A, fs, amu, kJ/mol; pressures in bar
    vel = maxwell_boltzmann(pme, masses, opt.temp, opt.seed)
    lv = Langevin(pme, masses, h, opt.temp, opt.friction, opt.seed)
    baro = CRescaleBarostat(pme, masses, opt.nbaro * h, opt.temp, opt.pressure, opt.tau_p, opt.compress, opt.seed)
    pos, pairs, e123, grad = minimize(w, opt, w.pos)
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
        baro_now = (step + 1) % opt.nbaro == 0
        rec = baro_now and (step // opt.nbaro % max(opt.log // opt.nbaro, 1) == 0 or step + opt.nbaro >= opt.steps)
        lv.kick(pos, vel, grad, want_ekin=rec)                         # B: v(t + h)
        if baro_now:
            dbox = w.box_gradient(pos, pairs)                          # four evaluations at the current positions and list
            kin, rg, xi = baro.sums(pos, vel, grad)                    # one launch, one host read
            p_inst = baro.pressure(box, dbox, kin, rg)
            if rec:
                log.append((step, epot_now(e123), lv.temperature(), p_inst, abs(float(np.linalg.det(box)))))
            baro.apply(pos, vel, box, p_inst, xi)                      # r, v and the cell (in place: the closures hold `box`)
            pairs = nbl.allocate(pos)
            e123, grad = forces(pos, pairs)                            # the next kick takes the scaled configuration's gradients
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    m_tot = float(masses.sum())
    for (s, ep, tk, p, v) in log:
        print('step %5d  Epot %14.4f  T_kin %8.2f  P_inst %12.2f  V %14.4f  density %7.4f'
              % (s, ep, tk, p, v, m_tot / v * G_CM3_PER_AMU_A3))
    ns_day = opt.steps * h * 1e-6 / wall * 86400.0
    if opt.pol:
        print('# mean SCF cycles per evaluation (thresh %g): %.1f' % (settings.POL_CONV, state['cyc'] / state['n']))
        print('# SCF forms over the run (real dynamics): %s' % pme.scf_stats())
    half = [r for r in log if r[0] >= opt.steps // 2]
    tk, pp, vv = (np.array([r[k] for r in half]) for k in (2, 3, 4))
    print('# %d waters, %s, %s, dt %.2f fs, Langevin %.1f K, friction %g /fs, seed %d, barostat %.1f bar, tau_p %g fs, every %d '
          'steps: over the second half T_kin mean %.1f K, P mean %.1f bar std %.1f bar, V mean %.2f A^3 std %.2f A^3 (%d records), '
          'V_final %.4f A^3; %.3f ms/step, %.2f ns/day (all terms, list rebuilt every %d steps and after each rescaling)'
          % (n_mol, 'polarizable' if opt.pol else 'fixed multipoles', settings.PRECISION, h, opt.temp, opt.friction, opt.seed,
             opt.pressure, opt.tau_p, opt.nbaro, tk.mean(), pp.mean(), pp.std(), vv.mean(), vv.std(), len(half),
             abs(float(np.linalg.det(box))), wall / opt.steps * 1e3, ns_day, opt.rebuild))


if __name__ == '__main__':
    main()
