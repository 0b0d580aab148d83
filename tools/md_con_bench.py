"""The two constrained half-step kernels alone (admp_amd.md.ConstrainedLangevin.kick_drift = admp_md_con_step, .kick =
admp_md_con_kick) on a box of rigid waters, per size, precision, tile capacity and with / without the thermostat's noise, next to
ONE step of the existing unconstrained chain (admp_md_langevin + admp_md_kick_drift).  Microseconds per call from device events
around back-to-back calls (20 warm-up calls, median [min, max] of 5 batches), and the most sweeps any cluster made.  Tolerance
1e-8 in double, 1e-6 in single (the defaults of examples/md/rigid_water.py); zero gradient, so the molecules translate and turn.

    python tools/md_con_bench.py [atoms ...]          (default: 648 98304 1048575)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admp_amd import settings                                              # noqa: E402
from admp_amd.md import Constraints, ConstrainedLangevin, Langevin         # noqa: E402
from tools.md_mts_bench import R0, TH0, system, timed                      # noqa: E402


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [648, 98304, 1048575]
    for prec in ('double', 'single'):
        settings.PRECISION = prec
        tol = 1e-8 if prec == 'double' else 1e-6
        for n_atoms in sizes:
            r, v, mass, _, _, box = system(n_atoms)
            n_mol = n_atoms // 3
            a = 3 * np.arange(n_mol)
            pairs = np.stack([np.stack([a, a + 1], 1), np.stack([a, a + 2], 1), np.stack([a + 1, a + 2], 1)], axis=1).reshape(-1, 2)
            lengths = np.tile([R0, R0, 2.0 * R0 * np.sin(0.5 * TH0)], n_mol)
            reps = 400 if n_atoms < 500000 else 100
            first = True
            for cap in (64, 128, 256):
                c = Constraints(3 * n_mol, pairs, lengths, mass[:3 * n_mol], tolerance=tol, tile_atoms=cap)
                rd = torch.as_tensor(r[:3 * n_mol], dtype=c._dtype, device=c._device).contiguous()
                vd = torch.as_tensor(v[:3 * n_mol], dtype=c._dtype, device=c._device).contiguous()
                g = torch.zeros_like(rd)
                if first:
                    lv = Langevin(c, mass[:3 * n_mol], 2.0, 300.0, 0.05, 1)

                    def chain():
                        lv.kick_drift(rd, vd, g)
                        lv.kick(rd, vd, g)
                    print('%s n %7d existing chain (langevin + kick, one unconstrained step): %.2f us [%.2f, %.2f]'
                          % ((prec, n_atoms) + timed(chain, reps)), flush=True)
                    first = False
                for gamma in (0.0, 0.05):
                    rd.copy_(torch.as_tensor(r[:3 * n_mol]))
                    vd.copy_(torch.as_tensor(v[:3 * n_mol]))
                    c.project_positions(rd, box)
                    c.project_velocities(rd, vd, box, 2.0)
                    c.reset_failures()
                    integ = ConstrainedLangevin(c, 2.0, 300.0, gamma, 1)
                    info = c.plan_info()
                    def both():      # (a kick repeated on its own output would find every constraint converged)
                        integ.kick_drift(rd, vd, g, box)
                        integ.kick(rd, vd, g, box)
                    t_step = timed(lambda: integ.kick_drift(rd, vd, g, box), reps)
                    t_both = timed(both, reps)
                    print('%s n %7d cap %3d gamma %.2f tiles %6d lds %5d B: step %.2f us [%.2f, %.2f]; step + kick %.2f us [%.2f, %.2f]; '
                          'most sweeps %d, failures %d' % ((prec, n_atoms, cap, gamma, info['tiles'], info['lds_bytes']) + t_step + t_both
                                                          + (c.max_sweeps_seen(), c.failures())), flush=True)
                    assert torch.isfinite(rd).all()


if __name__ == '__main__':
    main()
