"""One `DipoleRecorder.record` (admp_pme_dipoles = k_dipole_groups + k_dipole_fold) next to one `VelocityVerlet.kick`, the
cheapest thing a step launches anyway, per size and precision, on boxes of water (one group per molecule).  Microseconds per call
from device events around back-to-back calls through the Python classes, so the figures include the host's share of a call (20
warm-up calls, median [min, max] of 5 batches).  The kicks alternate in sign, so nothing grows.

    python tools/dipole_bench.py [waters ...]          (default: 1024, i.e. 3072 atoms)
"""
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admp_amd import settings, systems as S                                # noqa: E402
from tools.md_mts_bench import timed                                       # noqa: E402

MASS = (15.999, 1.008, 1.008)


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [1024]
    for prec in ('double', 'single'):
        settings.PRECISION = prec
        from admp_amd.md import DipoleRecorder, VelocityVerlet
        from admp_amd.pme import ADMPPmeForce
        for n_mol in sizes:
            pos, box = S.synthetic_water_box(n_mol, seed=20240)
            at, ai, _ = S.water_topology(n_mol)
            n = 3 * n_mol
            pme = ADMPPmeForce(box, at, ai, sp.csr_matrix((n, n), dtype=np.int32), 4.0, 1e-4, 2, lpol=False)
            dev = lambda a: torch.as_tensor(np.asarray(a), dtype=pme._dtype, device=pme._device).contiguous()      # noqa: E731
            rng = np.random.default_rng(5)
            r, Q = dev(pos), dev(S.water_parameters(n_mol)['Q_local'])
            U, v, g = dev(rng.normal(size=(n, 3)) * 0.05), dev(rng.normal(size=(n, 3)) * 1e-2), dev(rng.normal(size=(n, 3)) * 50.0)
            masses = np.tile(MASS, n_mol)
            reps = 400
            rec = DipoleRecorder(pme, np.repeat(np.arange(n_mol), 3), masses, 25 * reps)
            vv = VelocityVerlet(pme, masses, 0.5)
            k = [0]

            def record():
                rec.record(r, box, Q, U)

            def kick():
                k[0] += 1
                vv.dt = 0.5 if k[0] & 1 else -0.5
                vv.kick(r, v, g)
            for label, fn in (('VelocityVerlet.kick', kick), ('DipoleRecorder.record', record)):
                t = timed(fn, reps)
                print('%s %7d atoms %-22s %8.2f us [%.2f, %.2f]' % ((prec, n, label) + t), flush=True)
            rows = rec.rows()
            assert rows.shape == (20 + 5 * reps, 16) and np.isfinite(rows).all() and (rows == rows[0]).all() and rows[0, 12] == n_mol


if __name__ == '__main__':
    main()
