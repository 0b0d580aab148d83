"""One `CorrelationRecorder.record` (admp_md_tcf) with a full ring of 512 lags at 3072 atoms and at 98 304 atoms, O and H of
water, in both precisions, next to

  * one `VelocityVerlet.kick` of the same system, the cheapest thing a step launches anyway, and
  * the same sums written in torch over the same ring: the ring's d rows minus the current frame's, squared and summed per type,
    and the v rows times the current frame's, all in double, added to an accumulator (the push is not included).

Microseconds per call from device events around back-to-back calls through the Python classes, so the figures include the host's
share of a call (20 warm-up calls, median [min, max] of 5 batches), and the bytes the lag kernel must read per record --
lags x n_slots x 6 x sizeof(real): every ring word of the lags in play once -- divided by the time of a record.  The kicks
alternate in sign, so nothing grows; the recorded frame does not move, which changes no load or store of the kernels.

    python tools/tcf_bench.py [waters ...]          (default: 1024 32768, i.e. 3072 and 98 304 atoms)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admp_amd import settings, systems as S                                # noqa: E402
from tools.md_mts_bench import timed                                       # noqa: E402

MASS = (15.999, 1.008, 1.008)
N_LAGS = 512


def torch_sums(ring, cur_slot, bounds, acc):
    """ring (L, 2, 3, n_slots); bounds: the slot range of every type; acc (2, n_types, L) double"""
    cur = ring[cur_slot].double()
    dd = ring[:, 0].double() - cur[0]
    msd = (dd * dd).sum(dim=1)
    vacf = (ring[:, 1].double() * cur[1]).sum(dim=1)
    for a, (lo, hi) in enumerate(bounds):
        acc[0, a] += msd[:, lo:hi].sum(dim=1)
        acc[1, a] += vacf[:, lo:hi].sum(dim=1)


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [1024, 32768]
    for prec in ('double', 'single'):
        settings.PRECISION = prec
        from admp_amd.md import CorrelationRecorder, HarmonicBonded, VelocityVerlet
        for n_mol in sizes:
            pos, box = S.synthetic_water_box(n_mol, seed=20240)
            n = 3 * n_mol
            o = HarmonicBonded(n, [], [], [], [])
            dev = lambda a: torch.as_tensor(np.asarray(a), dtype=o._dtype, device=o._device).contiguous()      # noqa: E731
            rng = np.random.default_rng(5)
            r, v, g = dev(pos), dev(rng.normal(size=(n, 3)) * 1e-2), dev(rng.normal(size=(n, 3)) * 50.0)
            rec = CorrelationRecorder(o, np.tile([0, 1, 1], n_mol), N_LAGS, 1.0, max_ring_bytes=2 ** 33)
            vv = VelocityVerlet(o, np.tile(MASS, n_mol), 0.5)
            k = [0]

            def record():
                rec.record(r, v, box)

            def kick():
                k[0] += 1
                vv.dt = 0.5 if k[0] & 1 else -0.5
                vv.kick(r, v, g)
            for _ in range(N_LAGS):                                         # a full ring before anything is timed
                record()
            ring = rec._ring.view(N_LAGS, 2, 3, rec.n_slots)
            n_o = -(-n_mol // rec.tile_atoms) * rec.tile_atoms
            bounds = [(0, n_o), (n_o, rec.n_slots)]
            acc = torch.zeros(2, 2, N_LAGS, dtype=torch.float64, device=o._device)
            reps = 100 if n <= 4096 else 20
            item = ring.element_size()
            moved = N_LAGS * rec.n_slots * 6 * item

            runs = [('VelocityVerlet.kick', kick, 200), ('CorrelationRecorder.record', record, reps)]
            runs.append(('torch sums over the ring', lambda: torch_sums(ring, 0, bounds, acc), 10))
            for label, fn, nrep in runs:
                t = timed(fn, nrep)
                extra = ''
                if fn is record:
                    i = rec.info()
                    extra = ('   %d workgroups of %d lags, %.1f MB of ring read per record: %.0f GB/s'
                             % (i['workgroups'], i['lags_per_workgroup'], moved / 1e6, moved / (t[0] * 1e-6) / 1e9))
                print('%s %7d atoms %-27s %10.2f us [%.2f, %.2f]%s' % ((prec, n, label) + t + (extra,)), flush=True)
            s = rec.sums()
            assert rec.info()['large_jumps'] == 0 and (s['msd'] == 0).all() and (s['vacf'][:, 0] > 0).all()      # (the frame never moves)
            del rec, ring, acc
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
