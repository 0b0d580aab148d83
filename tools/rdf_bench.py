"""One `RdfRecorder.record` (admp_md_rdf) at 3072 atoms (the tile form) and at 98 304 atoms (the cell form: binning and
sweep), r_max 10 A and 200 bins, O-O / O-H / H-H with the intramolecular pairs excluded, in both precisions, next to

  * one `VelocityVerlet.kick` of the same system, the cheapest thing a step launches anyway, and
  * at 3072 atoms the plain torch formulation a user would write today: all minimum-image distances as one (n, n) tensor, then
    `bincount` on the device (a host read per frame not included).

Microseconds per call from device events around back-to-back calls through the Python classes, so the figures include the host's
share of a call (20 warm-up calls, median [min, max] of 5 batches).  The kicks alternate in sign, so nothing grows.

    python tools/rdf_bench.py [waters ...]          (default: 1024 32768, i.e. 3072 and 98 304 atoms)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admp_amd import settings, systems as S                                # noqa: E402
from tools.md_mts_bench import timed                                       # noqa: E402

MASS = (15.999, 1.008, 1.008)
R_MAX, N_BINS = 10.0, 200


def torch_rdf(r, box_t, inv_t, types, mol, hist):
    """the frame's counts added to hist (3 x N_BINS int64): every pair twice in an (n, n) tensor, halved by i < j"""
    n = r.shape[0]
    d = r[:, None, :] - r[None, :, :]
    s = d @ inv_t
    d = (s - torch.floor(s + 0.5)) @ box_t
    dist = torch.sqrt((d * d).sum(dim=2))
    i = torch.arange(n, device=r.device)
    keep = (dist < R_MAX) & (i[:, None] < i[None, :]) & (mol[:, None] != mol[None, :])
    ch = types[:, None] + types[None, :]                                   # O-O 0, O-H 1, H-H 2: the channel of two types
    idx = ch * N_BINS + torch.clamp((dist * (N_BINS / R_MAX)).long(), max=N_BINS - 1)
    hist += torch.bincount(idx[keep], minlength=3 * N_BINS)


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [1024, 32768]
    for prec in ('double', 'single'):
        settings.PRECISION = prec
        from admp_amd.md import HarmonicBonded, RdfRecorder, VelocityVerlet
        for n_mol in sizes:
            pos, box = S.synthetic_water_box(n_mol, seed=20240)
            n = 3 * n_mol
            o = HarmonicBonded(n, [], [], [], [])
            dev = lambda a: torch.as_tensor(np.asarray(a), dtype=o._dtype, device=o._device).contiguous()      # noqa: E731
            rng = np.random.default_rng(5)
            r, v, g = dev(pos), dev(rng.normal(size=(n, 3)) * 1e-2), dev(rng.normal(size=(n, 3)) * 50.0)
            types, mol = np.tile([0, 1, 1], n_mol), np.repeat(np.arange(n_mol), 3)
            rec = RdfRecorder(o, types, R_MAX, N_BINS, groups=mol)
            vv = VelocityVerlet(o, np.tile(MASS, n_mol), 0.5)
            k = [0]

            def record():
                rec.record(r, box)

            def kick():
                k[0] += 1
                vv.dt = 0.5 if k[0] & 1 else -0.5
                vv.kick(r, v, g)
            reps = 200 if n <= 4096 else 20
            runs = [('VelocityVerlet.kick', kick, 200), ('RdfRecorder.record', record, reps)]
            if n <= 4096:
                box_t, inv_t = dev(box), dev(np.linalg.inv(np.asarray(box, dtype=np.float64).reshape(3, 3)))
                ty_t, mol_t = torch.as_tensor(types).to(o._device), torch.as_tensor(mol).to(o._device)
                hist = torch.zeros(3 * N_BINS, dtype=torch.int64, device=o._device)
                runs.append(('torch distances + bincount', lambda: torch_rdf(r, box_t, inv_t, ty_t, mol_t, hist), 20))
            for label, fn, nrep in runs:
                t = timed(fn, nrep)
                extra = ''
                if fn is record:
                    i = rec.info()
                    extra = '   %s form, %d workgroups, %d B of LDS' % (i['form'], i['workgroups'], i['lds_bytes'])
                print('%s %7d atoms %-27s %10.2f us [%.2f, %.2f]%s' % ((prec, n, label) + t + (extra,)), flush=True)
            counts = rec.counts()
            frames = 20 + 5 * reps
            assert rec.frames == frames and (counts % frames == 0).all() and counts.sum() > 0
            if n <= 4096:      # the torch formulation counts the same pairs, up to those its own rounding moves across an edge
                mine, theirs = counts // frames, hist.cpu().numpy().reshape(3, N_BINS) // 120
                print('%s %7d atoms pairs per frame %d (torch formulation %d, %d counts in other bins)'
                      % (prec, n, mine.sum(), theirs.sum(), np.abs(mine.astype(np.int64) - theirs).sum()), flush=True)


if __name__ == '__main__':
    main()
