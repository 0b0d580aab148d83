"""The two kernels of the molecular barostat alone (admp_md_mol_sums = k_md_mol_sums, admp_md_mol_scale = k_md_mol_scale) on a box
of waters, one group per molecule, per size, precision and tile capacity, next to the two kernels of the atomic barostat on the
same arrays (admp_md_virial, admp_md_scale).  The library's entries are called directly, without the host read of
`MolecularCRescaleBarostat.sums`.  Microseconds per call from device events around back-to-back calls (20 warm-up calls, median
[min, max] of 5 batches).  The scalings alternate mu and 1 / mu, so the box keeps its size.

    python tools/md_mol_bench.py [atoms ...]          (default: 648 98304 1048575)
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admp_amd import _lib, settings                                        # noqa: E402
from admp_amd.md import HarmonicBonded, MolecularCRescaleBarostat          # noqa: E402
from tools.md_mts_bench import system, timed                               # noqa: E402


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [648, 98304, 1048575]
    up, down = float(np.expm1(1e-4)), float(np.expm1(-1e-4))
    for prec in ('double', 'single'):
        settings.PRECISION = prec
        o = HarmonicBonded(3, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 2)))
        L, h, P = o._L, o._h, o._ptr
        o._use_current_stream()      # the entries are called directly: the events must sit on the stream the kernels run on
        for n_atoms in sizes:
            r, v, mass, _, _, box = system(n_atoms)
            n = 3 * (n_atoms // 3)
            rd = torch.as_tensor(r[:n], dtype=o._dtype, device=o._device).contiguous()
            vd = torch.as_tensor(v[:n], dtype=o._dtype, device=o._device).contiguous()
            g = torch.as_tensor(np.random.default_rng(2).normal(size=(n, 3)) * 50.0, dtype=o._dtype, device=o._device).contiguous()
            out = torch.zeros(21, dtype=torch.float64, device=o._device)
            cell = (ctypes.c_double * 9)(*box.ravel())
            reps = 400 if n_atoms < 500000 else 100
            flip = [0]

            def check(rc, what):
                _lib.check(h, rc, what)
            for cap in (None, 64, 128, 256):
                if cap is None:
                    im = o._real(1.0 / mass[:n])

                    def sums():
                        check(L.admp_md_virial(h, n, P(rd), P(vd), P(g), P(im), 1, 0, P(out)), 'admp_md_virial')

                    def scale():
                        flip[0] ^= 1
                        check(L.admp_md_scale(h, n, P(rd), P(vd), 1.0 + (up if flip[0] else down)), 'admp_md_scale')
                    label = 'atomic (virial, scale)        '
                else:
                    bs = MolecularCRescaleBarostat(o, mass[:n], np.arange(n) // 3, 5.0, 300.0, 1.0, 1000.0, 4.5e-5, 1, tile_atoms=cap)
                    im, info = bs.inv_mass, bs.plan_info()

                    def sums():
                        check(L.admp_md_mol_sums(h, n, P(rd), P(vd), P(g), P(im), cell, 1, 0, P(out)), 'admp_md_mol_sums')

                    def scale():
                        flip[0] ^= 1
                        check(L.admp_md_mol_scale(h, n, P(rd), P(vd), P(im), cell, up if flip[0] else down, down if flip[0] else up),
                              'admp_md_mol_scale')
                    label = 'molecular cap %3d tiles %5d lds %5d B' % (cap, info['tiles'], info['lds_bytes'])
                flip[0] = 0
                t_sums = timed(sums, reps)
                t_scale = timed(scale, reps)
                print('%s n %7d %s: sums %.2f us [%.2f, %.2f]; scale %.2f us [%.2f, %.2f]' % ((prec, n_atoms, label) + t_sums + t_scale),
                      flush=True)
                assert torch.isfinite(rd).all() and torch.isfinite(out).all()


if __name__ == '__main__':
    main()
