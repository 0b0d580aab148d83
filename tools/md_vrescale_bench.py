"""The velocity-rescaling thermostat's entry alone (admp_md_vrescale = k_md_vr_sums + k_md_vr_scale) per size and precision, with a
gradient (the closing half kick rides in the sums kernel) and without (the thermostat alone), next to what a thermostatted step
would otherwise launch on the same arrays: admp_md_kick_drift with the kinetic-energy word (dt = 0), and admp_md_scale.  The
library's entries are called directly.  Microseconds per call from device events around back-to-back calls (20 warm-up calls,
median [min, max] of 5 batches).  The half kicks alternate in sign and the scalings alternate mu and 1 / mu, so nothing grows.

    python tools/md_vrescale_bench.py [atoms ...]          (default: 648 98304 1048575)

Bytes moved per call, T the size of a real: kick_drift 3 n (2 T + T) + n T (read v, g; write v; read inv_mass) = 10 n T;
scale 12 n T (it scales positions too); vrescale with a gradient 10 n T + 6 n T (v read and written once more) = 16 n T,
without 3 n T + n T + 6 n T = 10 n T.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admp_amd import _lib, settings                                        # noqa: E402
from admp_amd.md import KB, HarmonicBonded                                 # noqa: E402
from tools.md_mts_bench import system, timed                               # noqa: E402


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [648, 98304, 1048575]
    half, kT_acc, c = 0.25e-4, KB * 300.0 * 1e-4, float(np.exp(-0.5 / 100.0))
    up = float(np.exp(1e-4))
    for prec in ('double', 'single'):
        settings.PRECISION = prec
        o = HarmonicBonded(3, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 2)))
        L, h, P = o._L, o._h, o._ptr
        o._use_current_stream()      # the entries are called directly: the events must sit on the stream the kernels run on
        T = 4 if prec == 'single' else 8
        for n_atoms in sizes:
            r, v, mass, _, _, _ = system(n_atoms)
            n = 3 * (n_atoms // 3)
            rd = torch.as_tensor(r[:n], dtype=o._dtype, device=o._device).contiguous()
            vd = torch.as_tensor(v[:n], dtype=o._dtype, device=o._device).contiguous()
            g = torch.as_tensor(np.random.default_rng(2).normal(size=(n, 3)) * 50.0, dtype=o._dtype, device=o._device).contiguous()
            im = o._real(1.0 / mass[:n])
            ekin = torch.zeros(1, dtype=torch.float64, device=o._device)
            state = torch.zeros((2, 8), dtype=torch.float64, device=o._device)
            state[:, 2] = 1.0
            reps = 400 if n_atoms < 500000 else 100
            k = [0]

            def sign():
                k[0] += 1
                return 1.0 if k[0] & 1 else -1.0

            def kick():
                _lib.check(h, L.admp_md_kick_drift(h, n, None, P(vd), P(g), P(im), sign() * half, 0.0, P(ekin)), 'admp_md_kick_drift')

            def scale():
                _lib.check(h, L.admp_md_scale(h, n, P(rd), P(vd), up if sign() > 0 else 1.0 / up), 'admp_md_scale')

            def vr_kick():
                _lib.check(h, L.admp_md_vrescale(h, n, P(vd), P(g), P(im), sign() * half, 3 * n, kT_acc, c, 1, k[0], k[0], P(state)),
                           'admp_md_vrescale')

            def vr_apply():
                sign()
                _lib.check(h, L.admp_md_vrescale(h, n, P(vd), None, P(im), 0.0, 3 * n, kT_acc, c, 1, k[0], k[0], P(state)),
                           'admp_md_vrescale')
            for label, fn, nbytes in (('kick_drift(ekin)', kick, 10 * n * T), ('scale', scale, 12 * n * T),
                                      ('vrescale kick', vr_kick, 16 * n * T), ('vrescale apply', vr_apply, 10 * n * T)):
                k[0] = 0
                t = timed(fn, reps)
                print('%s n %7d %-16s %8.2f us [%.2f, %.2f]  %6.1f MB  %7.1f GB/s' % ((prec, n_atoms, label) + t + (nbytes / 1e6, nbytes / t[0] / 1e3)),
                      flush=True)
            words = state[(k[0] + 1) & 1].cpu().numpy()      # the slot the last call wrote
            assert torch.isfinite(vd).all() and words[7] == 0.0 and words[4] > 0, words


if __name__ == '__main__':
    main()
