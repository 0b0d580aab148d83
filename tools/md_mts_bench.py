"""The fused multiple-time-step kernel alone (admp_amd.md.MTSLangevin.kick_drift = admp_md_mts_step: the slow half kick and four
inner BAOAB steps on the bonded terms of a water box), per size, precision, tile capacity and with / without the thermostat's
noise, next to what ONE 0.5 fs step of the existing chain spends on the same terms (admp_md_bonded + admp_md_langevin +
admp_md_kick_drift).  Two figures per configuration: microseconds per call from device events around back-to-back calls (20
warm-up calls, median [min, max] of 5 batches), and the kernel between the library's own events (profile('md_mts'), 100
launches; the events add about 2 us).

    python tools/md_mts_bench.py [atoms ...]          (default: 648 98304 1048575)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from admp_amd import settings                                        # noqa: E402
from admp_amd.md import HarmonicBonded, Langevin, MTSLangevin        # noqa: E402

K_BOND, R0, K_ANG, TH0 = 3765.6, 0.9572, 460.24, 1.82421813418
MASS = (15.999, 1.008, 1.008)


def system(n_atoms):
    """waters on a cubic grid, bond lengths 2 % off equilibrium, 300 K"""
    n_mol = n_atoms // 3
    g = int(np.ceil(n_mol ** (1 / 3)))
    idx = np.arange(n_mol)
    o = np.stack([idx % g, (idx // g) % g, idx // (g * g)], axis=1) * 3.1 + 1.0
    rng = np.random.default_rng(1)
    local = np.array([[0, 0, 0], [np.sin(TH0 / 2), np.cos(TH0 / 2), 0], [-np.sin(TH0 / 2), np.cos(TH0 / 2), 0]]) * R0
    r = (o[:, None, :] + local[None] * (1 + 0.02 * rng.normal(size=(n_mol, 3, 1)))).reshape(-1, 3)
    mass = np.tile(MASS, n_mol)
    v = rng.normal(size=r.shape) * np.sqrt(1e-4 * 0.0083144626 * 300 / mass)[:, None]
    a = 3 * idx
    bonds = np.stack([np.concatenate([a, a]), np.concatenate([a + 1, a + 2])], axis=1)
    angles = np.stack([a + 1, a, a + 2], axis=1)
    return r, v, mass, bonds, angles, np.eye(3) * 3.1 * g


def timed(fn, reps, batches=5):
    for _ in range(20):
        fn()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return float(np.median(out)), min(out), max(out)


def main():
    sizes = [int(x) for x in sys.argv[1:]] or [648, 98304, 1048575]
    for prec in ('double', 'single'):
        settings.PRECISION = prec
        for n_atoms in sizes:
            r, v, mass, bonds, angles, box = system(n_atoms)
            n_mol = n_atoms // 3
            o = HarmonicBonded(n_atoms, bonds, np.tile([K_BOND, R0], (2 * n_mol, 1)), angles, np.tile([K_ANG, TH0], (n_mol, 1)))
            rd = torch.as_tensor(r, dtype=o._dtype, device=o._device).contiguous()
            vd = torch.as_tensor(v, dtype=o._dtype, device=o._device).contiguous()
            gs, g = torch.zeros_like(rd), torch.zeros_like(rd)
            reps = 400 if n_atoms < 500000 else 100
            lv = Langevin(o, mass, 0.5, 300.0, 0.05, 1)

            def chain():
                o.add_forces(rd, box, g)
                lv.kick_drift(rd, vd, g)
                lv.kick(rd, vd, g)
            print('%s n %7d existing chain (bonded + langevin + kick, one 0.5 fs step): %.2f us [%.2f, %.2f]'
                  % ((prec, n_atoms) + timed(chain, reps)), flush=True)
            for cap in (32, 64, 128, 256):
                for gamma in (0.0, 0.05):
                    mts = MTSLangevin(o, mass, 2.0, 4, 300.0, gamma, 1, tile_atoms=cap)
                    rd.copy_(torch.as_tensor(r))
                    vd.copy_(torch.as_tensor(v))
                    fn = lambda: mts.kick_drift(rd, vd, gs, box)      # noqa: E731
                    info = mts.plan_info()
                    t = timed(fn, reps)
                    o.profile(True, only='md_mts')
                    o.profile_reset()
                    for _ in range(100):
                        fn()
                    torch.cuda.synchronize()
                    ms, cnt = o.profile_report()['md_mts']
                    o.profile(False)
                    print('%s n %7d cap %3d gamma %.2f tiles %6d lds %5d B: per call %.2f us [%.2f, %.2f]; kernel between events %.2f us'
                          % ((prec, n_atoms, cap, gamma, info['tiles'], info['lds_bytes']) + t + (ms / cnt * 1e3,)), flush=True)
                    assert torch.isfinite(rd).all()


if __name__ == '__main__':
    main()
