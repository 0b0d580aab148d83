#!/usr/bin/env python3
"""The two first-half kernels of the MD integrators on the same arrays, for a kernel trace (k_md_langevin against
k_md_kick_drift; both precisions, three sizes):
    rocprofv3 --kernel-trace --stats --output-format csv -d profile_out/md_trace -- python3 tools/md_kernels_trace.py [launches]
    python3 tools/md_kernels_trace.py --summary profile_out/md_trace        # average us per kernel, precision and size
Sizes are told apart in the trace by their grids (3072, 98304 and 262144 lanes)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (3072, 98304, 1048575)


def run(launches):
    import numpy as np
    import torch
    from admp_amd import settings
    from admp_amd.md import HarmonicBonded, Langevin, VelocityVerlet
    for prec in ('single', 'double'):
        settings.PRECISION = prec
        o = HarmonicBonded(3, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 2)))
        for n in SIZES:
            mass = np.tile((15.999, 1.008, 1.008), n // 3 + 1)[:n]
            g = torch.Generator(device='cuda').manual_seed(1)
            r = torch.rand((n, 3), generator=g, device='cuda', dtype=o._dtype) * 100.0
            v = torch.randn((n, 3), generator=g, device='cuda', dtype=o._dtype) * 1e-2
            f = torch.randn((n, 3), generator=g, device='cuda', dtype=o._dtype) * 50.0
            lv, vv = Langevin(o, mass, 0.5, 300.0, 0.05, 1), VelocityVerlet(o, mass, 0.5)
            for _ in range(launches):          # alternating, so both see the same caches and clocks
                lv.kick_drift(r, v, f)
                vv.kick_drift(r, v, f)
            torch.cuda.synchronize()
            print('%s %d atoms: %d launches of each' % (prec, n, launches))


def summary(folder):
    rows = {}
    for path in glob.glob(os.path.join(folder, '**', '*kernel_trace.csv'), recursive=True):
        for rec in csv.DictReader(open(path)):
            name = rec['Kernel_Name']
            if 'k_md_langevin' not in name and 'k_md_kick_drift' not in name:
                continue
            key = (name.split('(')[0].split(' ')[-1], int(rec['Grid_Size_X']))
            rows.setdefault(key, []).append((int(rec['End_Timestamp']) - int(rec['Start_Timestamp'])) * 1e-3)
    for key in sorted(rows):
        t = sorted(rows[key])
        print('%-40s grid %7d: median %8.2f us, mean %8.2f us (%d launches)' % (key[0], key[1], t[len(t) // 2],
                                                                                    sum(t) / len(t), len(t)))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--summary':
        summary(sys.argv[2])
    else:
        run(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
