"""What the predictor-corrector dipoles (ADMPPmeForce.set_aspc) cost and save per MD step, next to the existing starts of the SCF, on
the moving frames of bench.py: S1 (water_pol_1024, double) and S2 (the 98 304-atom box, single).  Per workload and start:

    previous       U_init = U(n-1), SCF to the threshold (10 and 1e-2)
    predict 1      U_init = 2 U(n-1) - U(n-2) formed with torch operations on the host side (water_md.py --predict 1), 1e-2
    aspc 2         set_aspc(2): predictor kernel, one damped Jacobi step, no residual read

ms per step is wall time over a batch of back-to-back get_forces calls (each returns after its own host read of the energies), the
device synchronised before and after; 20 warm-up steps, then the median [min, max] of 5 batches of `steps` steps.  Field
evaluations per step = n_cycle + 1 as the library reports it.  The frames are the same for every start.  The last column is
how far the dipoles of the last step are from converged ones (a second handle, threshold 1e-6 in double / 1e-3 in single):
max|U - U_conv| / max|U_conv|.

With --drift the NVE driver is run for 200 steps per start (examples/md/nve_water.py --pol, fresh processes) and its relative
energy drift and ms per step are printed.

    python tools/scf_aspc_bench.py [--steps 100] [--workloads S1 S2] [--drift]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B                                                          # noqa: E402
from admp_amd import settings                                              # noqa: E402

STARTS = (('previous', 10.0), ('previous', 1e-2), ('predict 1', 1e-2), ('aspc 2', None))


def run(w, frames, start, thresh, steps, warmup=20, batches=5):
    f, a = B.make_force(w)
    old = settings.POL_CONV
    settings.POL_CONV = 10.0 if thresh is None else thresh
    try:
        seq = [frames.step_frame(k) for k in range(warmup + batches * steps)]
        if start.startswith('aspc'):
            f.set_aspc(int(start.split()[1]))
        U = U0 = U1 = None
        evals, times, k = 0, [], 0
        for batch in range(batches + 1):
            n = warmup if batch == 0 else steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                U_init = (2.0 * U1 - U0) if (start.startswith('predict') and U0 is not None) else U
                B.step(f, a, U_init, seq[k])
                U = f.U_ind
                if start.startswith('predict'):
                    U0, U1 = U1, U
                if batch:
                    evals += f.n_cycle + 1
                k += 1
            torch.cuda.synchronize()
            if batch:
                times.append((time.perf_counter() - t0) / n * 1e3)
        g, _ = B.make_force(w)
        settings.POL_CONV = 1e-6 if w['prec'] == 'double' else 1e-3
        old_max, settings.MAX_N_POL = settings.MAX_N_POL, 200
        try:
            B.step(g, a, U, seq[k - 1])
        finally:
            settings.MAX_N_POL = old_max
        dev = float((U.double() - g.U_ind.double()).abs().max() / g.U_ind.double().abs().max())
        info = f.aspc_info()
    finally:
        settings.POL_CONV = old
    return float(np.median(times)), min(times), max(times), evals / float(batches * steps), dev, info


def drift(w_name):
    size = {'S1': ['--waters', '1024'], 'S2': ['--waters', '32768', '--single', '--mesh', '128']}[w_name]
    for label, extra in (('previous, 10', ['--thresh', '10']), ('previous, 1e-2', ['--thresh', '1e-2']),
                         ('predict 1, 1e-2', ['--thresh', '1e-2', '--predict', '1']), ('aspc 2', ['--aspc', '2'])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'md', 'nve_water.py'), '--pol', '--steps', '200'] + size + extra,
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        if r.returncode != 0:
            print('%s NVE %-16s failed: %s' % (w_name, label, r.stderr[-500:]), flush=True)
            continue
        tail = [x for x in r.stdout.splitlines() if x.startswith('#')]
        print('%s NVE 200 steps %-16s %s' % (w_name, label, ' | '.join(x[2:] for x in tail if 'ms/step' in x or 'field evaluations' in x
                                                                      or 'mean SCF' in x)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--workloads', nargs='+', default=['S1', 'S2'], choices=sorted(B.WORKLOADS))
    ap.add_argument('--drift', action='store_true')
    opt = ap.parse_args()
    for name in opt.workloads:
        w = B.make_workload(name)
        frames = B.ThermalFrames(w, torch.device('cuda', 0))
        print('# %s: %s; %s' % (name, w['desc'], frames.describe()), flush=True)
        for start, thresh in STARTS:
            med, lo, hi, ev, dev, info = run(w, frames, start, thresh, opt.steps)
            print('%s %-10s thresh %-5s %8.4f ms/step [%.4f, %.4f]  %5.2f field evaluations/step  |U - U_conv| %.2e%s'
                  % (name, start, '-' if thresh is None else '%g' % thresh, med, lo, hi, ev, dev,
                     '  (fixed %d, warm-up %d, fallback %d)' % (info['fixed'], info['warmup'], info['fallback']) if thresh is None else ''),
                  flush=True)
        if opt.drift:
            drift(name)


if __name__ == '__main__':
    main()
