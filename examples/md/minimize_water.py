#!/usr/bin/env python
"""The two minimisers of the MD drivers side by side on the synthetic water box, from the same start and for the same number of
force evaluations: the capped steepest descent of water_md.minimize (no atom moves more than 0.02 A per evaluation; one host
read and half a dozen torch launches per iteration) and FIRE (admp_amd.md.FireMinimizer: one C call per iteration,
admp_md_fire_step, its control loop on the device).  Every 10 evaluations the potential energy and the largest |g_i| of each
are printed (two host reads, made for this table only), and one final line holds both pairs at the end.

    python examples/md/minimize_water.py [--waters 1024] [--minimize 200] [--pol] [--single] [--mesh K] [--rebuild 10]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from water_md import add_arguments, setup, minimize      # noqa: E402
from admp_amd import settings                            # noqa: E402

EVERY = 10


def gmax(grad):
    return float(grad.double().norm(dim=1).max())


def run(w, opt, which):
    """water_md.minimize with --minimizer `which` from w.pos; returns ({evaluation: (Epot, gmax)}, (Epot, gmax) at the end)"""
    inner, table, count = w.forces, {}, [0]

    def forces(p, pairs, bonded=True):
        e, g = inner(p, pairs, bonded)
        if count[0] % EVERY == 0 and count[0] <= opt.minimize:      # (the k-th evaluation sees the positions after k moves)
            table[count[0]] = (w.epot_now(e), gmax(g))
        count[0] += 1
        return e, g
    w.forces, opt.minimizer = forces, which
    try:
        _, _, e, grad = minimize(w, opt, w.pos)
    finally:
        w.forces = inner
    return table, (w.epot_now(e), gmax(grad))


def main():
    ap = argparse.ArgumentParser()
    add_arguments(ap)
    opt = ap.parse_args()
    w = setup(opt)
    start = w.pos.clone()
    sd, sd_end = run(w, opt, 'sd')
    assert bool((w.pos == start).all())                     # both start from the same positions
    fire, fire_end = run(w, opt, 'fire')
    print('%11s  %14s %12s  %14s %12s' % ('evaluations', 'sd: Epot', 'max |g_i|', 'fire: Epot', 'max |g_i|'))
    for k in sorted(set(sd) & set(fire)):
        print('%11d  %14.4f %12.4f  %14.4f %12.4f' % ((k,) + sd[k] + fire[k]))
    print('# %d waters, %s, %s, after %d evaluations: sd Epot %.6f gmax %.6f; fire Epot %.6f gmax %.6f (kJ/mol, kJ/mol/A)'
          % (w.n_mol, 'polarizable' if opt.pol else 'fixed multipoles', settings.PRECISION, opt.minimize, sd_end[0], sd_end[1],
             fire_end[0], fire_end[1]))


if __name__ == '__main__':
    main()
