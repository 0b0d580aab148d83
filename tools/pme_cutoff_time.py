#!/usr/bin/env python3
"""The polarizable PME call on a Verlet list with a skin, with and without admp_set_cutoff (the multipolar kernels walk the
inner table of the call), against the exact-rc list and the pruned inner list; then bench.md_all_terms with the cutoff set.
    python tools/pme_cutoff_time.py [S2|S3] [reps=5] [steps=10]
One process, the four variants alternated rep by rep; warm-started SCF at a fixed geometry, device-synchronised wall time
per call (median over reps of the mean over steps).
  (a) exact: list searched at rc            (b) skin: list at rc + 1 A, no cutoff
  (c) skin + cutoff rc                      (d) pruned: the skin table pruned to rc (admp_prune_pairs)
The cutoff recovers (b - c) / (b - a) of the skin's cost."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench

name = sys.argv[1] if len(sys.argv) > 1 else 'S2'
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
w = bench.make_workload(name)
pos, box = w['pos'], w['box']
forces = {}
for v in ('exact', 'skin', 'skin_cut', 'pruned'):
    f, a = bench.make_force(w)
    p = a['positions']
    if v == 'exact':
        f.set_pairs(a['pairs'])
    else:
        f.update_neighbors(p, box, rc=bench.RC + bench.SKIN)
    a = dict(a, pairs=None)
    U = None
    for _ in range(3):                   # (the first evaluation compiles the site classes into the table as built)
        bench.step(f, a, U)
        U = f.U_ind
    if v == 'skin_cut':
        f.set_cutoff(bench.RC)
    elif v == 'pruned':
        f.prune_neighbors(p, box, bench.RC)
    forces[v] = (f, a, [U])
    if v == 'skin':
        n_skin = f.n_pairs
    elif v == 'exact':
        n_exact = f.n_pairs

res = {v: [] for v in forces}
for r in range(reps):
    order = list(forces) if r % 2 == 0 else list(reversed(list(forces)))
    for v in order:
        f, a, Ubox = forces[v]
        for _ in range(2):
            bench.step(f, a, Ubox[0]); Ubox[0] = f.U_ind
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            bench.step(f, a, Ubox[0]); Ubox[0] = f.U_ind
        torch.cuda.synchronize()
        res[v].append((time.perf_counter() - t0) / steps * 1e3)

E = {}
for v, (f, a, Ubox) in forces.items():
    E[v] = float(bench.step(f, a, Ubox[0])[0])
med = {v: statistics.median(x) for v, x in res.items()}
a_, b_, c_ = med['exact'], med['skin'], med['skin_cut']
out = {'workload': name, 'n_pairs_exact': n_exact, 'n_pairs_skin': n_skin, 'reps': reps, 'steps': steps,
       'ms_per_call_median': {v: round(x, 4) for v, x in med.items()},
       'ms_per_call_all': {v: [round(t, 4) for t in x] for v, x in res.items()},
       'recovered_fraction': round((b_ - c_) / (b_ - a_), 3) if b_ > a_ else None,
       'energy': E, 'energy_cut_minus_exact': E['skin_cut'] - E['exact']}
print(json.dumps(out))

f, a, _ = forces['skin_cut']
fr = bench.ThermalFrames(w, torch.device('cuda', 0))
md = bench.md_all_terms(w, f, a, fr, 10, 2)
print(json.dumps({'workload': name, 'md_all_terms_with_cutoff': {k: md[k] for k in ('ms_per_step', 'step_ms_min_median_max')
                                                                  if k in md}}))
