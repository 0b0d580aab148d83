"""The closing pair kernel riding in the x pass of the mesh convolution (k_xconv_pair_full, ADMP_PAIR_RIDER) against the
launch of its own (ADMP_PAIR_RIDER=0): one build, one process, two handles that see the same inputs call by call -- the
switch is read per call, so the process sets it before every evaluation.

Cases: the headline system of bench.py (3072 atoms, double precision, 97^3 mesh) over a moving sequence with
get_forces_and_dQ (dE/dQ_local requested: the general pair forms) and with get_forces (charge-only forms), at the default
SCF threshold and at a tight one (chains of two and more Jacobi steps); 216 waters on a Verlet list with a skin and
set_cutoff (the kernels walk the inner table); a triclinic cell (the x pass runs the two transforms, not the circulant
product); one single-precision handle, which keeps the launch of its own (asserted) and must be left as it was.

Compared per call: the four energy parts, gradient, dipoles, dE/dQ_local, cycle count and convergence flag.  Counts and
flags are equal.  The rows the pair kernel writes (gradient, potential, field) are summed without atomics and the rider
walks each row in the same order with the same arithmetic, so they are expected bit-equal; the calculator hands out only
sums of them with the mesh part, whose spread and energy words are accumulated with floating-point atomics in an order that
changes from launch to launch, so two runs of ONE form already differ in the last bits and the rows cannot be isolated
here.  The bound is therefore the one tests/test_gpu_dft_circulant.py uses for run-to-run differences of the same kernels:
a reordered sum of n <= 1e3 partial sums per word, 1e3 * 2^-53 = 1.1e-13 of the largest word of the array (single
precision: 1e3 * 2^-24)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = """
import os, sys, numpy as np
sys.path.insert(0, %r)
import torch
from tests.test_gpu_parity import water_system
from admp_amd import settings
from admp_amd import systems as S
from admp_amd.pme import ADMPPmeForce
from admp_amd.neighbor import NeighborList
out = {}

def host(x):
    return np.asarray(torch.as_tensor(x).cpu(), dtype=np.float64)

def call(f, mode, dq, pos, box, pairs, par, U):
    os.environ['ADMP_PAIR_RIDER'] = mode
    rest = (par['Q_local'], par['pol'], par['tholes'], par['mScales'], par['pScales'], par['dScales'])
    if dq:
        E, G, dQ = f.get_forces_and_dQ(pos, box, pairs, *rest, U_init=U)
    else:
        (E, G), dQ = f.get_forces(pos, box, pairs, *rest, U_init=U), None
    r = dict(parts=np.asarray(f.energy_parts, dtype=np.float64), G=host(G), U=host(f.U_ind),
             n=np.asarray([int(f.n_cycle), int(bool(f.lconverg))]))
    if dq:
        r['dQ'] = host(dQ)
    return r

def sequence(key, make, frames, dq, box, pairs, par):
    # handle A rides, handle B launches the kernel on its own; both start every call from A's dipoles
    fA, fB = make(), make()
    U = None
    forms = []
    for k, pos in enumerate(frames):
        before = fA.scf_stats()
        a = call(fA, '1', dq, pos, box, pairs, par, U)
        b = call(fB, '0', dq, pos, box, pairs, par, U)
        after = fA.scf_stats()
        forms.append([after[q] - before[q] for q in ('plain', 'speculative', 'chained')] + [int(a['n'][0])])
        U = fA.U_ind
        U = U.clone() if hasattr(U, 'clone') else np.array(U)
        for name in a:
            out['%%s|%%d|%%s|A' %% (key, k, name)] = a[name]
            out['%%s|%%d|%%s|B' %% (key, k, name)] = b[name]
    sA, sB = fA.scf_stats(), fB.scf_stats()
    keys = ('plain', 'speculative', 'speculative_failed', 'chained', 'chained_too_short')
    out[key + '|scf|A'] = np.asarray([sA[q] for q in keys])
    out[key + '|scf|B'] = np.asarray([sB[q] for q in keys])
    rA, rB = fA.pair_rider_stats(), fB.pair_rider_stats()
    out[key + '|ride|A'] = np.asarray([rA['rode'], rA['own_launch']])
    out[key + '|ride|B'] = np.asarray([rB['rode'], rB['own_launch']])
    out[key + '|forms'] = np.asarray(forms)
    x = fA.xpass_stats()
    out[key + '|xpass'] = np.asarray([x['circulant'], x['transforms']])

# ---- the headline system: 3072 atoms, double precision, 97^3 mesh, thermal motion
import bench
w = bench.make_workload('S1')
_, a = bench.make_force(w)
frames = bench.ThermalFrames(w, torch.device('cuda'))
par = dict(Q_local=a['Q_local'], pol=a['pol'], tholes=a['tholes'], mScales=a['mScales'], pScales=a['pScales'],
           dScales=a['dScales'])

def s1():
    f = bench.make_force(w)[0]
    return f
for key, dq, thresh, n in (('S1dq', True, None, 10), ('S1', False, None, 10), ('S1tight', False, 1e-2, 12)):
    old = settings.POL_CONV
    if thresh is not None:
        settings.POL_CONV = thresh
    try:
        sequence(key, s1, [frames.step_frame(k) for k in range(n)], dq, a['box'], a['pairs'], par)
    finally:
        settings.POL_CONV = old
f = s1()
assert (f.K1, f.K2, f.K3) == (97, 97, 97), (f.K1, f.K2, f.K3)
del f

# ---- 216 waters: skin list with a cutoff, triclinic cell, single precision
pos, box, at, ai, cov, par2, pairs = water_system(216, 5, True)
box = np.asarray(box, dtype=np.float64)
rng = np.random.default_rng(5)
kick = rng.standard_normal(pos.shape)

def moved(p, n):
    # every geometry three times in a row: a call that starts from the converged dipoles of its own geometry passes its
    # first check, and the one after it is enqueued in the speculative form
    return [p + 0.001 * (k // 3) * kick for k in range(n)]

def small(prec, bx, K, cutoff=0.0):
    def make():
        settings.PRECISION = prec
        settings.REFERENCE_KPOINT_ORDER = False      # (the literal order is no Ewald sum on unequal meshes: the SCF diverges)
        f = ADMPPmeForce(bx, at, ai, cov, 4.0, 1e-4, 2, lpol=True)
        f.K1, f.K2, f.K3 = K
        f.refresh_calculators()
        if cutoff:
            f.set_cutoff(cutoff)
        return f
    return make

skin = S.build_pairs(pos, box, 5.0)
sequence('cut', small('double', box, (31, 34, 38), 4.0), moved(pos, 6), False, box, skin, par2)
sequence('cutdq', small('double', box, (31, 34, 38), 4.0), moved(pos, 6), True, box, skin, par2)
tric = box.copy()
tric[1, 0] = 0.9
tric[2, 0] = -0.6
tric[2, 1] = 0.7
ptric = (pos @ np.linalg.inv(box)) @ tric
sequence('tric', small('double', tric, (31, 34, 38)), moved(ptric, 6), False, tric, NeighborList(tric, 4.0).allocate(ptric).cpu().numpy(),
         par2)
sequence('f32', small('single', box, (31, 34, 38)), moved(pos, 6), False, box, pairs, par2)
np.savez(sys.argv[1], **out)
print('PAIR-RIDER-RUN-OK')
""" % ROOT

TOL64 = 1e3 * 2.0 ** -53
TOL32 = 1e3 * 2.0 ** -24


@pytest.mark.gpu
def test_pair_rider_vs_own_launch(tmp_path):
    path = str(tmp_path / 'rider.npz')
    env = dict(os.environ, ADMP_DFT='1')
    env.pop('ADMP_PAIR_RIDER', None)
    r = subprocess.run([sys.executable, '-c', CODE, path], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and 'PAIR-RIDER-RUN-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    res = dict(np.load(path))
    cases = ('S1dq', 'S1', 'S1tight', 'cut', 'cutdq', 'tric', 'f32')
    for key in cases:
        scfA, scfB = res[key + '|scf|A'], res[key + '|scf|B']
        rideA, rideB = res[key + '|ride|A'], res[key + '|ride|B']
        print(key, 'forms (plain, speculative, failed, chained, too short):', scfA, 'rode / own launch:', rideA, rideB,
              'x passes (circulant, transforms):', res[key + '|xpass'])
        assert np.array_equal(scfA, scfB), (key, scfA, scfB)            # the same decisions
        assert rideB[0] == 0 and rideB[1] > 0, (key, rideB)            # switched off: never rides
        if key == 'f32':
            assert rideA[0] == 0 and rideA[1] > 0, (key, rideA)        # single precision keeps its own launch
        else:
            # every speculative and every chained call carries its closing pair kernel in an x pass
            assert rideA[0] >= scfA[1] + scfA[3] and rideA[0] > 0, (key, rideA, scfA)
            assert rideA[0] + rideA[1] == rideB[1], (key, rideA, rideB)
    # the headline sequences went through every form of the SCF driver, the tight one through chains of >= 2 steps
    for key in ('S1dq', 'S1', 'S1tight'):
        scf = res[key + '|scf|A']
        assert scf[0] > 0 and scf[1] + scf[3] > 0, (key, scf)
        assert res[key + '|xpass'][0] > 0 and res[key + '|xpass'][1] == 0, (key, res[key + '|xpass'])
    for key in ('S1dq', 'S1'):
        scf = res[key + '|scf|A']
        assert scf[0] > 0 and scf[1] > 0 and scf[3] > 0, (key, scf)
    forms = res['S1tight|forms']
    assert ((forms[:, 2] > 0) & (forms[:, 3] >= 2)).any(), forms
    assert res['tric|xpass'][0] == 0 and res['tric|xpass'][1] > 0, res['tric|xpass']

    worst = {}
    for name, b in res.items():
        if not name.endswith('|B') or name.count('|') != 3:
            continue
        key, k, what, _ = name.split('|')
        a = res[name[:-1] + 'A']
        if what == 'n':
            assert np.array_equal(a, b), (name, a, b)                   # cycle count and convergence flag
            continue
        assert np.isfinite(a).all() and np.isfinite(b).all(), name
        scale = np.abs(b).max()
        err = np.abs(a - b).max()
        kind = ('f32 ' if key == 'f32' else 'f64 ') + what
        worst[kind] = max(worst.get(kind, 0.0), err / scale)
        print('%-8s call %2s %-5s max|on - off| / max|off| = %.2e' % (key, k, what, err / scale))
        assert err <= (TOL32 if key == 'f32' else TOL64) * scale, (name, err, scale)
    print('largest |rider on - rider off| / max|off|:', {k: '%.2e' % v for k, v in sorted(worst.items())})
