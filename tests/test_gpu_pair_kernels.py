"""The real-space pair kernels (admp_amd/csrc/pair_kernels.hip) row by row against the float64 oracle, at every lane count
they are compiled for.  k_pair_full and k_pair_field run alone through the C entry admp_pair_real (what an evaluation does
up to that kernel, then its raw rows: energy, dE/dr, dE/dQ_global, dE/dU); inputs, reference, single-precision floors and
bars come from tests/pair_ref.py and are proved sound without a GPU in tests/test_pair_ref_cpu.py.

The lane switches (ADMP_PAIR_LPR, ADMP_FIELD_LPR, ADMP_SCALAR_LPR, ADMP_TT_LPR, ADMP_PAIR_MINW) are read once per process,
so every setting gets a child process: 1, 2, 4, 8, 16 and 32 lanes per row, nothing forced (the rule's own choice), and the
other minimum-waves instance at 16 lanes (one child per precision: the default differs).  A child runs every case in both
precisions through one call sequence per handle --

    1  first call on a fresh handle            5  the charge-only sites were given moments: the table's classes are stale
    2  second call (same table: bitwise equal)  6  the call after that (classes recompiled)
    3  the field kernel on that table           7, 8  the field kernel and its increment again
    4  its increment (k_pair_field_ind after    9, 10  charge-only forms not allowed (bitwise equal)
       the SCF's Jacobi step on a field given)

-- and every call is compared with the reference: double precision at the bars of the host test of the same functions,
single precision at FLOOR_FACTOR times the host-f32 floor of the same case and output.  The children also run the scalar
pair kernel (k_pair_scalar: Tang-Toennies and dispersion, same lane counts, same two-ahead prefetch) on two systems of
tests/neighbour_ref.py with that file's rules, and the refusals of the entry.  The references are computed once in the
parent and handed over in a file.  A child that faults, aborts or runs into its time limit ends the module: no further
child is started."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import neighbour_ref as NR
from tests import pair_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR_SYSTEMS = ('gas4097', 'gas15')      # the cell path and the brute path of the table builder
DISP_PMAX = 6

# (id, environment, lanes per row expected, precisions, run the refusals)
LANE_ENV = ('ADMP_PAIR_LPR', 'ADMP_FIELD_LPR', 'ADMP_SCALAR_LPR', 'ADMP_TT_LPR')
SETTINGS = [('lpr%d' % L, {k: str(L) for k in LANE_ENV}, L, ('double', 'single'), False) for L in (1, 2, 4, 8, 16, 32)]
SETTINGS.append(('rule', {}, 16, ('double', 'single'), True))     # every case has fewer than 8192 rows: the rule says 16
SETTINGS.append(('minw2_double', dict({k: '16' for k in LANE_ENV}, ADMP_PAIR_MINW='2'), 16, ('double',), False))
SETTINGS.append(('minw1_single', dict({k: '16' for k in LANE_ENV}, ADMP_PAIR_MINW='1'), 16, ('single',), False))

CHILD = r'''
import ctypes, json, pickle, sys, time
t_start = time.time()
sys.path.insert(0, %r)
import numpy as np
import torch
from admp_amd import settings, _lib
from admp_amd.pme import ADMPPmeForce
from tests import pair_ref as R
from tests import neighbour_ref as NR

data = pickle.load(open(sys.argv[1], 'rb'))
precs = sys.argv[3].split(',')
out = {'calls': [], 'scalar': 0, 'refusals': 0, 'secs': [time.time() - t_start]}


def force(c):
    f = ADMPPmeForce(c['box'], c['axis_type'], c['axis_indices'], c['cov'], R.RC_LIST, 1e-4, 2, lpol=c['lpol'])
    f.kappa, f.K1, f.K2, f.K3 = c['kappa'], 16, 16, 16       # (the mesh is allocated, never used: no mesh kernel runs)
    f.refresh_calculators()
    if c['cutoff']:
        f.set_cutoff(c['cutoff'])
    return f


def call(f, c, variant, which, flags, field):
    Ql = c['Q_local_B'] if variant == 'B' else c['Q_local']
    r = f.pair_real(c['pos'], c['box'], c['pairs'], Ql, R.MSCALES, c['pol'], c['thole'], R.PSCALES, c['U'], which=which, flags=flags,
                    field=field if which == 2 else None)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


SEQ = [('A', 0, 1), ('A', 0, 1), ('A', 1, 1), ('A', 2, 1), ('B', 0, 1), ('B', 0, 1), ('B', 1, 1), ('B', 2, 1), ('B', 0, 0), ('B', 0, 0)]
for prec in precs:
    settings.PRECISION = prec
    for name in data['names']:
        c = data['cases'][name]
        f = force(c)
        n = c['n']
        raw = []
        for step, (variant, which, flags) in enumerate(SEQ):
            if which >= 1 and not c['lpol']:
                raw.append(None)
                continue
            got = call(f, c, variant, which, flags, data['fields'].get(name))
            raw.append(got)
            ref = data['refs'][name][variant] if which < 2 else data['refs_ind'][name][prec]
            mono = c['mono'] if variant == 'A' else np.zeros(n, dtype=bool)
            cmp, zeros_ok = dict(got), True
            if not c['lpol']:
                cmp['fld'] = None
            if which == 0:
                reduced = mono if flags & 1 else np.zeros(n, dtype=bool)       # rows walked in the charge-only forms:
                zeros_ok = not got['pot'][reduced, 1:].any()                  # only slot 0 of pot is formed, no field
                cmp['pot'] = np.where(reduced[:, None] & (np.arange(9) > 0)[None, :], ref['pot'], got['pot'])
                if c['lpol']:
                    zeros_ok = zeros_ok and not got['fld'][reduced].any()
                    cmp['fld'] = np.where(reduced[:, None], ref['fld'], got['fld'])
            else:
                act = c['pol'] > 0                                           # the field kernel's rows; the others stay zero
                zeros_ok = not got['fld'][~act].any()
                cmp = {'fld': np.where(act[:, None], got['fld'], ref['fld'])}
            iso = c['isolated']
            iso_ok = all(not got[k][iso].any() for k in ('grad', 'pot', 'fld') if got.get(k) is not None)
            same = None
            if step in (1, 9):
                same = all(np.array_equal(got[k], raw[step - 1][k]) for k in ('grad', 'pot', 'fld') if got.get(k) is not None)
            out['calls'].append(dict(name=name, prec=prec, step=step, variant=variant, which=which, flags=flags,
                                     info=list(got['info']), err=R.errors(cmp, ref), excess=R.double_excess(cmp, ref),
                                     zeros_ok=bool(zeros_ok), iso_ok=bool(iso_ok), same=same))
        del f

out['secs'].append(time.time() - t_start)
# ---- the scalar pair kernel: Tang-Toennies and dispersion on an explicit list (nothing is classified by distance)
from admp_amd.pairwise import generate_pairwise_interaction, TT_damping_qq_c6_kernel
from admp_amd.disp_pme import ADMPDispPmeForce
for prec in precs:
    settings.PRECISION = prec
    tolE, tolG = (1e-11, 1e-11) if prec == 'double' else (2e-5, 2e-4)      # the rules of tests/neighbour_ref.py (check_tt)
    for name in data['scalar_names']:
        s = data['scalar'][name]
        pos, box, pairs = np.array(s['pos']), np.array(s['box']), s['pairs']
        pot = generate_pairwise_interaction(TT_damping_qq_c6_kernel, s['cov'], static_args={})
        E, G = pot.value_and_grad(pos, box, pairs, NR.MSCALES, *s['params'])
        dm = pot.get_mscale_gradient(pos, box, None, NR.MSCALES, *s['params'])
        NR.check_tt(dict(E=float(E), grad=np.asarray(G, dtype=np.float64), dm=dm, n_pairs=pot.n_pairs), s['tt'], prec,
                    (0, 0, 0), n_pairs_ref=len(pairs))
        d = ADMPDispPmeForce(box, s['cov'], s['rc'], 1e-4, s['pmax'])
        assert (d.kappa, d.K1, d.K2, d.K3) == tuple(s['ewald']), ((d.kappa, d.K1, d.K2, d.K3), s['ewald'])
        c6 = s['params'][3][:, None]
        E, G = d.get_forces(pos, box, pairs, c6, NR.MSCALES)
        ref = s['disp']
        assert abs(d.energy_parts[0] - ref['parts'][0]) <= tolE * abs(ref['parts'][0]), (d.energy_parts, ref['parts'])
        # (the gradient holds the mesh part as well: double precision at the bar of the whole-evaluation tests, 1e-8)
        dg = np.linalg.norm(np.asarray(G, dtype=np.float64) - ref['grad'])
        assert dg <= max(tolG, 1e-8) * np.linalg.norm(ref['grad']), (dg, np.linalg.norm(ref['grad']))
        dmd = d.get_mscale_gradient(pos, box, None, c6, NR.MSCALES)
        assert np.abs(dmd - ref['dm']).max() <= tolG * np.abs(ref['dm']).max(), (dmd, ref['dm'])
        out['scalar'] += 1

out['secs'].append(time.time() - t_start)
# ---- refusals of admp_pair_real: each before anything is launched, and the handle serves a valid call afterwards
if sys.argv[4] == '1':
    settings.PRECISION = 'double'
    c = data['cases']['na3']
    L = _lib.load()
    f, g = force(c), force(dict(c, lpol=False))
    P = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()      # noqa: E731
    pos, Q, pol, th, U = P(c['pos']), P(c['Q_local']), P(c['pol']), P(c['thole']), P(c['U'])
    grad, pot, fld = P(np.zeros((3, 3))), P(np.zeros((3, 9))), P(np.zeros((3, 3)))
    E, info = ctypes.c_double(0.0), (ctypes.c_int * 4)()
    box, mS, pS = _lib.darr(c['box']), _lib.darr(R.MSCALES), _lib.darr(R.PSCALES)

    def raw(h, which, grad=grad, pot=pot, fld=fld, pol=pol, info=info, F=None):
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        return L.admp_pair_real(h._h, p(pos), box, p(Q), p(pol), p(th), 5, mS, pS, p(U), p(F), which, 1, 1, ctypes.byref(E),
                                p(grad), p(pot), p(fld), info)
    assert raw(f, 0) != 0 and b'pairs must be set' in L.admp_last_error(f._h)            # no pairs set
    f.set_pairs(c['pairs'])
    g.set_pairs(c['pairs'])
    assert raw(f, 0) == 0
    for kw in (dict(grad=None), dict(pot=None), dict(fld=None), dict(info=None), dict(pol=None)):     # null outputs / inputs
        assert raw(f, 0, **kw) != 0, kw
    assert raw(f, 1, fld=None) != 0
    assert raw(f, 3) != 0 and raw(f, -1) != 0 and b'which' in L.admp_last_error(f._h)    # unknown which
    assert raw(f, 2) != 0 and b'Jacobi' in L.admp_last_error(f._h)                       # the increment without its field
    assert raw(f, 2, F=grad) == 0
    assert raw(g, 1) != 0 and b'polarizable' in L.admp_last_error(g._h)                  # field kernels, non-polarizable handle
    assert raw(g, 2, F=grad) != 0
    assert raw(g, 0, fld=None) == 0                                                       # (which has no field to return)
    assert raw(f, 0) == 0 and raw(f, 1) == 0                                              # still serving
    _lib.check(f._h, L.admp_slab_configure(f._h, 0, 2), 'admp_slab_configure')
    assert raw(f, 0) != 0 and b'single rank' in L.admp_last_error(f._h)                  # slab handle
    out['refusals'] = 1

json.dump(out, open(sys.argv[2], 'w'))
print('child ok')
''' % ROOT


@pytest.fixture(scope='module')
def shared(tmp_path_factory):
    """cases, references and floors of tests/pair_ref.py and the scalar references, computed once and written to one file"""
    import torch
    from admp_amd.pme import setup_ewald_parameters
    from oracle import admp_oracle as O
    d = tmp_path_factory.mktemp('pair_kernels')
    data = dict(names=R.CASES, cases={n: R.case(n) for n in R.CASES},
                refs={n: {v: R.reference(n, v) for v in 'AB'} for n in R.CASES},
                floors={n: {v: R.floors(n, v) for v in 'AB'} for n in R.CASES}, scalar_names=SCALAR_SYSTEMS, scalar={})
    lpol = [n for n in R.CASES if R.case(n)['lpol']]
    data['fields'] = {n: R.jacobi_field(R.case(n)) for n in lpol}
    data['refs_ind'] = {n: {p: R.reference_ind(n, p) for p in ('double', 'single')} for n in lpol}
    data['floors_ind'] = {n: R.floors_ind(n) for n in lpol}
    for name in SCALAR_SYSTEMS:
        s = NR.table_system(name)
        pairs, r, tt, slack, n_band = NR.table_reference(name)
        pos, box = np.array(s['pos']), np.array(s['box'])
        kappa, K1, K2, K3 = setup_ewald_parameters(s['rc'], 1e-4, box)
        c6 = np.asarray(s['params'][3])[:, None]
        disp = O.disp_energy_and_grad(pos, box, pairs, c6, NR.MSCALES, s['cov'], kappa, (K1, K2, K3), DISP_PMAX)
        cls = (O.pair_nbonds(s['cov'], pairs) - 1) % len(NR.MSCALES)
        w = c6[pairs[:, 0], 0] * c6[pairs[:, 1], 0] / NR.pair_distances(pos, box, pairs) ** 6
        disp['dm'] = np.array([w[cls == k].sum() for k in range(len(NR.MSCALES))])     # E_real is linear in mScales
        data['scalar'][name] = dict(pos=pos, box=box, rc=s['rc'], cov=s['cov'], params=s['params'], pmax=DISP_PMAX,
                                    pairs=np.ascontiguousarray(pairs, dtype=np.int32), tt=tt, disp=disp,
                                    ewald=(kappa, K1, K2, K3))
    path = d / 'refs.pkl'
    with open(path, 'wb') as fh:
        pickle.dump(data, fh)
    script = d / 'child.py'
    script.write_text(CHILD)
    return dict(dir=d, refs=str(path), script=str(script), data=data, dead=[], ratios={})


ABNORMAL = (124, 137, 134, 139, -6, -9, -11)


@pytest.mark.parametrize('tag,env,lanes,precs,refusals', SETTINGS, ids=[s[0] for s in SETTINGS])
def test_pair_kernels_row_by_row(shared, tag, env, lanes, precs, refusals):
    if shared['dead']:
        pytest.fail('not started: the child %s ended abnormally (%s)' % tuple(shared['dead'][0]))
    out = shared['dir'] / ('%s.json' % tag)
    r = subprocess.run(['timeout', '-k', '10', '180', sys.executable, shared['script'], shared['refs'], str(out), ','.join(precs),
                        '1' if refusals else '0'], env=dict(os.environ, **env), capture_output=True, text=True, cwd=ROOT)
    if r.returncode in ABNORMAL or r.returncode < 0:
        shared['dead'].append((tag, r.returncode))
    assert r.returncode == 0 and 'child ok' in r.stdout, (tag, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.load(open(out))
    data = shared['data']
    assert res['scalar'] == len(SCALAR_SYSTEMS) * len(precs) and res['refusals'] == int(refusals)
    minw = int(env.get('ADMP_PAIR_MINW', 0))
    worst = {}
    seen = set()
    for q in res['calls']:
        c = data['cases'][q['name']]
        what = (tag, q['name'], q['prec'], q['step'])
        seen.add((q['name'], q['prec'], q['step']))
        info = q['info']
        assert info[0] == lanes, (what, info)
        assert info[1] == (1 if c['cutoff'] else 0), (what, info)
        stale = q['step'] == 4 and bool(c['mono'].any())
        want_mono = 0 if (stale or q['which'] == 2 or (q['which'] == 0 and not q['flags'])) else 1
        assert info[2] == want_mono, (what, info)
        if q['which'] == 0:
            w = minw if minw else (2 if q['prec'] == 'single' else 1)
            assert info[3] == (w if c['lpol'] else 2), (what, info)
        else:
            assert info[3] == 0, (what, info)
        assert q['zeros_ok'], what        # pot[1:] and the field of a row walked in the charge-only forms; fld off the field rows
        assert q['iso_ok'], what          # the row of an atom without partners is exactly zero
        if q['same'] is not None:
            assert q['same'], what        # two calls on one table: bitwise equal rows (no global atomics in the row sums)
        if q['prec'] == 'double':
            assert all(v <= 1.0 for v in q['excess'].values()), (what, q['excess'])
            continue
        fl = data['floors'][q['name']][q['variant']] if q['which'] < 2 else data['floors_ind'][q['name']]
        for k, e in q['err'].items():
            if k == 'E' and q['which'] > 0:
                continue
            if fl[k] == 0.0:
                assert e == 0.0, (what, k, e)
                continue
            key = (q['name'], k if q['which'] < 2 else 'ind')
            worst[key] = max(worst.get(key, 0.0), e / fl[k])
    for name in R.CASES:
        line = ' '.join('%s %.2f' % (k, worst[(name, k)]) for k in ('E', 'grad', 'pot', 'fld', 'ind') if (name, k) in worst)
        if line:
            print('RATIO %-12s %-14s device error / host-f32 floor: %s' % (tag, name, line))
    for prec in precs:
        for name in R.CASES:
            steps = {s for (n_, p_, s) in seen if n_ == name and p_ == prec}
            assert steps == (set(range(10)) if data['cases'][name]['lpol'] else {0, 1, 4, 5, 8, 9}), (tag, name, prec, steps)
    print('SECS %-12s child: imports %.1f, pair cases %.1f, scalar systems %.1f (cumulative)' % ((tag,) + tuple(res['secs'])))
    if worst:
        top = max(worst, key=worst.get)
        print('RATIO %-12s largest %.2f (%s %s); bar %.0f' % (tag, worst[top], top[0], top[1], R.FLOOR_FACTOR))
    over = {k: v for k, v in worst.items() if v > R.FLOOR_FACTOR}
    assert not over, (tag, over)
