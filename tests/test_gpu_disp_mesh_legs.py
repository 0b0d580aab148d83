"""The spread and gather legs of dispersion PME word by word and row by row against the long-double reference of
tests/disp_mesh_ref.py: k_spread_bricks_scalar<1|2|3>, k_spread_bricks_typed<1|2|3>, k_interleave, k_gather_scalar<NCH, IL> and
its typed form, k_gather_value, k_scalar_self, k_types_check, k_type_counts, k_onehot (disp_kernels.hip), and the batch forms of
the electrostatics kernels on the site-row paths (launch_scalar_sites_batch, spread_sites(nb), launch_gather_field(nb),
launch_scale_add(nb)) -- each leg alone, through the C entries admp_disp_mesh_spread / admp_disp_mesh_gather, which run the
part functions of Engine::disp's own paths.  Inputs, reference and bars are proved sound without a GPU in
tests/test_disp_mesh_ref_cpu.py and tests/test_disp_scale_cpu.py.  The batched and mixing convolution passes between the legs
are not run here.

The switches are read once per process, so every setting gets a child process (disp_mesh_ref.CHILDREN):

    default      nothing set: site-row PerPower on the rocFFT meshes; (32, 17, 18) takes the direct DFT by mesh_path's own rule
                 (DftBatched, DftTyped); the refusals of the entries
    bricks       ADMP_SPREAD_BRICK_MIN=0: BricksTyped (single precision), BricksBatched, BricksPerPower; (32, 16, 18) has one
                 brick along y and must fall back to the site rows, and info8 must say so
    dft          ADMP_DFT=1: DftTyped, and DftBatched with a batched spread
    dft_bricks   ADMP_DFT=1 ADMP_SPREAD_BRICK_MIN=0: DftBatched, one spread per power

Per case, precision, pmax and (for a case with types) with and without the type table: the spread twice (word by word against
the reference meshes, unreached words exactly zero, all words finite, info8 as disp_mesh_ref.expected_path says, the second
call bit for bit the first on the fixed-point forms), the gather on white noise (a different seed per mesh of the batch) and,
up to 700 atoms, on one plane wave per mesh, the value gather of the parameter gradient, and the self word of both legs.
Typed cases: a coefficient one ulp off its type's, a type index of -1 and one of nt must be refused with the text an
evaluation gives, and the handle serves afterwards.  A child that faults, aborts or runs into its time limit ends the module.

Every child prints err / bar per call (run with -s).  Measured on an MI355X, largest err / bar (f64, f32), C unwidened:
brick spreads BricksBatched 0.999, 0.997, BricksPerPower 0.999, 0.997, BricksTyped 0.979 (f32 only); site-row spreads scan form
0.999, 0.986, brick form 0.965, 0.368 (the quantum term of the fixed-point forms is tight by construction); gradient gather
BricksBatched 0.045, 0.073, BricksPerPower 0.067, 0.081, BricksTyped 0.028, DftBatched 0.076, 0.088, DftTyped 0.038, 0.025,
PerPower 0.103, 0.065; value gather 0.308, 0.220.  Children: default 14.5 s, bricks 14.9 s (the composition check included),
dft 7.1 s, dft_bricks 7.5 s (2 s of each are imports; the first handles of a mesh build the plans, 1.3 to 3.6 s, every later
case takes under 0.1 s).  The self word found the typed paths' self term formed from the unrounded type table in single
precision; fixed.  Composition check, |grad - oracle| / |oracle|: 6.7e-14, 5.7e-14 in f64; 1.6e-6 to 2.5e-5 in f32.
info8's workgroup count is the dispersion launchers' own (disp_spread_groups, disp_gather_groups, disp_value_groups, which the
launchers call); the test holds it to the reference's brick rule and to the 32-atom groups padded to 8; the site-row paths,
whose legs run the electrostatics launchers, report -1."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import disp_mesh_ref as D
from tests import mesh_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import ctypes, json, pickle, sys, time
t_start = time.time()
sys.path.insert(0, %r)
import numpy as np
import torch
from admp_amd import settings, _lib
from admp_amd.disp_pme import ADMPDispPmeForce
from tests import mesh_ref as R

data = pickle.load(open(sys.argv[1], 'rb'))
tag = sys.argv[3]
out = {'calls': [], 'refusals': 0, 'typed_refusals': 0, 'secs': [time.time() - t_start]}
NP = lambda t: t.cpu().numpy().astype(np.float64)      # noqa: E731
L = _lib.load()


def force(c, K=None):
    f = ADMPDispPmeForce(c['box'], R.EmptyCov(c['n']), 4.0, 1e-4, 10)
    f.kappa = c['kappa']
    f.K1, f.K2, f.K3 = K or c['K']
    f.refresh_calculators()
    return f


def ratio(err, bar):
    """largest err / bar; a word whose bar is zero must be exact"""
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    if (err[bar == 0] != 0).any():
        return float('inf')
    ok = bar > 0
    return float((err[ok] / bar[ok]).max()) if ok.any() else 0.0


def set_types(f, c, keep, types=None):
    if c['types'] is None or types is False:
        _lib.check(f._h, L.admp_disp_set_types(f._h, 0, None, None), 'admp_disp_set_types')
        return
    t = torch.as_tensor(np.asarray(c['types'] if types is None else types, dtype=np.int32)).cuda()
    keep.append(t)
    _lib.check(f._h, L.admp_disp_set_types(f._h, int(c['nt']), t.data_ptr(), _lib.darr(np.ascontiguousarray(c['ctab']))),
               'admp_disp_set_types')


for name in data['names']:
    c = data['cases'][name]
    for prec in c['precs']:
        settings.PRECISION = prec
        t_case = time.time()
        f = force(c)
        keep = []
        for job in data['jobs'][name][prec]:
            pmax, typed = job['pmax'], job['typed']
            f.pmax = pmax
            set_types(f, c, keep, None if typed else False)
            rec = dict(name=name, prec=prec, pmax=pmax, typed=typed, spread=[], gather=[])
            meshes = []
            for rep in range(2):
                mesh, e_self, info = f.mesh_spread(c['pos'], c['box'], c['pairs'], c['c'])
                m = NP(mesh)
                meshes.append(m)
                key = (info['path'], info['form'])
                refs = job['spread'].get(key)
                s = dict(info=info, e_self=e_self, finite=bool(np.isfinite(m).all()), known=refs is not None)
                if refs is not None and len(refs) == len(m):
                    s['ratio'] = [ratio(np.abs(m[b] - refs[b]['mesh']), refs[b]['bar']) for b in range(len(m))]
                    s['unreached_zero'] = bool(all(not m[b][refs[b]['unreached']].any() for b in range(len(m))))
                rec['spread'].append(s)
            rec['same'] = bool(np.array_equal(meshes[0], meshes[1]))
            for g in job['gather']:
                grad, e_self, info = f.mesh_gather(c['pos'], c['box'], c['pairs'], c['c'], g['phi'], which=g['which'])
                rec['gather'].append(dict(kind=g['kind'], which=g['which'], info=info, e_self=e_self, nphi=len(g['phi']),
                                          finite=bool(torch.isfinite(grad).all()), ratio=ratio(np.abs(NP(grad) - g['ref']), g['bar'])))
            # a type table that does not describe c_list: refused with the text an evaluation gives; the handle serves afterwards
            if typed and job['typed_path']:
                msgs = []
                cbad = np.array(c['c'], dtype=np.float64)
                i = c['n'] - 1                                       # (an atom of the second workgroup of k_types_check: n >= 257)
                one_ulp = np.nextafter(np.asarray(cbad[i, 0], dtype=R.RT[prec]), R.RT[prec](np.inf))
                cbad[i, 0] = float(one_ulp)
                for what, cl, ty in (('ulp', cbad, None), ('minus_one', c['c'], -1), ('nt', c['c'], int(c['nt']))):
                    types = None
                    if ty is not None:
                        types = np.array(c['types'])
                        types[i] = ty
                    set_types(f, c, keep, types)
                    try:
                        f.mesh_spread(c['pos'], c['box'], c['pairs'], cl)
                        msgs.append((what, None))
                    except _lib.AdmpHipError as e:
                        msgs.append((what, str(e)))
                # ... and by the gather leg alone (BricksTyped checks the table before its gather picks a mesh by the type index)
                g0 = job['gather'][0]
                for what, cl, ty in (('gather_ulp', cbad, None), ('gather_minus_one', c['c'], -1)):
                    types = None
                    if ty is not None:
                        types = np.array(c['types'])
                        types[i] = ty
                    set_types(f, c, keep, types)
                    try:
                        f.mesh_gather(c['pos'], c['box'], c['pairs'], cl, g0['phi'], which=0)
                        msgs.append((what, None))
                    except _lib.AdmpHipError as e:
                        msgs.append((what, str(e)))
                set_types(f, c, keep)
                mesh, _, info = f.mesh_spread(c['pos'], c['box'], c['pairs'], c['c'])
                grad, _, _ = f.mesh_gather(c['pos'], c['box'], c['pairs'], c['c'], g0['phi'], which=0)
                rec['type_refusals'] = dict(msgs=msgs, i=i, serves=bool(np.array_equal(NP(mesh), meshes[0])), path=info['path'],
                                            gather_serves=ratio(np.abs(NP(grad) - g0['ref']), g0['bar']))
            out['calls'].append(rec)
        set_types(f, c, keep, False)
        del f
        out['secs'].append(time.time() - t_case)

# ---- composition: spread, the parent's float64 convolution of the REFERENCE meshes, gather -- against the oracle's gradient
out['composition'] = []
for job in data.get('composition', []):
    c = data['cases'][job['name']]
    settings.PRECISION = job['prec']
    f = force(c)
    keep = []
    f.pmax = job['pmax']
    set_types(f, c, keep, None if job['typed'] else False)
    mesh, _, info = f.mesh_spread(c['pos'], c['box'], c['pairs'], c['c'])
    m = NP(mesh)
    grad, _, ginfo = f.mesh_gather(c['pos'], c['box'], c['pairs'], c['c'], job['phi'], which=0)
    g = NP(grad)
    out['composition'].append(dict(name=job['name'], prec=job['prec'], pmax=job['pmax'], typed=job['typed'], path=info['path'],
                                   gather_path=ginfo['path'], nmesh=info['nmesh'], nphi=len(job['phi']),
                                   spread_ratio=[ratio(np.abs(m[b] - job['spread'][b]['mesh']), job['spread'][b]['bar']) for b in range(len(m))],
                                   grel=float(np.linalg.norm(g - job['g_oracle']) / np.linalg.norm(job['g_oracle']))))
    set_types(f, c, keep, False)
    del f

# ---- refusals: each before any launch; the handle serves a valid call afterwards
if tag == 'default':
    settings.PRECISION = 'double'
    c = data['cases']['n65_general']
    f = force(c)
    n = c['n']
    P = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()      # noqa: E731
    pos, cl = P(c['pos']), P(c['c'])
    mesh, phi, grad = P(np.zeros((3,) + tuple(c['K']))), P(np.ones((3,) + tuple(c['K']))), P(np.zeros((n, 3)))
    E, i8 = ctypes.c_double(0.0), (ctypes.c_int * 8)()
    box = _lib.darr(c['box'])
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    Eref = ctypes.byref(E)

    def spread(h, pos=pos, cl=cl, pmax=10, mesh=mesh, E=Eref, info=i8):
        return L.admp_disp_mesh_spread(h._h, p(pos), box, p(cl), pmax, 1, p(mesh), E, info)

    def gather(h, which=0, pos=pos, cl=cl, pmax=10, phi=phi, E=Eref, grad=grad, info=i8):
        return L.admp_disp_mesh_gather(h._h, p(pos), box, p(cl), pmax, p(phi), which, 1, E, p(grad), info)
    err = lambda h: L.admp_last_error(h._h)      # noqa: E731
    assert spread(f) != 0 and b'pairs must be set' in err(f)                             # state not set
    assert gather(f) != 0 and b'pairs must be set' in err(f)
    f.set_pairs(c['pairs'])
    assert spread(f) == 0 and gather(f) == 0 and gather(f, 1) == 0
    for kw in (dict(pos=None), dict(cl=None), dict(mesh=None), dict(E=None), dict(info=None)):
        assert spread(f, **kw) != 0 and b'null argument' in err(f), kw
    for kw in (dict(pos=None), dict(cl=None), dict(phi=None), dict(E=None), dict(grad=None), dict(info=None)):
        assert gather(f, **kw) != 0 and b'null argument' in err(f), kw
    for bad in (7, 4, 12):
        assert spread(f, pmax=bad) != 0 and b'pmax must be 6, 8 or 10' in err(f)
        assert gather(f, pmax=bad) != 0 and b'pmax must be 6, 8 or 10' in err(f)
    assert gather(f, 2) != 0 and b'which' in err(f) and gather(f, -1) != 0 and b'which' in err(f)
    assert spread(f) == 0 and gather(f) == 0                                             # still serving
    small = force(c, K=(5, 33, 35))                                                      # order-6 splines need 6 points
    small.set_pairs(c['pairs'])
    assert spread(small) != 0 and b'at least 6' in err(small)
    assert gather(small) != 0 and b'at least 6' in err(small)
    assert spread(f) == 0 and gather(f) == 0 and gather(f, 1) == 0
    slab = force(c)                                                                      # a slab handle of its own
    slab.set_pairs(c['pairs'])
    _lib.check(slab._h, L.admp_slab_configure(slab._h, 0, 2), 'admp_slab_configure')
    assert spread(slab) != 0 and b'single rank' in err(slab)
    assert gather(slab) != 0 and b'single rank' in err(slab) and gather(slab, 1) != 0 and b'single rank' in err(slab)
    assert spread(f) == 0 and gather(f) == 0 and gather(f, 1) == 0                        # still serving after the last refusal
    out['refusals'] = 1

out['secs'].append(time.time() - t_start)
json.dump(out, open(sys.argv[2], 'w'))
print('child ok')
''' % ROOT

TYPES_TEXT = 'c_list rows differ from the coefficients of their types'
ABNORMAL = (124, 137, 134, 139, -6, -9, -11)
FIXED_POINT = {'scan', 'bricks', None}        # spread forms that sum integers: two calls agree bit for bit (None: the brick paths)


def _plain(c):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _mesh_entry(r, bar):
    return dict(mesh=np.asarray(r.mesh, dtype=np.float64), bar=np.asarray(bar, dtype=np.float64), unreached=r.unreached)


def _jobs(name, prec, env):
    """what a child runs for one case and precision, with the references of every (path, form) its calls may report"""
    c = D.case(name)
    jobs = []
    for pmax in c['pmaxes']:
        nch = (pmax - 4) // 2
        for typed in ((False, True) if c['types'] is not None else (False,)):
            path, nmesh, per_type = D.expected_path(c['K'], c['n'], env, pmax, c['nt'] if typed else 0, prec)
            refs = D.mesh_refs(name, prec, pmax, per_type)
            cr = D.rounded_c(c, prec)
            if path in D.BRICK_PATHS:
                form = None
                entries = [_mesh_entry(r, D.spread_bar_bricks(r, None if per_type else cr[:, b], prec, typed=per_type)) for b, r in enumerate(refs)]
            else:
                form = D.expected_form(c['K'], c['n'], env)
                entries = [_mesh_entry(r, r.bar(form)) for r in refs]
            gathers = []
            for kind in (('noise', 'wave') if c['n'] <= 700 else ('noise',)):
                phi = D.phi_batch(c, prec, nmesh, kind)
                ref, bar = D.gather_reference(name, prec, pmax, per_type, phi)
                gathers.append(dict(kind=kind, which=0, phi=phi, ref=ref, bar=bar))
                if not typed:
                    phi1 = D.phi_batch(c, prec, nch, kind)
                    ref1, bar1 = D.value_reference(name, prec, pmax, phi1)
                    gathers.append(dict(kind=kind, which=1, phi=phi1, ref=ref1, bar=bar1))
            jobs.append(dict(pmax=pmax, typed=typed, typed_path=path in D.TYPED_PATHS and c['n'] >= 257, spread={(path, form): entries},
                             gather=gathers, expect=dict(path=path, nmesh=nmesh, per_type=per_type, form=form)))
    return jobs


def _composition_job(name, pmax, typed, prec, env):
    c = D.case(name)
    path, nmesh, per_type = D.expected_path(c['K'], c['n'], env, pmax, c['nt'] if typed else 0, prec)
    assert path in D.BRICK_PATHS and per_type == typed
    phi, g_oracle = D.composition(name, prec, pmax, per_type)
    cr = D.rounded_c(c, prec)
    refs = D.mesh_refs(name, prec, pmax, per_type)
    spread = [_mesh_entry(r, D.spread_bar_bricks(r, None if per_type else cr[:, b], prec, typed=per_type)) for b, r in enumerate(refs)]
    return dict(name=name, pmax=pmax, typed=typed, prec=prec, path=path, nmesh=nmesh, phi=phi, g_oracle=g_oracle, spread=spread)


@pytest.fixture(scope='module')
def shared(tmp_path_factory):
    d = tmp_path_factory.mktemp('disp_mesh_legs')
    script = d / 'child.py'
    script.write_text(CHILD)
    return dict(dir=d, script=str(script), dead=[], results={}, data={})


def run_child(shared, tag):
    if tag in shared['results']:
        return shared['results'][tag], shared['data'][tag]
    if shared['dead']:
        pytest.fail('not started: the child %s ended abnormally (%s)' % tuple(shared['dead'][0]))
    env, meshes = D.CHILDREN[tag]
    names = [n for n in D.CASES if D.case(n)['K'] in meshes]
    data = dict(names=names, cases={n: _plain(D.case(n)) for n in names},
                jobs={n: {prec: _jobs(n, prec, env) for prec in D.case(n)['precs']} for n in names})
    if tag == 'bricks':
        data['composition'] = [_composition_job(*q, env=env) for q in D.COMPOSITION]
    refs = shared['dir'] / ('%s.pkl' % tag)
    with open(refs, 'wb') as fh:
        pickle.dump(data, fh)
    out = shared['dir'] / ('%s.json' % tag)
    r = subprocess.run(['timeout', '-k', '10', '240', sys.executable, shared['script'], str(refs), str(out), tag],
                       env=dict(os.environ, **env), capture_output=True, text=True, cwd=ROOT)
    if r.returncode in ABNORMAL or r.returncode < 0:
        shared['dead'].append((tag, r.returncode))
    assert r.returncode == 0 and 'child ok' in r.stdout, (tag, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    shared['results'][tag] = json.load(open(out))
    shared['data'][tag] = data
    return shared['results'][tag], data


NEED = {'default': {'PerPower', 'DftBatched', 'DftTyped'}, 'bricks': {'BricksTyped', 'BricksBatched', 'BricksPerPower', 'PerPower'},
        'dft': {'DftTyped', 'DftBatched', 'PerPower'}, 'dft_bricks': {'DftBatched'}}


@pytest.mark.parametrize('tag', list(D.CHILDREN))
def test_spread_and_gather_legs_word_by_word(shared, tag):
    res, data = run_child(shared, tag)
    assert res['refusals'] == int(tag == 'default')
    env = D.CHILDREN[tag][0]
    worst, paths_seen, over, n_type_refusals = {}, set(), [], 0

    def note(key, v, what):
        worst[key] = max(worst.get(key, 0.0), v)
        if not v <= 1.0:
            over.append((what, key, v))
    it = iter(res['calls'])
    for name in data['names']:
        c = data['cases'][name]
        for prec in c['precs']:
            for job in data['jobs'][name][prec]:
                q = next(it)
                ex = job['expect']
                what = (tag, name, prec, job['pmax'], 'typed' if job['typed'] else 'untyped')
                assert (q['name'], q['prec'], q['pmax'], q['typed']) == (name, prec, job['pmax'], job['typed'])
                nch = (job['pmax'] - 4) // 2
                sref, sbar, st = D.self_reference(c, prec, job['pmax'])
                line = []
                for s in q['spread']:
                    info = s['info']
                    assert info['path'] == ex['path'] and info['nmesh'] == ex['nmesh'] and info['per_type'] == ex['per_type'], (what, info, ex)
                    assert tuple(info['bricks']) == R.make_bricks(c['K']) and info['form'] == ex['form'], (what, info, ex)
                    # the launcher's own count: one workgroup per brick of the reference's brick rule; the site-row paths report none
                    assert info['groups'] == (int(np.prod(R.make_bricks(c['K']))) if ex['path'] in D.BRICK_PATHS else -1), (what, info)
                    assert s['known'] and s['finite'] and s['unreached_zero'], (what, s)
                    for b, v in enumerate(s['ratio']):
                        note(('spread', ex['path'], ex['form'], prec), v, what + ('mesh %d' % b,))
                    line.append('/'.join('%.3f' % v for v in s['ratio']))
                    # the self word of the spread leg: the site-row paths of the powers sum it with their rows
                    if ex['path'] in ('PerPower', 'DftBatched'):
                        assert abs(s['e_self'] - sref) <= sbar, (what, s['e_self'], sref, sbar)
                    else:
                        assert s['e_self'] == 0.0, (what, s['e_self'])
                if ex['form'] in FIXED_POINT:
                    assert q['same'], (what, 'two spreads differ')
                paths_seen.add(ex['path'])
                gl = []
                for g in q['gather']:
                    assert g['finite'], (what, g)
                    if g['which'] == 0:
                        assert g['info']['path'] == ex['path'] and g['info']['nmesh'] == ex['nmesh'] == g['nphi'], (what, g)
                        # k_gather_scalar: 32 atoms per workgroup, the grid padded to the 8 XCDs
                        assert g['info']['groups'] == ((((c['n'] + 31) // 32 + 7) // 8) * 8 if ex['path'] in D.BRICK_PATHS else -1), (what, g)
                        note(('gather', ex['path'], prec), g['ratio'], what + (g['kind'],))
                        # the self word: formed after the convolution on the brick and typed paths; both legs give the reference
                        leg = q['spread'][0]['e_self'] + g['e_self']
                        assert abs(leg - sref) <= sbar, (what, leg, sref, sbar)
                        if ex['path'] in D.TYPED_PATHS:
                            assert abs(g['e_self'] - st) <= sbar, (what, g['e_self'], st)
                    else:
                        assert g['info']['groups'] == (c['n'] + 127) // 128 and g['e_self'] == 0.0, (what, g)
                        note(('value', prec), g['ratio'], what + (g['kind'],))
                    gl.append('%s%d %.3f' % (g['kind'][0], g['which'], g['ratio']))
                if job['typed'] and job['typed_path']:
                    tr = q['type_refusals']
                    assert tr['serves'] and tr['path'] == ex['path'] and tr['i'] >= 256, (what, tr)
                    assert [m[0] for m in tr['msgs']] == ['ulp', 'minus_one', 'nt', 'gather_ulp', 'gather_minus_one']
                    assert tr['gather_serves'] <= 1.0, (what, tr)
                    assert all(m[1] is not None and TYPES_TEXT in m[1] for m in tr['msgs']), (what, tr)
                    n_type_refusals += 1
                print('RATIO %-10s %-22s %-6s pmax %2d %-7s %-14s %-6s spread (2 calls, per mesh): %s | gather: %s'
                      % (tag, name, prec, job['pmax'], what[4], ex['path'], ex['form'], ' '.join(line), ' '.join(gl)))
    assert next(it, None) is None
    assert NEED[tag] <= paths_seen, (tag, NEED[tag] - paths_seen)
    if tag in ('bricks', 'dft'):
        assert n_type_refusals >= 1
    if tag == 'bricks':      # the one-brick mesh fell back to the site rows, in the scan form: as the calls themselves reported
        fell = [s['info'] for q in res['calls'] if q['name'] == 'n65_one_brick_y' for s in q['spread']]
        assert len(fell) == 12 and all(i['path'] == 'PerPower' and i['form'] == 'scan' and i['groups'] == -1 for i in fell), fell
    for key in sorted(worst, key=str):
        print('WORST %-10s %-44s err / bar %.3g' % (tag, key, worst[key]))
    print('SECS  %-10s child: imports %.1f, total %.1f; per case and precision: %s'
          % (tag, res['secs'][0], res['secs'][-1], ' '.join('%.1f' % s for s in res['secs'][1:-1])))
    assert not over, over[:20]


def test_composition_meets_the_oracle(shared):
    """The one check across the legs, no new bars: for two cases per brick path the spread runs, the parent forms phi_p = N
    ifftn(G_p fftn(mesh_p)) in float64 from the REFERENCE meshes (psi_t per type on the typed path), the gather takes it, and
    the gradient must meet oracle.admp_oracle.disp_energy_and_grad's reciprocal gradient of that heterogeneous system within
    tests/test_gpu_disp_paths.py's tolerance.  Ties mesh layout, per-type versus per-power meaning, and the sign and Jac factor of
    the gradient to the oracle."""
    from tests.test_gpu_disp_paths import TOL
    res, data = run_child(shared, 'bricks')
    assert len(res['composition']) == len(D.COMPOSITION) == 6
    seen = {}
    for q, job in zip(res['composition'], data['composition']):
        print('COMPOSITION %-20s %-6s pmax %2d %-14s spread err / bar %s | |grad - oracle| / |oracle| = %.3g'
              % (q['name'], q['prec'], q['pmax'], q['path'], '/'.join('%.3f' % v for v in q['spread_ratio']), q['grel']))
        assert q['path'] == q['gather_path'] == job['path'] and q['nmesh'] == q['nphi'] == job['nmesh'], (q, job['path'])
        assert all(v <= 1.0 for v in q['spread_ratio']), q
        assert q['grel'] < max(TOL[q['prec']], 1e-8), q
        seen[q['path']] = seen.get(q['path'], 0) + 1
    assert seen == {'BricksTyped': 2, 'BricksBatched': 2, 'BricksPerPower': 2}, seen
