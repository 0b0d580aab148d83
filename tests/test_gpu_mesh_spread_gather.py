"""The mesh spread and gather kernels word by word and row by row against the long-double reference of tests/mesh_ref.py:
k_spread_scan, k_spread_planes, k_bin + k_scan_small + k_spread_bricks (recip_kernels.hip), zy_plane_spread inside the forward
plane kernel (dft_kernels.hip), k_gather_staged with the atom-side energy and k_gather_field_staged over the handle's list of
polarizable sites -- each alone, through the C entries admp_mesh_spread / admp_mesh_gather (what an evaluation does up to that
kernel, through the evaluation's own launchers).  Inputs, reference and bars are proved sound without a GPU in
tests/test_mesh_ref_cpu.py.

The switches that pick the spread form are read once per process, so every setting gets a child process:

    scan          nothing set: fewer than 20 000 atoms take k_spread_scan
    bricks        ADMP_SPREAD_BRICK_MIN=0: the binned form (meshes with one brick on some axis keep the scan form)
    planes        ADMP_SPREAD_SCAN_MAX=0: global float atomics (same exception)
    plane_kernel  ADMP_DFT=1: which = 1 spreads inside the forward plane kernel, double precision, where
                  dft_zy_spread_fits holds (of the meshes here: 33 x 31 x 47); everything else must be refused

A child runs every case in both types: four which = 0 spreads (stencil-window scale; entry-count scale; no stencil records;
the first again: test_repeated_spread_is_bit_for_bit), which = 1 (phi against N ifftn(G fftn(mesh_ref)) at the flat
kappa of tests/test_gpu_mesh_convolve.py, or the refusal), the gather on white noise (and on a plane wave for the small
cases) and the field gather.  info8 / info4 must name the form meant, the brick counts, the scale flag and the workgroups.
Bars: mesh_ref.SpreadRef.bar / GatherRef.bars, i.e. DEVICE_FACTOR x C_HOST x u x W + the fixed-point quanta (+ the summation
term of the forms that sum in the handle's type); phi: B_word of the convolution + sumG |bar|_1.  Exact: words that no
stencil reaches are zero; rows outside the polarizable list are zero in the field gather.

The default child also runs the refusals: a mesh axis below 6, a slab handle, null arguments, an unknown `which`, the field
gather on a non-polarizable handle.  A child that faults, aborts or runs into its time limit ends the module.

Every child prints err / bar per case (run with -s).  Measured on an MI355X, largest err / bar (f64, f32): scan form 0.955,
0.930; planes form 0.115, 0.247; brick form 0.955, 0.951 (the quantum term of these two fixed-point forms is tight by
construction: a word that one term reaches is off by up to half a quantum, which is the whole bar there); phi behind the plane kernel 2.5e-5 (f64 only); gather
pot 0.139, 0.062, grad 0.054, 0.031, fld 0.092, 0.047, field gather 0.049, 0.036, energy word 2.7e-3, 1.3e-3.  A child takes
19 to 20 s, 2 s of it imports: the first handle of a mesh and type builds the transform plans, 1.0 to 1.8 s for each of the 11
mesh-type pairs; every later case takes 0.01 s.  That is more than the few seconds asked of a child; the kernels take
microseconds, so cutting the case list in two would give eight children of 10 s and the same total."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import mesh_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [('scan', {}), ('bricks', {'ADMP_SPREAD_BRICK_MIN': '0'}), ('planes', {'ADMP_SPREAD_SCAN_MAX': '0'}),
            ('plane_kernel', {'ADMP_DFT': '1'})]
SPREAD_FLAGS = (1, 0, 3, 1)

CHILD = r'''
import ctypes, json, pickle, sys, time
t_start = time.time()
sys.path.insert(0, %r)
import numpy as np
import torch
from admp_amd import settings, _lib
from admp_amd.pme import ADMPPmeForce
from tests import mesh_ref as R

data = pickle.load(open(sys.argv[1], 'rb'))
tag = sys.argv[3]
settings.REFERENCE_KPOINT_ORDER = False      # (the G table of the convolution: frequencies axis by axis)
out = {'calls': [], 'refusals': 0, 'secs': [time.time() - t_start]}
NP = lambda t: None if t is None else t.cpu().numpy().astype(np.float64)      # noqa: E731


def force(c, K=None, lpol=None, kappa=None):
    lp = c['lpol'] if lpol is None else lpol
    f = ADMPPmeForce(c['box'], c['axis_type'], c['axis_indices'], R.EmptyCov(c['n']), 4.0, 1e-4, 2, lpol=lp)
    f.kappa = c['kappa'] if kappa is None else kappa
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


for name in data['names']:
    c = data['cases'][name]
    for prec in c['precs']:
        settings.PRECISION = prec
        t_case = time.time()
        ref = data['refs'][name][prec]
        f = force(c)
        kw = dict(pol=c['pol'], tholes=c['thole'], U=c['U']) if c['lpol'] else {}
        rec = dict(name=name, prec=prec, spread=[], gather=[])
        meshes = []
        for flags in SPREAD_FLAGS_:
            mesh, info = f.mesh_spread(c['pos'], c['box'], c['pairs'], c['Q'], which=0, flags=flags, **kw)
            m = NP(mesh)
            meshes.append(m)
            form = info['form']
            rec['spread'].append(dict(flags=flags, info=info, ratio=ratio(np.abs(m - ref['mesh']), ref['bar'][form]) if form in ref['bar'] else None,
                                      unreached_zero=bool(not m[ref['unreached']].any()), finite=bool(np.isfinite(m).all())))
        rec['same'] = bool(np.array_equal(meshes[0], meshes[3]))
        rec['same_ratio'] = ratio(np.abs(meshes[0] - meshes[3]), ref['bar'][form])
        # which = 1: the forward plane kernel spreads, or the entry refuses
        try:
            phi, info = f.mesh_spread(c['pos'], c['box'], c['pairs'], c['Q'], which=1, flags=1, **kw)
            p = NP(phi)
            rec['plane'] = dict(info=info, ratio=ratio(np.abs(p - ref['phi']), np.full(p.shape, ref['bar_phi'])) if 'phi' in ref else None)
            phi2, info2 = f.mesh_spread(c['pos'], c['box'], c['pairs'], c['Q'], which=1, flags=3, **kw)
            rec['plane']['ratio_norecords'] = ratio(np.abs(NP(phi2) - ref['phi']), np.full(p.shape, ref['bar_phi'])) if 'phi' in ref else None
            rec['plane']['records'] = (info['records'], info2['records'])
        except _lib.AdmpHipError as e:
            rec['plane'] = dict(refused=str(e))
        for kind, g in ref['gather'].items():
            r = f.mesh_gather(c['pos'], c['box'], c['pairs'], c['Q'], g['phi'], which=0, **kw)
            q = dict(kind=kind, which=0, info=r['info'], pot=ratio(np.abs(NP(r['pot']) - g['pot']), g['bar_pot']),
                     grad=ratio(np.abs(NP(r['grad']) - g['grad']), g['bar_grad']), E=abs(r['E'] - g['E']) / g['bar_E'])
            if c['lpol']:
                q['fld'] = ratio(np.abs(NP(r['fld']) - g['fld']), g['bar_fld'])
            rec['gather'].append(q)
            if c['lpol']:
                r = f.mesh_gather(c['pos'], c['box'], c['pairs'], c['Q'], g['phi'], which=1, **kw)
                act = c['pol'] > 0
                fld = NP(r['fld'])
                rec['gather'].append(dict(kind=kind, which=1, info=r['info'], fld=ratio(np.abs(fld - g['fld'])[act], g['bar_fld'][act]),
                                          zeros_ok=bool(not fld[~act].any()), n_act=int(act.sum())))
        del f
        rec['secs'] = time.time() - t_case
        out['calls'].append(rec)

out['secs'].append(time.time() - t_start)
# ---- refusals: each before a kernel is launched, and the handle serves a valid call afterwards
if tag == 'scan':
    settings.PRECISION = 'double'
    c = data['cases']['bricks2_n65']
    L = _lib.load()
    f, g = force(c), force(c, lpol=False)
    n = c['n']
    P = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()      # noqa: E731
    pos, Q, pol, th, U = P(c['pos']), P(c['Q']), P(c['pol']), P(c['thole']), P(c['U'])
    mesh, pot, grad, fld = P(np.zeros(c['K'])), P(np.zeros((n, 9))), P(np.zeros((n, 3))), P(np.zeros((n, 3)))
    E, i8, i4 = ctypes.c_double(0.0), (ctypes.c_int * 8)(), (ctypes.c_int * 4)()
    box = _lib.darr(c['box'])
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def spread(h, which=0, pos=pos, Q=Q, pol=pol, U=U, mesh=mesh, info=i8):
        return L.admp_mesh_spread(h._h, p(pos), box, p(Q), p(pol), p(th), p(U), which, 1, 1, p(mesh), info)

    def gather(h, which=0, phi=mesh, pot=pot, grad=grad, fld=fld, info=i4, pol=pol):
        return L.admp_mesh_gather(h._h, p(pos), box, p(Q), p(pol), p(th), p(U), p(phi), which, 1, ctypes.byref(E), p(pot), p(grad),
                                  p(fld), info)
    assert spread(f) != 0 and b'pairs must be set' in L.admp_last_error(f._h)            # no pairs set
    assert gather(f) != 0 and b'pairs must be set' in L.admp_last_error(f._h)
    f.set_pairs(c['pairs'])
    g.set_pairs(c['pairs'])
    assert spread(f) == 0 and gather(f) == 0
    for kw in (dict(pos=None), dict(Q=None), dict(pol=None), dict(U=None), dict(mesh=None), dict(info=None)):
        assert spread(f, **kw) != 0, kw
    for kw in (dict(phi=None), dict(pot=None), dict(grad=None), dict(fld=None), dict(info=None), dict(pol=None)):
        assert gather(f, **kw) != 0, kw
    assert gather(f, 1, fld=None) != 0 and gather(f, 1, pot=None, grad=None) == 0
    assert spread(f, 2) != 0 and spread(f, -1) != 0 and b'which' in L.admp_last_error(f._h)
    assert gather(f, 2) != 0 and b'which' in L.admp_last_error(f._h)
    assert spread(f, 1) != 0 and b'plane kernel' in L.admp_last_error(f._h)              # rocFFT mesh: never another path
    assert gather(g, 1) != 0 and b'polarizable' in L.admp_last_error(g._h)               # field gather, non-polarizable handle
    assert spread(g, pol=None, U=None) == 0 and gather(g, fld=None, pol=None) == 0
    small = force(c, K=(5, 18, 33))                                                      # order-6 splines need 6 points
    small.set_pairs(c['pairs'])
    assert spread(small) != 0 and b'at least 6' in L.admp_last_error(small._h)
    assert gather(small) != 0 and b'at least 6' in L.admp_last_error(small._h)
    assert spread(f) == 0 and gather(f) == 0 and gather(f, 1) == 0                        # still serving
    _lib.check(f._h, L.admp_slab_configure(f._h, 0, 2), 'admp_slab_configure')
    assert spread(f) != 0 and b'single rank' in L.admp_last_error(f._h)                  # slab handle
    assert gather(f) != 0 and b'single rank' in L.admp_last_error(f._h)
    out['refusals'] = 1

out['secs'].append(time.time() - t_start)
json.dump(out, open(sys.argv[2], 'w'))
print('child ok')
''' % ROOT
CHILD = CHILD.replace('SPREAD_FLAGS_', repr(SPREAD_FLAGS))


def _plain(c):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


@pytest.fixture(scope='module')
def shared(tmp_path_factory):
    """cases, references and bars of tests/mesh_ref.py, computed once and written to one file"""
    d = tmp_path_factory.mktemp('mesh_spread_gather')
    data = dict(names=R.CASES, cases={}, refs={})
    kappas = {}
    for name in R.CASES:
        c = _plain(R.case(name))
        data['refs'][name] = {}
        for prec in c['precs']:
            r = R.spread_ref(name, prec)
            ref = dict(mesh=np.asarray(r.mesh, dtype=np.float64), unreached=r.unreached,
                       bar={form: r.bar(form) for form in ('scan', 'planes', 'bricks')}, gather={})
            if R.plane_spread_fits(c['K'], c['n'], prec):
                cv = R.convolved(r)
                kappas[name] = cv['kappa']
                ref['phi'] = cv['phi']
                ref['bar_phi'] = cv['B_word'] + cv['sumG'] * float(r.bar('plane_kernel').sum())
            for kind in (('noise', 'wave') if c['n'] <= 700 else ('noise',)):
                g = R.gather_ref(name, prec, kind)
                b = g.bars()
                phi = R.phi_noise(c, prec) if kind == 'noise' else R.phi_wave(c, prec)
                ref['gather'][kind] = dict(phi=phi, pot=g.pot, grad=g.grad, fld=g.fld, E=g.E, bar_pot=b['pot'], bar_grad=b['grad'],
                                           bar_fld=b['fld'], bar_E=b['E'])
            data['refs'][name][prec] = ref
        c['kappa'] = kappas.get(name, 3.0)        # (only the plane kernel's convolution reads the G table)
        data['cases'][name] = c
    path = d / 'refs.pkl'
    with open(path, 'wb') as fh:
        pickle.dump(data, fh)
    script = d / 'child.py'
    script.write_text(CHILD)
    return dict(dir=d, refs=str(path), script=str(script), data=data, dead=[], results={})


ABNORMAL = (124, 137, 134, 139, -6, -9, -11)


def expected_form(tag, K, n):
    """the launcher's rule: one brick on an axis -> scan; at least ADMP_SPREAD_BRICK_MIN atoms (20 000; 0 in the bricks child), or
    4096 atoms and 24 per brick -> bricks (the 8192-atom case, in every child); else scan, or planes above ADMP_SPREAD_SCAN_MAX"""
    nb = R.make_bricks(K)
    if min(nb) == 1:
        return 'scan'
    brick_min = 0 if tag == 'bricks' else 20000
    if n >= brick_min or (n >= 4096 and n >= 24 * nb[0] * nb[1] * nb[2]):
        return 'bricks'
    return 'planes' if tag == 'planes' else 'scan'


def run_child(shared, tag):
    """the child of one setting, started once; its results serve every test of the module"""
    if tag in shared['results']:
        return shared['results'][tag]
    if shared['dead']:
        pytest.fail('not started: the child %s ended abnormally (%s)' % tuple(shared['dead'][0]))
    out = shared['dir'] / ('%s.json' % tag)
    r = subprocess.run(['timeout', '-k', '10', '180', sys.executable, shared['script'], shared['refs'], str(out), tag],
                       env=dict(os.environ, **dict(SETTINGS)[tag]), capture_output=True, text=True, cwd=ROOT)
    if r.returncode in ABNORMAL or r.returncode < 0:
        shared['dead'].append((tag, r.returncode))
    assert r.returncode == 0 and 'child ok' in r.stdout, (tag, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    shared['results'][tag] = json.load(open(out))
    return shared['results'][tag]


@pytest.mark.parametrize('form', ['scan', 'bricks'])
def test_repeated_spread_is_bit_for_bit(shared, form):
    """Two which = 0 calls with the same flags on one handle must agree bit for bit on the scan and brick forms.  This test
    found both forms wanting.  The brick form sums integers, but a group of its class sort in which two classes met took the
    general form for all its entries, and which entries of the lower class fell into it changed from call to call (places are
    handed out in arrival order): seen once, plane_n3073 in double precision, 0.05 of the bar.  Every class now starts on a
    group boundary.  It also found that the scan form did not: its LDS tile was summed by ds_add_f64 in arrival
    order (spread_entry_list: 256 threads add the columns of up to 32 entries at once, and the entry list itself is filled by
    an LDS counter in arrival order), so that 10 of the 11 double precision cases differed between two calls, by 0.001 to
    0.016 of the bar.  The scan form now sums 64-bit fixed-point words at both precisions, scaled by the brick form's f64 rule
    from a bound pass over the brick's own entries, and its bar carries that quantum."""
    res = run_child(shared, form)
    data = shared['data']
    differ = []
    for q in res['calls']:
        if expected_form(form, data['cases'][q['name']]['K'], data['cases'][q['name']]['n']) == form and not q['same']:
            differ.append((q['name'], q['prec'], q['same_ratio']))
    for d in differ:
        print('REPEAT %-8s %-14s %-6s two calls differ by %.3g of the bar' % ((form,) + d))
    assert not differ, (form, differ)


@pytest.mark.parametrize('tag,env', SETTINGS, ids=[s[0] for s in SETTINGS])
def test_spread_and_gather_word_by_word(shared, tag, env):
    res = run_child(shared, tag)
    data = shared['data']
    assert res['refusals'] == int(tag == 'scan')
    worst, forms_seen, seen = {}, set(), set()

    def note(key, v):
        worst[key] = max(worst.get(key, 0.0), v)
    for q in res['calls']:
        c = data['cases'][q['name']]
        what = (tag, q['name'], q['prec'])
        seen.add((q['name'], q['prec']))
        form = expected_form(tag, c['K'], c['n'])
        line = []
        for s in q['spread']:
            info, flags = s['info'], s['flags']
            assert info['form'] == form, (what, info)
            assert tuple(info['bricks']) == R.make_bricks(c['K']), (what, info)
            assert info['tight'] == int(form == 'bricks' and q['prec'] == 'single' and bool(flags & 1)), (what, flags, info)
            assert info['records'] == int(not flags & 2) and info['path'] is None, (what, flags, info)
            assert s['finite'] and s['unreached_zero'], (what, flags)
            forms_seen.add((form, q['prec']))
            note((form, q['prec']), s['ratio'])
            line.append('%.3f' % s['ratio'])
        fits = (tag == 'plane_kernel' or R.direct_dft_by_default(c['K'])) and R.plane_spread_fits(c['K'], c['n'], q['prec'])
        if fits:
            p = q['plane']
            assert 'refused' not in p, (what, p)
            assert p['info']['form'] == 'plane_kernel' and p['info']['path'] == 'direct_planes' and p['records'] == [1, 0], (what, p)
            forms_seen.add(('plane_kernel', q['prec']))
            note(('plane_kernel', q['prec']), max(p['ratio'], p['ratio_norecords']))
            line.append('phi %.2e %.2e' % (p['ratio'], p['ratio_norecords']))
        else:
            assert 'refused' in q['plane'] and 'plane kernel' in q['plane']['refused'], (what, q['plane'])
        gl = []
        for g in q['gather']:
            n_rows = c['n'] if g['which'] == 0 else g['n_act']
            groups = (n_rows + 31) // 32
            assert list(g['info']) == [g['which'], n_rows, groups, (groups + 7) // 8 * 8], (what, g)
            if g['which'] == 1:
                assert g['zeros_ok'], what
                note(('gather_field', q['prec']), g['fld'])
                gl.append('field %.3f' % g['fld'])
                continue
            for k in ('pot', 'grad', 'fld', 'E'):
                if k in g:
                    note(('gather_' + k, q['prec']), g[k])
            gl.append('%s pot %.3f grad %.3f E %.3f' % (g['kind'], g['pot'], g['grad'], g['E']))
        print('RATIO %-12s %-14s %-6s spread err / bar (flags 1, 0, 3, 1): %s | gather: %s | %.2f s' % (tag, q['name'], q['prec'], ' '.join(line), '; '.join(gl), q['secs']))
    want = {(n_, p_) for n_ in R.CASES for p_ in data['cases'][n_]['precs']}      # every case runs in every child
    assert seen == want, (tag, want - seen)
    # every form meant for this child ran, in the types it exists in
    need = {('scan', 'double'), ('scan', 'single')}
    if tag in ('bricks', 'planes'):
        need |= {(tag, 'double'), (tag, 'single')}
    need |= {('plane_kernel', 'double')}      # (33 x 31 x 47 takes the direct DFT in every child: 31 and 47 are prime)
    assert need <= forms_seen, (tag, need - forms_seen)
    assert {('gather_pot', 'double'), ('gather_pot', 'single'), ('gather_field', 'double'), ('gather_field', 'single')} <= set(worst)
    for key in sorted(worst):
        print('WORST %-12s %-14s %-6s err / bar %.3g' % ((tag,) + key + (worst[key],)))
    print('SECS  %-12s child: imports %.1f, cases %.1f, refusals %.1f (cumulative)' % ((tag,) + tuple(res['secs'])))
    over = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not over, (tag, over)
