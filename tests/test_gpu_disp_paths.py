"""Which reciprocal-space path a dispersion PME call takes (engine.hip `disp`, chosen by csrc/disp_plan.h `disp_path`), pinned
by the launch counts of its mesh labels, and the argument refusals of the scalar entry points with their texts.

One child process per environment (ADMP_SPREAD_BRICK_MIN is read once per process, ADMP_DFT at each plan set-up), every case of
an environment in that child.  Per case: one warm call, profile(True), profile_reset(), one call, profile_report(); the counts of
MESH_LABELS (a missing label counts 0, other labels are ignored) must equal the table of the case, and the call must meet
oracle.admp_oracle.disp_energy_and_grad, computed once per (mesh, pmax) in this process and handed to the children.

System and tolerances of the brick test of tests/test_gpu_parity.py: water_system(216, 11, True), 648 atoms, rc 4.0, ethresh 1e-4;
energy within tol * max|parts|, gradient rel < max(tol, 1e-8), tol = 1e-9 in double and 5e-4 in single.

The two typed paths share their labels with the batched ones; they are told apart by a wrong type table (one coefficient times
1.5 through admp_disp_set_types): a typed path refuses the call ('types' in the text), every other path never reads the table and
still meets the oracle."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RC, ETHRESH = 4.0, 1e-4
TOL = {'double': 1e-9, 'single': 5e-4}
DFT5 = ('dft_z_r2c', 'dft_y_fwd', 'dft_x_kspace', 'dft_y_inv', 'dft_z_c2r')
MESH_LABELS = ('atom_bases', 'disp_pair', 'scalar_sites', 'spread', 'interleave', 'gather_field', 'scale_add', 'scalar_self') + \
    DFT5 + ('dft_zy_fwd', 'dft_yz_inv', 'rocfft_r2c', 'rocfft_c2r', 'rocfft_r2c_yz', 'rocfft_c2r_yz', 'kspace', 'fftx_kspace')


def counts(**kw):
    c = dict.fromkeys(MESH_LABELS, 0)
    c['disp_pair'] = 1
    for k, v in kw.items():
        if k == 'dft5':
            c.update(dict.fromkeys(DFT5, v))
        else:
            assert k in c, k
            c[k] = v
    return c


FUSED_X = dict(atom_bases=1, spread=1, rocfft_r2c_yz=1, fftx_kspace=1, rocfft_c2r_yz=1, gather_field=1)
BRICKS_TYPED = counts(**FUSED_X)
BRICKS_BATCHED = counts(interleave=1, scalar_self=1, **FUSED_X)
BRICKS_PER_POWER_FX = counts(scalar_self=1, **FUSED_X)
BRICKS_PER_POWER_3D = counts(atom_bases=1, spread=1, rocfft_r2c=3, kspace=3, rocfft_c2r=3, gather_field=3, scalar_self=1)
DFT_BATCH_SPREAD_PER_POWER = counts(scalar_sites=3, spread=3, dft5=1, gather_field=1, scale_add=1)
DFT_ONE_SPREAD = counts(scalar_sites=1, spread=1, dft5=1, gather_field=1, scale_add=1)      # DftTyped, DftBatched (batched spread)
PER_POWER_PLANES = counts(scalar_sites=1, spread=1, dft_zy_fwd=1, dft_x_kspace=1, dft_yz_inv=1, gather_field=1, scale_add=1)
PER_POWER_3D = counts(scalar_sites=3, spread=3, rocfft_r2c=3, kspace=3, rocfft_c2r=3, gather_field=3, scale_add=3)

# case: (name, mesh or None for the handle's own, pmax, precision, c_list as a device tensor?, counts, wrong type table: None /
# 'refused' / 'ignored')
M64, M60, M313438, M9610045 = (64, 64, 64), (60, 60, 60), (31, 34, 38), (96, 100, 45)
CHILDREN = {
    'bricks': (dict(ADMP_SPREAD_BRICK_MIN='0'), [
        ('BricksTyped', M64, 10, 'single', True, BRICKS_TYPED, 'refused'),
        ('BricksBatched pmax 10', M64, 10, 'double', True, BRICKS_BATCHED, 'ignored'),
        ('BricksBatched pmax 8', M64, 8, 'double', False, BRICKS_BATCHED, None),
        ('BricksPerPower fused x', M64, 6, 'double', False, BRICKS_PER_POWER_FX, None),
        ('BricksPerPower rocFFT 3-D', M60, 10, 'double', False, BRICKS_PER_POWER_3D, None),
        ('DftBatched, a spread per power', None, 10, 'double', False, DFT_BATCH_SPREAD_PER_POWER, None),
    ]),
    'dft': (dict(ADMP_DFT='1'), [
        ('DftTyped double', M313438, 10, 'double', True, DFT_ONE_SPREAD, 'refused'),
        ('DftTyped single', M313438, 10, 'single', True, DFT_ONE_SPREAD, 'refused'),
        ('DftBatched double', M313438, 10, 'double', False, DFT_ONE_SPREAD, None),
        ('DftBatched single', M313438, 10, 'single', False, DFT_ONE_SPREAD, None),
        ('PerPower through convolve', M313438, 6, 'double', False, PER_POWER_PLANES, None),
    ]),
    'two_level': (dict(ADMP_DFT='2', ADMP_PFA_MIN='0'), [
        ('DftBatched two-level', M9610045, 10, 'double', False, DFT_ONE_SPREAD, None),
    ]),
    'rocfft': (dict(ADMP_DFT='0'), [
        ('PerPower rocFFT 3-D', M313438, 10, 'double', True, PER_POWER_3D, 'ignored'),
    ]),
}


@functools.lru_cache(maxsize=None)
def system():
    from tests.test_gpu_parity import water_system
    return water_system(216, 11, True)


def own_mesh():
    from admp_amd.pme import setup_ewald_parameters
    return tuple(int(k) for k in setup_ewald_parameters(RC, ETHRESH, system()[1])[1:])


@functools.lru_cache(maxsize=None)
def reference(mesh, pmax):
    """the oracle's (E, max|parts|, grad) of one (mesh, pmax): computed once, shared by every case and child that needs it"""
    from admp_amd.pme import setup_ewald_parameters
    from oracle import admp_oracle as O
    pos, box, at, ai, cov, par, pairs = system()
    kappa = setup_ewald_parameters(RC, ETHRESH, box)[0]
    r = O.disp_energy_and_grad(pos, box, pairs, par['c_list'], par['mScales'], cov, kappa, mesh, pmax)
    g = np.array(r['grad'])
    g.setflags(write=False)
    return float(r['E']), float(max(abs(p) for p in r['parts'])), g


def child_main(path):
    """runs in the child: every case of the file `path`, results back into it"""
    import torch
    from admp_amd import _lib, settings
    from admp_amd.disp_pme import ADMPDispPmeForce
    pos, box, at, ai, cov, par, pairs = system()
    job = json.load(open(path))
    refs = np.load(job['refs'])
    out = []
    for name, mesh, pmax, prec, tensor in job['cases']:
        settings.PRECISION = prec
        d = ADMPDispPmeForce(box, cov, RC, ETHRESH, pmax)
        if mesh:
            d.K1, d.K2, d.K3 = mesh
            d.refresh_calculators()
        mesh = (d.K1, d.K2, d.K3)
        cl = np.asarray(par['c_list'], dtype=np.float64)
        if tensor:
            cl = torch.as_tensor(cl, dtype=torch.float32 if prec == 'single' else torch.float64, device='cuda')
        g_ref = refs['%d_%d_%d_%d' % (mesh + (pmax,))]

        def call():
            E, G = d.get_forces(pos, box, pairs, cl, par['mScales'])
            G = np.asarray(G, dtype=np.float64)          # (positions are a numpy array: so is the gradient)
            return float(E), float(np.linalg.norm(G - g_ref) / np.linalg.norm(g_ref))
        call()                                   # warm: plans, tables, the type table of a tensor c_list
        d.profile(True)
        d.profile_reset()
        E, grel = call()
        rep = d.profile_report()
        d.profile(False)
        res = dict(name=name, mesh=mesh, E=E, grel=grel, counts={k: int(rep[k][1]) if k in rep else 0 for k in MESH_LABELS},
                   typed=getattr(d, '_types', None) is not None)
        if tensor and res['typed']:              # a table that does not describe c_list (tests/test_gpu_parity.py does the same)
            wrong = d._types[1].copy()
            wrong[0, 0] *= 1.5
            _lib.check(d._h, d._L.admp_disp_set_types(d._h, len(wrong), d._ptr(d._types[0]), _lib.darr(wrong)), 'set_types')
            try:
                res['wrong_E'], res['wrong_grel'] = call()
                res['wrong'] = 'ignored'
            except _lib.AdmpHipError as e:
                res['wrong'], res['wrong_text'] = 'refused', str(e)
        out.append(res)
    json.dump(out, open(path, 'w'))
    print('DISP-PATHS-OK')


@pytest.mark.parametrize('child', list(CHILDREN))
def test_path_of_every_case(tmp_path, child):
    env, cases = CHILDREN[child]
    own = own_mesh()
    assert own == (58, 58, 58)                   # 2 * 29: a direct-DFT mesh (tests/test_gpu_parity.py relies on it too)
    refs = {}
    for name, mesh, pmax, prec, tensor, want, wrong in cases:
        refs['%d_%d_%d_%d' % ((mesh or own) + (pmax,))] = reference(mesh or own, pmax)[2]
    np.savez(str(tmp_path / 'refs.npz'), **refs)
    path = str(tmp_path / 'job.json')
    json.dump(dict(refs=str(tmp_path / 'refs.npz'), cases=[c[:5] for c in cases]), open(path, 'w'))
    code = 'import sys; sys.path.insert(0, %r); from tests.test_gpu_disp_paths import child_main; child_main(%r)' % (ROOT, path)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
    assert r.returncode == 0 and 'DISP-PATHS-OK' in r.stdout, 'child exited %d\n' % r.returncode + r.stdout[-2000:] + r.stderr[-3000:]
    results = json.load(open(path))
    assert len(results) == len(cases)
    failures = []
    for (name, mesh, pmax, prec, tensor, want, wrong), res in zip(cases, results):
        E_ref, scale, _ = reference(mesh or own, pmax)
        tol = TOL[prec]
        print(child, name, res)
        if res['counts'] != want:
            failures.append((name, 'counts', {k: (res['counts'][k], want[k]) for k in want if res['counts'][k] != want[k]}))
        if not (abs(res['E'] - E_ref) < tol * scale and res['grel'] < max(tol, 1e-8)):
            failures.append((name, 'oracle', res['E'], E_ref, scale, res['grel']))
        if wrong is not None:
            if not res['typed'] or res.get('wrong') != wrong:
                failures.append((name, 'wrong type table', res.get('typed'), res.get('wrong'), res.get('wrong_text')))
            elif wrong == 'refused' and 'types' not in res['wrong_text']:
                failures.append((name, 'refusal text', res['wrong_text']))
            elif wrong == 'ignored' and not (abs(res['wrong_E'] - E_ref) < tol * scale and res['wrong_grel'] < max(tol, 1e-8)):
                failures.append((name, 'oracle after the wrong table', res['wrong_E'], E_ref, res['wrong_grel']))
    assert not failures, failures


# ---- refusals: host-side argument checks that return before any launch -------------------------------------------------------
STATE = 'topology, ewald parameters and pairs must be set first'
REFUSALS = {
    'disp before set_ewald': ('pairs', 'disp', {}, STATE),
    'disp pmax 7': ('ewald', 'disp', dict(pmax=7), 'pmax must be 6, 8 or 10'),
    'disp null E': ('ewald', 'disp', dict(E=None), 'null argument'),
    'disp null E and pmax 7': ('ewald', 'disp', dict(E=None, pmax=7), 'null argument'),      # the null check comes first
    'tt before pairs': ('top', 'tt', {}, 'topology and pairs must be set first'),
    'disp_box_grad null dbox': ('ewald', 'disp_box_grad', dict(dbox=None), 'null argument'),
    'mscale_grad kind 3': ('ewald', 'mscale_grad', dict(kind=3), 'kind must be 0 (multipolar PME), 1 (dispersion) or 2 (Tang-Toennies)'),
}


@pytest.fixture(scope='module')
def handles():
    """plain double-precision handles: 'top' with a topology, 'pairs' with a pair list too, 'ewald' with Ewald parameters too"""
    import torch
    from admp_amd import _lib, settings
    from admp_amd._device import HipForceBase
    pos, box, at, ai, cov, par, pairs = system()
    old = settings.PRECISION
    settings.PRECISION = 'double'
    try:
        hs = {k: HipForceBase(len(pos), cov) for k in ('top', 'pairs', 'ewald')}
    finally:
        settings.PRECISION = old
    for k in ('pairs', 'ewald'):
        hs[k].set_pairs(pairs)
    h = hs['ewald']
    _lib.check(h._h, h._L.admp_set_ewald(h._h, 0.7, 64, 64, 64, 0, 0), 'admp_set_ewald')
    dev = {k: torch.zeros((len(pos), n), dtype=torch.float64, device='cuda') for k, n in (('pos', 3), ('c', 3), ('abqc', 4), ('g', 3))}
    dev['pos'].copy_(torch.as_tensor(pos))
    return hs, dev, box


@pytest.mark.parametrize('case', list(REFUSALS))
def test_refusals_keep_their_code_and_text(handles, case):
    import ctypes
    from admp_amd import _lib
    hs, dev, box = handles
    which, entry, kw, text = REFUSALS[case]
    h = hs[which]
    L, p = h._L, h._ptr
    b, mS = _lib.darr(np.asarray(box).reshape(-1)), _lib.darr([0.0, 0.0, 0.0, 0.0, 1.0, 1.0])
    E, dbox, out = (ctypes.c_double * 3)(), (ctypes.c_double * 9)(), (ctypes.c_double * 6)()
    E = kw.get('E', E)
    pmax = kw.get('pmax', 10)
    if entry == 'disp':
        rc = L.admp_disp_energy_grad(h._h, p(dev['pos']), b, p(dev['c']), pmax, 6, mS, E, p(dev['g']), 1)
    elif entry == 'tt':
        rc = L.admp_tt_energy_grad(h._h, p(dev['pos']), b, p(dev['abqc']), 6, mS, E, p(dev['g']), 1)
    elif entry == 'disp_box_grad':
        rc = L.admp_disp_box_grad(h._h, p(dev['pos']), b, p(dev['c']), pmax, 6, mS, E, kw.get('dbox', dbox))
    else:
        rc = L.admp_mscale_grad(h._h, kw['kind'], p(dev['pos']), b, p(dev['c']), pmax, 6, out, 1)
    msg = L.admp_last_error(h._h).decode()
    print(case, rc, msg)
    assert rc == -1 and msg == text      # ADMP_E_ARG
