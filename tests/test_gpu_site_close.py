"""The first and the last stage of an evaluation, atom by atom against the float64 reference of tests/site_ref.py: the site table
(k_prepare_sites: frames under every axis rule, local -> global rotation, charge-only mark, list of polarizable sites, the
next evaluation's energy words) and the closing kernels k_finish_pull<4>, k_finish_pull<1>, k_finish_groups, k_finish_rows
(atom_kernels.hip), the closing epilogue of k_gather_staged<.., FIN> (recip_kernels.hip) and k_frame_virial -- each alone,
through the C entries admp_site_table / admp_site_close (what an evaluation does up to that kernel, through the evaluation's own
launchers).  Cases, reference, floors and the launch forms to expect are proved sound without a GPU in
tests/test_site_ref_cpu.py.

ADMP_FINISH4_MAX and ADMP_FINISH_GROUPS are read once per process, so every setting gets a child process:

    default   nothing set: pull = k_finish_pull<4>; the site table, the frame virial and the refusals run here
    pull1     ADMP_FINISH4_MAX=0: pull = k_finish_pull<1>
    nogroups  ADMP_FINISH_GROUPS=0: no topology has frame groups: every switch ends in the pull form, which = 1 is refused

Inside a child the per-call switches pick the form: rows (ADMP_FINISH_GROUPS_MIN=0), rows with ADMP_FINISH_ROWS_GRID=2 and =1
(one workgroup walks 2 and 3 runs of the 760-atom case), groups (ADMP_FINISH_ROWS=0), pull (ADMP_FINISH_GROUPS_MIN above the
atom count), and the gather's epilogue (which = 1, on phi = 0 -- the reciprocal part is then exactly zero -- and once on white
noise, where the reference is mesh_ref.GatherRef + the closing work on pot_in + pot_recip and the bars add).  Every case runs in
both types with one handle per case and type; every form is called twice.

Checks per case, type and form: info names the form meant and the run counts of site_ref.expected_info.  Double: grad, dQ_local
and Q_global within rtol 1e-9 + atol 1e-8 (grad) / 1e-9 (Q_global, dQ_local) x max|ref|, energies within 1e-10 max(1, |E|)
(pair_ref.double_bars), forms equal to 1e-12 of the largest entry.  Single: max|X - ref| / max|ref| <= pair_ref.FLOOR_FACTOR (8)
x the host floor of the case and output (site_ref.floors), energies within 8 x their floor.  Exact: a charge-only axis-free
site returns dQ_local[1:] = pot_in[1:] bit for bit, an axis-free site that is nobody's axis atom gets a zero gradient row; the
second call of a form equals the first bit for bit; a case with far atoms in the unused index slots equals the case with -1
there bit for bit, form by form, and still takes the group forms; the list of polarizable sites is a permutation of
where(pol > 0), ascending inside each block of 256 atoms, n_act exact; the charge-only mark is pair_ref.mono_mask; the energy
words of a call's half read zero two calls after a closing call wrote them; the virial is exactly zero where no group lies
across a face, and within 8 x floor (single) / 1e-9 of its largest entry (double) elsewhere.

Every child prints err / bar per case and form (run with -s).  Measured on an MI355X, largest err / bar (f64, f32), the same
for k_finish_pull<4>, k_finish_pull<1>, k_finish_groups, k_finish_rows (grids 3, 2 and 1) and the gather's epilogue: grad 1.8e-4,
0.177; dQ_local 3.5e-6, 0.134; E_self 2.2e-5, 0.125; E_pen 3.1e-6, 0.125 (rows, groups, epilogue: 0.073); site table Q_global
2.0e-4, 0.155; frame virial 7.1e-4, 0.172.  A float32 ratio of 0.125 = 1 / FLOOR_FACTOR says that the device's error IS the host
floor: the same frame_math.h gives the same bits on both.  The test found no kernel wrong.  A child takes 5.5 to 6 s, 2.2 s of it
imports; the module 22 s."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import site_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [('default', {}), ('pull1', {'ADMP_FINISH4_MAX': '0'}), ('nogroups', {'ADMP_FINISH_GROUPS': '0'})]
# form -> (ADMP_FINISH_GROUPS_MIN, ADMP_FINISH_ROWS, ADMP_FINISH_ROWS_GRID or None, which)
FORMS = {'rows': ('0', '1', None, 0), 'rows_grid2': ('0', '1', '2', 0), 'rows_grid1': ('0', '1', '1', 0),
         'groups': ('0', '0', None, 0), 'pull': ('100000000', '1', None, 0), 'gather': ('100000000', '1', None, 1)}
CHILD_FORMS = {'default': tuple(FORMS), 'pull1': ('pull', 'rows'), 'nogroups': ('rows', 'groups', 'pull', 'gather')}

CHILD = r'''
import ctypes, json, os, pickle, sys, time
t_start = time.time()
sys.path.insert(0, %r)
import numpy as np
import torch
from admp_amd import settings, _lib
from admp_amd.pme import ADMPPmeForce
from tests import site_ref as S
from tests.mesh_ref import EmptyCov

data = pickle.load(open(sys.argv[1], 'rb'))
tag = sys.argv[3]
FORMS, forms = data['FORMS'], data['CHILD_FORMS'][tag]
out = {'calls': [], 'refusals': 0, 'secs': [time.time() - t_start]}
NP = lambda t: None if t is None else t.cpu().numpy().astype(np.float64)      # noqa: E731
RT = {'single': np.float32, 'double': np.float64}


def force(c, lpol=True):
    f = ADMPPmeForce(c['box'], c['axis_type'], c['axis_indices'], EmptyCov(c['n']), 4.0, 1e-4, 2, lpol=lpol)
    f.kappa = c['kappa']
    f.K1, f.K2, f.K3 = c['K']
    f.refresh_calculators()
    return f


def switches(form):
    gmin, rows, grid, which = FORMS[form]
    os.environ['ADMP_FINISH_GROUPS_MIN'] = gmin
    os.environ['ADMP_FINISH_ROWS'] = rows
    os.environ.pop('ADMP_FINISH_ROWS_GRID', None)
    if grid is not None:
        os.environ['ADMP_FINISH_ROWS_GRID'] = grid
    return which


def excess(got, ref, atol_factor):
    return S.double_excess(got, ref, None, atol_factor)


kept = {}
for name in data['names']:
    c = data['cases'][name]
    free = c['axis_type'] == S.NOAXIS
    used = np.zeros(c['n'], dtype=bool)       # atoms that are somebody's axis atom
    use = S.used_slots(c['axis_type'])
    for k in range(3):
        used[c['axis_indices'][use[:, k], k]] = True
    for prec in ('double', 'single'):
        settings.PRECISION = prec
        t_case = time.time()
        ref = data['refs'][name][prec]
        f = force(c)
        kw = dict(pol=c['pol'], tholes=c['thole'], U=c['U'])
        rec = dict(name=name, prec=prec, forms={})
        pot_t = np.asarray(c['pot_in'], dtype=RT[prec])
        phi = c['phi'] if c['phi'] is not None else np.zeros(c['K'])
        for form in forms:
            if c['phi'] is not None and form != 'gather':      # (the white-noise case is about the gather's epilogue alone)
                continue
            which = switches(form)
            q = dict()
            try:
                calls = [f.site_close(c['pos'], c['box'], c['pairs'], c['Q_local'], c['pot_in'], phi=phi if which == 1 else None,
                                      which=which, **kw) for _ in range(2)]
            except _lib.AdmpHipError as e:
                rec['forms'][form] = dict(refused=str(e))
                continue
            r = calls[0]
            grad, dQ = NP(r['grad']), NP(r['dQ'])
            q['info'] = {k: r[k] for k in ('form', 'ngroups', 'nrowblk', 'rows_grid', 'ngathblk') if k in r}
            # (the arrays: no atomics there; the workgroups' energy sums are added by atomics, in arrival order)
            q['repeat_same'] = bool(np.array_equal(grad, NP(calls[1]['grad'])) and np.array_equal(dQ, NP(calls[1]['dQ'])))
            q['finite'] = bool(np.isfinite(grad).all() and np.isfinite(dQ).all())
            mono_free = free & c['mono']
            q['free_dQ_exact'] = bool(np.array_equal(dQ[mono_free, 1:], pot_t[mono_free, 1:].astype(np.float64))) if c['phi'] is None else True
            q['free_grad_zero'] = bool(not grad[free & ~used].any()) if c['phi'] is None else True
            if prec == 'double':
                if c['phi'] is None:
                    q['grad'], q['dQ'] = excess(grad, ref['grad'], 1e-8), excess(dQ, ref['dQ'], 1e-9)
                else:      # the bars add: the gather's own (per word) and the closing kernel's
                    tol_g = ref['bar_grad_gather'] + 1e-8 * np.abs(ref['grad']).max() + 1e-9 * np.abs(ref['grad'])
                    tol_q = ref['bar_pot_gather'].sum(1, keepdims=True) + 1e-9 * np.abs(ref['dQ']).max() + 1e-9 * np.abs(ref['dQ'])
                    q['grad'], q['dQ'] = float((np.abs(grad - ref['grad']) / tol_g).max()), float((np.abs(dQ - ref['dQ']) / tol_q).max())
                q['E_self'] = abs(r['E_self'] - ref['E_self']) / (1e-10 * max(1.0, abs(ref['E_self'])))
                q['E_pen'] = abs(r['E_pen'] - ref['E_pen']) / (1e-10 * max(1.0, abs(ref['E_pen'])))
            else:
                b = ref['bars']
                if c['phi'] is None:
                    eg, eq = S.rel_err(grad, ref['grad']), S.rel_err(dQ, ref['dQ'])
                    q['grad'] = eg / b['grad'] if b['grad'] > 0 else (0.0 if eg == 0 else float('inf'))
                    q['dQ'] = eq / b['dQ']
                else:
                    tol_g = ref['bar_grad_gather'] + b['grad'] * np.abs(ref['grad_frames']).max()
                    tol_q = ref['bar_pot_gather'].sum(1, keepdims=True) + b['dQ'] * np.abs(ref['dQ']).max()
                    q['grad'], q['dQ'] = float((np.abs(grad - ref['grad']) / tol_g).max()), float((np.abs(dQ - ref['dQ']) / tol_q).max())
                q['E_self'] = abs(r['E_self'] - ref['E_self']) / b['E_self']
                q['E_pen'] = abs(r['E_pen'] - ref['E_pen']) / b['E_pen'] if b['E_pen'] > 0 else (0.0 if r['E_pen'] == ref['E_pen'] else float('inf'))
            kept[(name, prec, form)] = (grad, dQ, r['E_self'], r['E_pen'])
            rec['forms'][form] = q
        # the forms among themselves (double), relative to the largest entry
        if prec == 'double':
            have = [fm for fm in forms if (name, prec, fm) in kept]
            worst = 0.0
            for fm in have[1:]:
                for k in (0, 1):
                    a, b0 = kept[(name, prec, have[0])][k], kept[(name, prec, fm)][k]
                    scale = np.abs(a).max()
                    worst = max(worst, float(np.abs(a - b0).max() / scale) if scale > 0 else float(np.abs(a - b0).max()))
            rec['forms_agree'] = worst
        base = data['UNUSED_OF'].get(name)
        if base is not None:
            rec['unused_same'] = {fm: bool(all(np.array_equal(x, y) for x, y in zip(kept[(name, prec, fm)][:2], kept[(base, prec, fm)][:2])))
                                  for fm in forms if (name, prec, fm) in kept and (base, prec, fm) in kept}
        if tag == 'default' and c['phi'] is not None:
            rec['vir'] = rec['table'] = None
        elif tag == 'default':
            # ---- frame virial
            switches('pull')
            v = f.site_close(c['pos'], c['box'], c['pairs'], c['Q_local'], c['pot_in'], which=2, **kw)['vir']
            scale = np.abs(ref['vir']).max()
            e = float(np.abs(v - ref['vir']).max())
            if scale == 0.0:
                rec['vir'] = dict(exact_zero=bool(not v.any()), ratio=0.0 if not v.any() else float('inf'))
            else:
                bar = 1e-9 if prec == 'double' else ref['bars']['vir']
                rec['vir'] = dict(exact_zero=False, ratio=e / scale / bar)
            # ---- site table: two calls after a closing call, so that the second reads the half that call wrote
            tabs = [f.site_table(c['pos'], c['box'], c['pairs'], c['Q_local'], **kw) for _ in range(2)]
            t = tabs[1]
            rows = NP(t['sites'])
            x = {k: np.asarray(c[k], dtype=RT[prec]).astype(np.float64) for k in ('pos', 'U', 'thole', 'pol')}
            tr = ref['table']
            p6 = np.asarray(np.asarray(c['pol'], dtype=RT[prec]).astype(np.float64) ** (1.0 / 6.0), dtype=RT[prec]).astype(np.float64)
            act = NP(t['act']).astype(np.int64)
            blocks_ok = sorted(act.tolist()) == tr['act'].tolist() and t['n_act'] == len(tr['act'])
            for b0 in range(0, c['n'], 256):       # a workgroup's sites stay together and in order
                mine = act[(act >= b0) & (act < b0 + 256)]
                where = np.nonzero((act >= b0) & (act < b0 + 256))[0]
                blocks_ok = blocks_ok and bool((np.diff(mine) > 0).all()) and (len(where) == 0 or where[-1] - where[0] + 1 == len(where))
            if prec == 'double':
                qg = excess(rows[:, 3:12], tr['Q'], 1e-9)
            else:
                qg = S.rel_err(rows[:, 3:12], tr['Q']) / ref['bars']['Qg']
            rec['table'] = dict(
                Qg=qg, r_exact=bool(np.array_equal(rows[:, 0:3], x['pos'])), U_exact=bool(np.array_equal(rows[:, 12:15], x['U'][:, [2, 0, 1]])),
                p6=float(np.abs(rows[:, 15] - p6).max() / (2.0 ** (-52 if prec == 'double' else -23))),
                thole_exact=bool(np.array_equal(rows[:, 16], x['thole'])), mono_ok=bool(np.array_equal(rows[:, 17] == 1.0, tr['mono'])),
                pad_ok=bool(not rows[:, 18:20].any() and set(np.unique(rows[:, 17])) <= {0.0, 1.0}), list_ok=bool(blocks_ok),
                n_act=t['n_act'], records=t['records'], dirty=[tabs[0]['dirty_energy_words'], tabs[1]['dirty_energy_words']],
                same=bool(np.array_equal(rows, NP(tabs[0]['sites']))))
        del f
        rec['secs'] = time.time() - t_case
        out['calls'].append(rec)

out['secs'].append(time.time() - t_start)
# ---- refusals: each before a kernel is launched, and the handle serves a valid call afterwards
if tag == 'default':
    settings.PRECISION = 'double'
    c = data['cases']['rules_ortho']
    switches('rows')
    L = _lib.load()
    f, g = force(c), force(c, lpol=False)
    n = c['n']
    P = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()      # noqa: E731
    pos, Q, pol, th, U, pot = P(c['pos']), P(c['Q_local']), P(c['pol']), P(c['thole']), P(c['U']), P(c['pot_in'])
    phi, grad, dQ, sites = P(np.zeros(c['K'])), P(np.zeros((n, 3))), P(np.zeros((n, 9))), P(np.zeros((n, 20)))
    act = torch.zeros(n, dtype=torch.int32).cuda()
    E2, V9, i4 = (ctypes.c_double * 2)(), (ctypes.c_double * 9)(), (ctypes.c_int * 4)()
    box = _lib.darr(c['box'])
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def close(h, which=0, pos=pos, Q=Q, pol=pol, th=th, U=U, pot=pot, phi=phi, want_dQ=1, E=E2, grad=grad, dQ=dQ, vir=V9, info=i4):
        return L.admp_site_close(h._h, p(pos), box, p(Q), p(pol), p(th), p(U), p(pot), p(phi), which, want_dQ, 1, E, p(grad), p(dQ),
                                 vir, info)

    def table(h, pos=pos, Q=Q, pol=pol, th=th, U=U, sites=sites, act=act, info=i4):
        return L.admp_site_table(h._h, p(pos), box, p(Q), p(pol), p(th), p(U), 1, p(sites), p(act), info)
    err = lambda h: L.admp_last_error(h._h)      # noqa: E731
    assert close(f) != 0 and b'pairs must be set' in err(f)                     # no pairs set
    assert table(f) != 0 and b'pairs must be set' in err(f)
    f.set_pairs(c['pairs'])
    g.set_pairs(c['pairs'])
    assert close(f) == 0 and close(f, 1) == 0 and close(f, 2) == 0 and table(f) == 0
    for kw in (dict(pos=None), dict(Q=None), dict(pot=None), dict(info=None), dict(E=None), dict(grad=None), dict(dQ=None),
               dict(pol=None), dict(th=None), dict(U=None)):
        assert close(f, **kw) != 0, kw
        assert close(f, 1, **kw) != 0, kw
    assert close(f, dQ=None, want_dQ=0) == 0
    assert close(f, 2, vir=None) != 0 and close(f, 2, E=None, grad=None, dQ=None) == 0
    assert close(f, 1, phi=None) != 0 and b'phi_in' in err(f)
    assert close(f, 3) != 0 and b'which' in err(f) and close(f, -1) != 0 and b'which' in err(f)
    for kw in (dict(pos=None), dict(Q=None), dict(sites=None), dict(info=None), dict(act=None), dict(pol=None), dict(th=None), dict(U=None)):
        assert table(f, **kw) != 0, kw
    assert close(g, pol=None, th=None, U=None) == 0 and table(g, pol=None, th=None, U=None, act=None) == 0 and i4[0] == 0
    os.environ['ADMP_FUSE_FIN_MAX'] = '0'                                        # an evaluation would not close in the gather
    assert close(f, 1) != 0 and b'do not close in the gather' in err(f)
    del os.environ['ADMP_FUSE_FIN_MAX']
    assert close(f) == 0 and i4[0] == 3 and close(f, 1) == 0 and i4[0] == 4 and table(f) == 0      # still serving
    _lib.check(f._h, L.admp_slab_configure(f._h, 0, 2), 'admp_slab_configure')
    assert close(f) != 0 and b'single rank' in err(f)                            # slab handle
    assert table(f) != 0 and b'single rank' in err(f)
    out['refusals'] = 1

out['secs'].append(time.time() - t_start)
json.dump(out, open(sys.argv[2], 'w'))
print('child ok')
''' % ROOT


def _plain(c):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in c.items() if k != 'cond'}


@pytest.fixture(scope='module')
def shared(tmp_path_factory):
    """cases, references and bars of tests/site_ref.py, computed once and written to one file"""
    d = tmp_path_factory.mktemp('site_close')
    data = dict(names=list(S.CASES), cases={}, refs={}, FORMS=FORMS, CHILD_FORMS=CHILD_FORMS, UNUSED_OF=S.UNUSED_OF)
    for name in S.CASES:
        c = S.case(name)
        data['cases'][name] = _plain(c)
        tab = S.site_table_ref(c)
        data['refs'][name] = {}
        for prec in ('double', 'single'):
            r = S.reference(name, prec)
            ref = dict(grad=r['grad'], dQ=r['dQ'], E_self=r['E_self'], E_pen=r['E_pen'], vir=r['vir'],
                       table=dict(Q=tab['Q'], mono=tab['mono'], act=tab['act']), bars=S.single_bars(name))
            if c['phi'] is not None:
                ref.update(grad_frames=r['grad_frames'], bar_grad_gather=r['gather']['bars']['grad'],
                           bar_pot_gather=r['gather']['bars']['pot'])
            data['refs'][name][prec] = ref
    path = d / 'refs.pkl'
    with open(path, 'wb') as fh:
        pickle.dump(data, fh)
    script = d / 'child.py'
    script.write_text(CHILD)
    return dict(dir=d, refs=str(path), script=str(script), data=data, dead=[], results={})


ABNORMAL = (124, 137, 134, 139, -6, -9, -11)


def run_child(shared, tag):
    """the child of one setting, started once; its results serve every test of the module"""
    if tag in shared['results']:
        return shared['results'][tag]
    if shared['dead']:
        pytest.fail('not started: the child %s ended abnormally (%s)' % tuple(shared['dead'][0]))
    out = shared['dir'] / ('%s.json' % tag)
    r = subprocess.run(['timeout', '-k', '10', '150', sys.executable, shared['script'], shared['refs'], str(out), tag],
                       env=dict(os.environ, **dict(SETTINGS)[tag]), capture_output=True, text=True, cwd=ROOT)
    if r.returncode in ABNORMAL or r.returncode < 0:
        shared['dead'].append((tag, r.returncode))
    assert r.returncode == 0 and 'child ok' in r.stdout, (tag, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    shared['results'][tag] = json.load(open(out))
    return shared['results'][tag]


def expected(tag, c, form):
    asked = {'rows_grid2': 'rows', 'rows_grid1': 'rows'}.get(form, form)
    grid = {'rows_grid2': 2, 'rows_grid1': 1}.get(form, 1024)
    return S.expected_info(c, asked, groups_on=tag != 'nogroups', lanes4=tag != 'pull1', rows_grid=grid)


@pytest.mark.parametrize('tag,env', SETTINGS, ids=[s[0] for s in SETTINGS])
def test_closing_kernels_atom_by_atom(shared, tag, env):
    res = run_child(shared, tag)
    assert res['refusals'] == int(tag == 'default')
    worst, over, seen, kernels = {}, [], set(), set()
    for q in res['calls']:
        c = S.case(q['name'])
        seen.add((q['name'], q['prec']))
        line = []
        for form in CHILD_FORMS[tag]:
            if c['phi'] is not None and form != 'gather':
                continue
            what = (tag, q['name'], q['prec'], form)
            want = expected(tag, c, form)
            got = q['forms'][form]
            if want is None:
                assert 'refused' in got and 'do not close in the gather' in got['refused'], (what, got)
                continue
            assert 'refused' not in got, (what, got)
            assert got['info'] == want, (what, got['info'], want)
            assert got['finite'] and got['repeat_same'] and got['free_dQ_exact'] and got['free_grad_zero'], (what, got)
            kernels.add((want['form'], q['prec']))
            for k in ('grad', 'dQ', 'E_self', 'E_pen'):
                key = (want['form'], q['prec'], k)
                worst[key] = max(worst.get(key, 0.0), got[k])
                if not got[k] <= 1.0:
                    over.append((what, k, got[k]))
            line.append('%s %.3f %.3f %.3f %.3f' % (form, got['grad'], got['dQ'], got['E_self'], got['E_pen']))
        if q['prec'] == 'double':
            assert q['forms_agree'] <= 1e-12, (tag, q['name'], q['forms_agree'])
        if q['name'] in S.UNUSED_OF:
            assert q['unused_same'] and all(q['unused_same'].values()), (tag, q['name'], q['prec'], q['unused_same'])
        print('RATIO %-8s %-18s %-6s err / bar (grad dQ E_self E_pen): %s | %.2f s' % (tag, q['name'], q['prec'], '; '.join(line), q['secs']))
    assert seen == {(n_, p_) for n_ in S.CASES for p_ in ('double', 'single')}
    need = {'default': ('pull4', 'groups', 'rows', 'gather_epilogue'), 'pull1': ('pull1', 'rows'), 'nogroups': ('pull4',)}[tag]
    assert {(k, p_) for k in need for p_ in ('double', 'single')} == kernels, (tag, kernels)
    for key in sorted(worst):
        print('WORST %-8s %-16s %-6s %-6s err / bar %.3g' % ((tag,) + key + (worst[key],)))
    print('SECS  %-8s child: imports %.1f, cases %.1f, refusals %.1f (cumulative)' % ((tag,) + tuple(res['secs'])))
    assert not over, (tag, over)


def test_grid_stride_loop_of_the_rows_form(shared):
    """ADMP_FINISH_ROWS_GRID = 2 and 1 on the 760-atom case: 3 runs on 2 and on 1 workgroup, the numbers of the 3-workgroup
    launch to 1e-12 (double; the energy sums are added in another order) -- and the info says the loop was entered"""
    res = run_child(shared, 'default')
    for q in res['calls']:
        if q['name'] == S.GRID_CASE:
            assert [q['forms'][f]['info']['rows_grid'] for f in ('rows', 'rows_grid2', 'rows_grid1')] == [3, 2, 1]
            assert q['forms']['rows']['info']['nrowblk'] == 3


def test_site_table_row_by_row(shared):
    res = run_child(shared, 'default')
    worst = {}
    for q in res['calls']:
        if q['table'] is None:
            continue
        c, t = S.case(q['name']), q['table']
        what = (q['name'], q['prec'])
        assert t['r_exact'] and t['U_exact'] and t['thole_exact'] and t['mono_ok'] and t['pad_ok'] and t['same'], (what, t)
        assert t['list_ok'] and t['n_act'] == int((c['pol'] > 0).sum()) and t['records'] == 1, (what, t)
        assert t['dirty'] == [0, 0], (what, t)          # also below E_WORDS atoms (n1, n4, n31 .. n33, the rules cases)
        assert t['p6'] <= 1.0, (what, t['p6'])          # pol^(1/6) within one unit in the last place of a number below 2
        worst[q['prec']] = max(worst.get(q['prec'], 0.0), t['Qg'])
        print('TABLE %-18s %-6s Q_global err / bar %.3f, p6 %.2f ulp, n_act %d' % (q['name'], q['prec'], t['Qg'], t['p6'], t['n_act']))
        assert t['Qg'] <= 1.0, (what, t['Qg'])
    print('WORST table Q_global err / bar: %s' % worst)


def test_frame_virial(shared):
    res = run_child(shared, 'default')
    worst = {}
    for q in res['calls']:
        c = S.case(q['name'])
        v = q['vir']
        if v is None:
            continue
        if not S.straddling(c).any():
            assert v['exact_zero'], (q['name'], q['prec'], v)
        worst[q['prec']] = max(worst.get(q['prec'], 0.0), v['ratio'])
        print('VIRIAL %-18s %-6s err / bar %.3f' % (q['name'], q['prec'], v['ratio']))
        assert v['ratio'] <= 1.0, (q['name'], q['prec'], v)
    assert any(not S.straddling(S.case(n)).any() for n in S.CASES)
    print('WORST virial err / bar: %s' % worst)
