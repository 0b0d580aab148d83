"""The dipole observable on the GPU (ADMPPmeForce.get_dipoles, admp_amd.md.DipoleRecorder; admp_pme_dipoles = k_dipole_groups +
k_dipole_fold, dipole_kernels.hip) against the float64 restatement of tests/dipole_ref.py, on the values the device tensors
actually hold.  Both precisions throughout.

Bars (tests/dipole_ref.py): a double handle 64 eps_f64 sum |terms| per word and per mu_c; a single handle, where only the frames
and the minimum images are formed in single, 4 x 0.58 eps_f32 sum |terms|: the host program of dipole_math.h in float arithmetic
is at most 0.577 eps_f32 sum |terms| from the restatement on these cases (tests/test_dipole_cpu.py measures it: water64 0.237,
water64_tric 0.236, general 0.577, general_tric 0.509), recorded as 0.58, and the factor 4 covers a different contraction order
on the device.  -s prints err / bar per case."""
import ctypes
import functools
import re

import numpy as np
import pytest

from tests import dipole_ref as R
from tests.test_gpu_md_langevin import run_driver

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -5      # include/admp_hip.h


@pytest.fixture(params=['double', 'single'])
def prec(request):
    from admp_amd import settings
    old = settings.PRECISION
    settings.PRECISION = request.param
    try:
        yield request.param
    finally:
        settings.PRECISION = old


def bar_eps(pme):
    import torch
    return 64 * R.EPS64 if pme._dtype == torch.float64 else 4 * R.SINGLE_RATIO * R.EPS32


def make_pme(c, lpol=False, cov=None):
    """a calculator of the case's topology in the precision the fixture set (no covalent map unless given: the observable
    needs neither it nor pairs)"""
    import scipy.sparse as sp
    from admp_amd.pme import ADMPPmeForce
    n = c['n']
    cov = sp.csr_matrix((n, n), dtype=np.int32) if cov is None else cov
    return ADMPPmeForce(c['box'], c['axis_type'], c['axis_idx'], cov, 4.0, 1e-4, 2, lpol=lpol)


def dev(pme, a):
    import torch
    return torch.as_tensor(np.array(a), dtype=pme._dtype, device=pme._device).contiguous()


def host(t):
    return t.double().cpu().numpy()


def held_masses(pme, masses):
    """the masses the kernel sees: 1 / (what the handle holds of 1 / m)"""
    return 1.0 / host(pme._real(1.0 / np.asarray(masses, dtype=np.float64)))


def words_of(d):
    w = np.zeros(16)
    w[0:3], w[3:6], w[6:9] = d['M_charge'], d['M_permanent'], d['M_induced']
    ng = len(d['mu'])
    w[9], w[10], w[11], w[12] = d['mean_abs'] * ng, d['rms'] ** 2 * ng, d['max_abs'], ng
    return w


def check(pme, c, pos, Q, U, masses, label=''):
    """get_dipoles(per_group) under the bars of the restatement at the tensors' own values; returns the dict"""
    d = pme.get_dipoles(pos, c['box'], Q, c['labels'], masses, U=U, per_group=True)
    ref = R.reference(c, host(pos), host(Q), None if U is None else host(U), held_masses(pme, masses))
    assert d['mu'].shape == ref['mu'].shape
    # (mean_abs and rms are words 9 and 10 over the number of groups: scaled back, one more rounding each)
    x = R.excess(words_of(d), d['mu'], ref, bar_eps(pme))
    print('%s %s%s: err / bar %.3f' % (c['name'], pme._dtype, label, x))
    assert x <= 1.0
    assert words_of(d)[12] == ref['words'][12] == len(ref['groups'])
    assert np.array_equal(d['M'], d['M_charge'] + d['M_permanent'] + d['M_induced'])
    return d, ref


# ---- 1. every word and every mu_c -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.CASES)
def test_words_and_molecular_dipoles_against_the_restatement(prec, name):
    c = R.case(name)
    pme = make_pme(c)
    pos, Q, U = dev(pme, c['pos']), dev(pme, c['Q_local']), dev(pme, c['U'])
    d, _ = check(pme, c, pos, Q, U, c['masses'])
    d0, _ = check(pme, c, pos, Q, None, c['masses'], ' (no U)')
    assert (d0['M_induced'] == 0).all()                     # a non-polarizable handle without U: exactly zero
    assert np.array_equal(d0['M_charge'], d['M_charge']) and np.array_equal(d0['M_permanent'], d['M_permanent'])
    short = pme.get_dipoles(pos, c['box'], Q, c['labels'], c['masses'], U=U)
    assert 'mu' not in short and all(np.array_equal(short[k], d[k]) for k in short)


# ---- 2. invariances ---------------------------------------------------------------------------------------------------------
def within(a, b, ref_a, ref_b, eps_bar):
    """the largest difference of two results over the bar of the restatement (where the two have different terms, the larger)"""
    wt = np.maximum(ref_a['word_terms'], ref_b['word_terms'])[:12]
    mt = np.maximum(ref_a['mu_terms'], ref_b['mu_terms'])
    return max((np.abs(words_of(a) - words_of(b))[:12] / (eps_bar * wt)).max(), (np.abs(a['mu'] - b['mu']) / (eps_bar * mt)).max())


@pytest.mark.parametrize('name', ['water64_tric', 'general_tric'])
def test_invariances(prec, name):
    """positions and cell on a grid of 2^-10 A, so that an atom and its lattice images are all exact in either precision and
    the images tested are the same configuration to the last bit: what differs is the kernel's arithmetic alone"""
    c = R.case(name)
    grid = lambda a: np.round(np.asarray(a) * 1024.0) / 1024.0      # noqa: E731
    c = dict(c, pos=grid(c['pos']), box=grid(c['box']))
    pme = make_pme(c)
    box, eps_bar = c['box'], bar_eps(pme)
    pos, Q, U = dev(pme, c['pos']), dev(pme, c['Q_local']), dev(pme, c['U'])
    assert np.array_equal(host(pos), c['pos'])
    d, ref = check(pme, c, pos, Q, U, c['masses'])
    # a lattice vector added to every atom; every atom wrapped on its own into another cell than the case's
    cells = np.floor((c['pos'] - 0.5 * box.sum(axis=0)) @ np.linalg.inv(box))      # (whole numbers: the images stay on the grid)
    for label, moved in (('translated', c['pos'] + box[1] - box[2]), ('re-wrapped', c['pos'] - cells @ box)):
        assert np.abs(moved - c['pos']).max() > 1.0
        moved_d = dev(pme, moved)
        assert np.array_equal(host(moved_d), moved)
        d2, ref2 = check(pme, c, moved_d, Q, U, c['masses'], ' ' + label)
        x = within(d, d2, ref, ref2, eps_bar)
        print('%s against the case: %.3f of the bar' % (label, x))
        assert x <= 1.0
    # the induced part is the plain sum of U
    Uh = host(U)
    ext = np.asarray(Uh.astype(np.longdouble).sum(axis=0), dtype=np.float64)
    assert (np.abs(d['M_induced'] - ext) <= eps_bar * np.abs(Uh).sum(axis=0)).all()
    # the rows of per_group add up to M
    assert (np.abs(d['mu'].astype(np.longdouble).sum(axis=0).astype(np.float64) - d['M'])
            <= eps_bar * ref['word_terms'][0:9].reshape(3, 3).sum(axis=0)).all()
    # two identical calls: bit for bit
    again = pme.get_dipoles(pos, box, Q, c['labels'], c['masses'], U=U, per_group=True)
    assert all(np.array_equal(again[k], d[k]) for k in d)
    if name.startswith('water64'):      # neutral groups: other masses, the same mu_c
        other = np.random.default_rng(8).uniform(1.0, 30.0, size=c['n'])
        d3, ref3 = check(pme, c, pos, Q, U, other, ' other masses')
        x = within(d, d3, ref, ref3, eps_bar)
        print('other masses against the case: %.3f of the bar' % x)
        assert x <= 1.0
    else:                               # charged groups: the centre of mass is the origin, so the masses matter
        other = np.random.default_rng(8).uniform(1.0, 30.0, size=c['n'])
        d3, ref3 = check(pme, c, pos, Q, U, other, ' other masses')
        assert within(d, d3, ref, ref3, eps_bar) > 1.0


# ---- 3. U=None ---------------------------------------------------------------------------------------------------------------
def test_default_dipoles_are_those_of_the_last_evaluation(prec):
    from admp_amd import systems as S
    c = R.case('water64')
    n_mol = c['n'] // 3
    par = S.water_parameters(n_mol, polarizable=True)
    pol_pme = make_pme(c, lpol=True, cov=S.water_topology(n_mol)[2])
    pos, Q = dev(pol_pme, c['pos']), dev(pol_pme, c['Q_local'])
    args = (pos, c['box'], Q, c['labels'], c['masses'])
    with pytest.raises(RuntimeError, match='there has been none'):
        pol_pme.get_dipoles(*args)
    pairs = S.build_pairs(c['pos'], c['box'], 4.0)
    pol_pme.get_forces(pos, c['box'], pairs, Q, dev(pol_pme, par['pol']), dev(pol_pme, par['tholes']), par['mScales'], par['pScales'],
                       par['dScales'])
    import torch
    assert isinstance(pol_pme.U_ind, torch.Tensor) and float(pol_pme.U_ind.abs().max()) > 1e-3
    a = pol_pme.get_dipoles(*args, per_group=True)
    b = pol_pme.get_dipoles(*args, U=pol_pme.U_ind, per_group=True)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.abs(a['M_induced']).max() > 0
    ref = R.reference(c, host(pos), host(Q), host(pol_pme.U_ind), held_masses(pol_pme, c['masses']))
    assert R.excess(words_of(a), a['mu'], ref, bar_eps(pol_pme)) <= 1.0
    print('mean molecular dipole of the synthetic box %.4f D' % (a['mean_abs'] * 4.80320471))
    # a non-polarizable handle: exactly zero
    plain = make_pme(c)
    assert (plain.get_dipoles(dev(plain, c['pos']), c['box'], dev(plain, c['Q_local']), c['labels'], c['masses'])['M_induced'] == 0).all()


# ---- 4. the recorder ------------------------------------------------------------------------------------------------------------
def test_recorder_rows_are_get_dipoles_bit_for_bit(prec):
    from admp_amd.md import DipoleRecorder
    c = R.case('general_tric')
    pme = make_pme(c)
    Q, U = dev(pme, c['Q_local']), dev(pme, c['U'])
    rng = np.random.default_rng(21)
    frames = [dev(pme, c['pos'] + 0.02 * k * rng.normal(size=c['pos'].shape)) for k in range(5)]
    rec = DipoleRecorder(pme, c['labels'], c['masses'], 5)
    assert rec.rows().shape == (0, 16)
    for p in frames:
        rec.record(p, c['box'], Q, U)
    with pytest.raises(IndexError):
        rec.record(frames[0], c['box'], Q, U)
    rows = rec.rows()
    assert rows.shape == (5, 16) and rec.k == 5
    for p, w in zip(frames, rows):
        d = pme.get_dipoles(p, c['box'], Q, c['labels'], c['masses'], U=U, per_group=True)
        assert np.array_equal(w[:9], np.concatenate([d['M_charge'], d['M_permanent'], d['M_induced']])) and w[12] == len(d['mu'])
        assert d['mean_abs'] == w[9] / w[12] and d['rms'] == np.sqrt(w[10] / w[12]) and d['max_abs'] == w[11]
        assert (w[13:] == 0).all()
    assert len({tuple(w) for w in rows}) == 5
    rec.reset()
    assert rec.k == 0 and rec.rows().shape == (0, 16)
    rec.record(frames[3], c['box'], Q, U)
    assert np.array_equal(rec.rows()[0], rows[3])
    assert [s['max_abs'] for s in rec.summary()] == [rows[3][11]]


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(prec):
    import torch
    from admp_amd import _lib
    from admp_amd.md import DipoleRecorder, _DipoleInputs
    c = R.case('water64')
    pme = make_pme(c)
    L, h = pme._L, pme._h
    pos, Q, U = dev(pme, c['pos']), dev(pme, c['Q_local']), dev(pme, c['U'])
    inp = _DipoleInputs.of(pme, c['labels'], c['masses'])
    out = torch.full((16,), 7.0, dtype=torch.float64, device=pme._device)
    mu = torch.full((inp.n_groups, 3), 7.0, dtype=torch.float64, device=pme._device)
    box = _lib.darr(c['box'])
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    good = [P(pos), box, P(Q), P(U), P(inp.inv_mass), inp.n_groups, P(inp.start), P(inp.atoms), P(mu), P(out)]
    pme._use_current_stream()
    for k in (0, 1, 2, 4, 6, 7, 9):                         # every required pointer
        a = list(good)
        a[k] = None
        assert L.admp_pme_dipoles(h, *a) == E_ARG, k
        assert b'null' in L.admp_last_error(h)
    a = list(good)
    a[5] = -1
    assert L.admp_pme_dipoles(h, *a) == E_ARG
    for bad in (np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]]), np.zeros((3, 3)), c['box'] + np.diag([0.0, np.nan, 0.0]),
                c['box'] + np.diag([0.0, np.inf, 0.0])):
        a = list(good)
        a[1] = _lib.darr(bad)
        assert L.admp_pme_dipoles(h, *a) == E_ARG, bad
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (mu == 7.0).all()        # nothing was written
    # a handle without a topology
    bare = ctypes.c_void_p()
    assert L.admp_create(ctypes.byref(bare), pme._dev_index, pme._nbytes) == 0
    try:
        assert L.admp_pme_dipoles(bare, *good) == E_STATE
        assert b'admp_set_topology' in L.admp_last_error(bare)
    finally:
        L.admp_destroy(bare)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (mu == 7.0).all()
    # no groups: nothing launched, the words zeroed; U and mu may be NULL
    a = list(good)
    a[5], a[3], a[8] = 0, None, None
    assert L.admp_pme_dipoles(h, *a) == 0
    torch.cuda.synchronize()
    assert (out == 0.0).all() and (mu == 7.0).all()
    assert L.admp_pme_dipoles(h, *good) == 0               # and the good call is good
    torch.cuda.synchronize()
    assert float(out[12]) == inp.n_groups and float(out[11]) > 0
    # Python: the library reads raw pointers
    other = torch.float32 if pme._dtype == torch.float64 else torch.float64
    args = dict(positions=pos, box=c['box'], Q_local=Q, groups=c['labels'], masses=c['masses'], U=U)
    for key, bad in (('positions', pos.to(other)), ('positions', pos[:-1]), ('positions', pos.cpu()),
                     ('positions', torch.stack([pos, pos], dim=1)[:, 0]), ('positions', host(pos)), ('Q_local', Q[:, :4].contiguous()),
                     ('Q_local', Q.to(other)), ('U', U.cpu()), ('U', U.to(other)), ('U', U.reshape(3, -1)),
                     ('groups', c['labels'][:-1]), ('masses', c['masses'][:-1]), ('masses', -c['masses']),
                     ('groups', c['labels'].astype(np.float64))):
        with pytest.raises(ValueError):
            pme.get_dipoles(**dict(args, **{key: bad}))
    rec = DipoleRecorder(pme, c['labels'], c['masses'], 2)
    with pytest.raises(ValueError):
        rec.record(pos.to(other), c['box'], Q, U)
    with pytest.raises(ValueError):
        rec.record(pos, np.zeros((3, 3)), Q, U)            # the library's refusal of the box
    assert rec.k == 0
    with pytest.raises(ValueError):
        DipoleRecorder(pme, c['labels'], c['masses'], -1)


# ---- 6. a driver end to end -----------------------------------------------------------------------------------------------------
def test_nvt_driver_reports_the_dipoles():
    """64 polarizable waters, 20 steps, a record every 5: the line is there, and the mean molecular dipole lies between the
    gas-phase 1.85 D and 4 D"""
    out = run_driver('nvt_water.py', '--waters', '64', '--steps', '20', '--pol', '--dipoles', '5')
    m = re.search(r'# dipoles over (\d+) records: mean molecular dipole ([-+0-9.e]+) D \(permanent share ([-+0-9.e]+) D, '
                  r'induced share ([-+0-9.e]+) D\); dielectric constant ([-+0-9.e]+) at', out)
    assert m, out[-1500:]
    print(m.group(0))
    n, mean, static, induced = int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4))
    assert n == 4
    assert np.isfinite(mean) and 1.85 < mean < 4.0
    assert np.isfinite(induced) and induced > 0 and abs(mean - static - induced) < 2e-4
    assert np.isfinite(float(m.group(5)))
    assert 'do not converge the dielectric constant' in out
