"""The inputs and the reference of tests/test_gpu_pair_kernels.py, proved sound without a GPU: the cases of tests/pair_ref.py
satisfy their own conditions, the host shim of the kernels' per-pair functions reproduces the float64 oracle on every one of
them, the single-precision floors exist, and a reference that is wrong the way a kernel can be wrong (a pair lost, a pair in
another class, a row's last partner lost, erfc off by 1e-6) lies outside the bars the GPU test applies."""
import numpy as np
import pytest

from tests import pair_ref as R


@pytest.mark.parametrize('name', R.CASES)
def test_cases_satisfy_their_conditions(name):
    c = R.case(name)
    n, pairs = c['n'], c['pairs']
    assert pairs.dtype == np.int32 and pairs.ndim == 2 and pairs.shape[1] == 2 and len(pairs) > 0
    assert (pairs[:, 0] < pairs[:, 1]).all() and pairs.min() >= 0 and pairs.max() < n
    assert c['cov'].min() >= 0 and c['cov'].max() <= 5 and (c['cov'] == c['cov'].T).all()
    assert c['cov'][pairs[:, 0], pairs[:, 1]].max() >= 1
    # the site classes are what the builder meant them to be, and variant B has no charge-only site left
    assert (c['U'][c['pol'] == 0] == 0).all()
    assert not R.mono_mask(c['Q_local_B'], c['pol'], c['U']).any() or not c['mono'].any()
    r = R.distances(c['pos'], c['box'], pairs)
    assert r.min() > 0.65
    if name != 'rows67':      # (its list is made by hand: any partner, at whatever minimum-image distance)
        assert r.max() < 0.5 * min(np.linalg.norm(c['box'], axis=1)) * 0.999
    if n == 577:
        assert [-(-n * lanes // 256) for lanes in (1, 2, 4, 8, 16, 32)] == [3, 5, 10, 19, 37, 73]
        assert len(c['isolated']) == 1
        frac = c['pos'] @ np.linalg.inv(c['box'])
        assert ((frac < 0) | (frac >= 1)).any(axis=1).sum() > 10          # atoms outside the cell
        lens = np.bincount(R.listed_pairs(c).reshape(-1), minlength=n)
        assert lens.max() > R.LROW and np.median(lens) > 30
    if n == 2309:
        lens = np.bincount(pairs.reshape(-1), minlength=n)
        assert -(-n // 256) == 10 and lens.max() < 20
    if c['cutoff']:
        assert np.abs(r - c['cutoff']).min() > 1e-5
        assert 0.5 * len(pairs) < len(R.listed_pairs(c)) < 0.8 * len(pairs)
    if name == 'rows67':
        mono = c['mono']
        for s, (nf, nm) in enumerate(R.ROW_SHAPES):
            for i in (2 * s, 2 * s + 1):
                partners = np.concatenate([pairs[pairs[:, 0] == i, 1], pairs[pairs[:, 1] == i, 0]])
                assert (int((~mono[partners]).sum()), int(mono[partners].sum())) == (nf, nm), (i, nf, nm)
            assert not mono[2 * s] and mono[2 * s + 1]
        L = R.LROW
        totals = {nf + nm for nf, nm in R.ROW_SHAPES}
        assert totals == {0, 1, L - 1, L, L + 1, 2 * L + 1, 3 * L}
        for t in totals - {0, 1}:       # each total: full-moment partners only, charge-only partners only, both
            kinds = {(nf > 0, nm > 0) for nf, nm in R.ROW_SHAPES if nf + nm == t}
            assert kinds == {(True, False), (False, True), (True, True)}, t
        assert {nf for nf, nm in R.ROW_SHAPES if nm > 0} == {0, 1, L, L + 1}
        assert list(c['isolated']) == [0, 1]
    if name.startswith('edge'):
        np.testing.assert_allclose(R.distances(c['pos'], c['box'], c['placed']), c['placed_r'], rtol=0, atol=1e-12)
    if name == 'edge_far':
        np.testing.assert_allclose(np.sort(c['placed_r'] * c['kappa']), [2.9, 2.9, 3.3, 3.3, 3.7, 3.7], atol=1e-12)
    if name == 'edge_short':
        cls = c['cov'][c['placed'][:, 0], c['placed'][:, 1]]
        assert sorted(zip(R.MSCALES[cls - 1], c['placed_r'])) == [(m, r) for m in (0.0, 0.5) for r in (0.7, 0.96, 1.5)]
    if name == 'edge_thole':
        i, j = c['placed'][:, 0], c['placed'][:, 1]
        p = R.PSCALES[(c['cov'][i, j] - 1) % 5]
        w0 = 1.0 / (np.exp(np.minimum((p - 1e-3) / 1e-5, 700.0)) + 1.0)
        a = w0 * 0.3 + (1 - w0) * (c['thole'][i] + c['thole'][j])
        dmp = np.maximum((c['pol'][i] * c['pol'][j]) ** (1.0 / 6.0), 1e-8)
        au = a * np.minimum(c['placed_r'] / dmp, 1e8)
        np.testing.assert_allclose(au[:9], [0.1, 0.1, 5, 5, 49, 49, 51, 51, 5], rtol=1e-12)
        assert au[9] > 1e6 and dmp[9] == 1e-8
    if name == 'params':
        full = ~c['mono']
        assert (full & (c['pol'] == 0)).sum() >= 50 and (np.abs(c['Q_local'][:, 1:]).max(1) == 0)[c['pol'] > 0].sum() >= 50
        z = c['thole'] == 0
        lp = R.listed_pairs(c)
        both = z[lp[:, 0]] & z[lp[:, 1]] & (c['pol'][lp[:, 0]] > 0) & (c['pol'][lp[:, 1]] > 0)
        one = (z[lp[:, 0]] ^ z[lp[:, 1]]) & (c['pol'][lp[:, 0]] > 0) & (c['pol'][lp[:, 1]] > 0)
        assert both.sum() >= 5 and one.sum() >= 50
        assert 0 < c['pol'][c['pol'] > 0].min() < 2e-3


def test_half_the_cases_are_triclinic():
    tric = [bool(np.abs(R.case(n)['box'] - np.diag(np.diag(R.case(n)['box']))).max() > 0) for n in R.CASES]
    assert 0.4 <= np.mean(tric) <= 0.6


def rows_of(c, reduced):
    """the rows on which an output of the charge-only dispatch is complete (see test_charge_only_pair_forms_match_oracle)"""
    return {'fld': ~c['mono']} if reduced else None


@pytest.mark.parametrize('variant', ['A', 'B'])
@pytest.mark.parametrize('name', R.CASES)
def test_host_shim_reproduces_the_reference(name, variant):
    c, ref = R.case(name), R.reference(name, variant)
    mono = c['mono'] if variant == 'A' else np.zeros(c['n'], dtype=bool)
    for mode in (0, 1, 2):
        got = R.shim(c, variant, 8, mode)
        if not c['lpol']:
            got['fld'] = None
        rows = None
        if mode == 2:
            assert not got['pot'][mono, 1:].any()
            if c['lpol']:
                assert not got['fld'][mono].any()
            got = dict(got, pot0=got['pot'][:, 0])
            keep = ~mono
            ex = R.double_excess(dict(got, pot=got['pot'][keep]), dict(ref, pot=ref['pot'][keep]) if keep.any() else ref,
                                 {'fld': keep, 'grad': slice(None)}) if keep.any() else {}
            bars = R.double_bars(ref)
            np.testing.assert_allclose(got['pot'][:, 0], ref['pot'][:, 0], rtol=1e-9, atol=bars['atol']['pot'])
            assert abs(got['E'] - ref['E']) <= bars['E']
            np.testing.assert_allclose(got['grad'], ref['grad'], rtol=1e-9, atol=bars['atol']['grad'])
            ex.pop('pot', None) if not keep.any() else None
        else:
            ex = R.double_excess(got, ref, rows)
        assert all(v <= 1.0 for v in ex.values()), (name, variant, mode, ex)
    if c['lpol']:
        f = R.shim(c, variant, 8, 3)['fld']
        np.testing.assert_allclose(f, ref['fld'], rtol=1e-9, atol=R.double_bars(ref)['atol']['fld'])


@pytest.mark.parametrize('name', [n for n in R.CASES if R.case(n)['lpol']])
def test_field_increment_reference(name):
    """k_pair_field_ind's reference (the oracle at Q = 0, U = dU) against the host shim's general pair function on the same
    moments, and its single-precision floor; the emulated Jacobi step gives the dU it was asked for to rounding"""
    c = R.case(name)
    act = c['pol'] > 0
    F = R.jacobi_field(c)
    for prec, eps in (('double', 2.0 ** -52), ('single', 2.0 ** -23)):
        dU = R.jacobi_step(c, F, prec)
        want = -c['pol'][:, None] * F / R.O.DIELECTRIC
        assert np.abs(dU - want).max() <= 2 * eps * np.abs(want).max() and not dU[~act].any()
        ref = R.reference_ind(name, prec)
        got = R.shim(c, 'A', 8, 1, moments=R._ind_moments(c, prec))
        ex = R.double_excess({'fld': got['fld']}, ref, {'fld': act})
        assert ex['fld'] <= 1.0, (name, prec, ex)
    fl = R.floors_ind(name)
    print('FLOOR %-14s increment fld %.3e' % (name, fl['fld']))
    assert (fl['fld'] > 0) == bool(np.abs(R.reference_ind(name, 'single')['fld']).max() > 0) and fl['fld'] < 1e-4


@pytest.mark.parametrize('name', R.CASES)
def test_single_precision_floors(name):
    for variant in ('A', 'B'):
        fl, ref = R.floors(name, variant), R.reference(name, variant)
        print('FLOOR %-14s %s  ' % (name, variant) + '  '.join('%s %.3e' % kv for kv in fl.items()))
        for k, v in fl.items():
            scale = ref['S_E'] if k == 'E' else np.abs(ref[k]).max()
            assert np.isfinite(v) and (v > 0 or scale == 0 or k == 'E'), (name, variant, k, v)
            assert v < 1e-4, (name, variant, k, v)       # f32 (eps 6e-8) over rows of <= 100 partners: far below this


@pytest.mark.parametrize('what', ['pair', 'class', 'last', 'erfc'])
@pytest.mark.parametrize('name', R.CASES)
def test_a_wrong_result_lies_outside_the_bars(name, what):
    """double: the worst output of the wrong reference exceeds its bar; single: it exceeds FLOOR_FACTOR floors.  erfc off by a
    relative 1e-6 is of the size the single-precision bar is there to admit (device erfc: 1.2e-7 and the f32 roundings of its
    exponent), so only the double bars are asserted for it; its single ratio is printed."""
    ref, wrong, fl = R.reference(name), R.perturbed(name, what), R.floors(name)
    ex = R.double_excess(wrong, ref)
    er = R.errors(wrong, ref)
    single = {k: (er[k] / (R.FLOOR_FACTOR * fl[k]) if fl[k] > 0 else (np.inf if er[k] > 0 else 0.0)) for k in er}
    print('SENS %-14s %-5s double ' % (name, what) + ' '.join('%s %.2e' % kv for kv in ex.items()) +
          ' | single ' + ' '.join('%s %.2e' % kv for kv in single.items()))
    assert max(ex.values()) > 1.0, (name, what, ex)
    if what != 'erfc':
        assert max(single.values()) > 1.0, (name, what, single)
