"""The arithmetic and the plan of the radial distribution functions on the host (admp_amd/csrc/rdf_math.h, rdf_plan.h: the text
the kernels of rdf_kernels.hip compile; tests/rdf_shim/main.cpp) against the float64 reference of tests/rdf_ref.py, the pure-numpy
normalisation of admp_amd.md, and the acceptance rule itself against six perturbed references.

Double arithmetic is held to delta = 64 eps_f64 S, and since no reference pair lies within delta of an edge its histogram must
equal the reference's exactly.  Float arithmetic is MEASURED: the largest |r_f32 - r_f64| / (eps_f32 S) over the pairs below r_max
of all small cases is printed with -s and held to rdf_ref.SINGLE_RATIO, the figure the GPU test's single-precision bar is four
times of.  Measured here: 1.104 (case n513_unwrapped, atoms up to three cells outside; every other case at most 0.47; recorded as 1.11)."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import rdf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ROOT + '/admp_amd/csrc'
SHIM = ROOT + '/tests/rdf_shim/main.cpp'


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the headers cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('rdf_shim') / 'rdf_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I', CSRC, '-o', exe, SHIM])
    return exe


def run(shim, *args, text=None):
    return subprocess.run([shim, *args], input=text, capture_output=True, text=True, check=True).stdout


def case_input(c, pos):
    lines = ['%d %d %d %.17g' % (c['n'], c['n_types'], c['n_bins'], c['r_max']), ' '.join('%.17g' % x for x in c['box'].reshape(-1))]
    lines += ['%.17g %.17g %.17g %d' % (*p, t) for p, t in zip(pos, c['tags'])]
    return '\n'.join(lines) + '\n'


def shim_histogram(shim, c, prec):
    out = run(shim, prec, 'h', text=case_input(c, R.held(c, prec)))
    return np.array(out.split(), dtype=np.uint64).reshape(-1, c['n_bins'])


_REF = {}


def ref_of(name, prec):
    """the reference of a case at the positions a handle of that precision holds, computed once"""
    key = (name, prec)
    if key not in _REF:
        c = R.case(name)
        _REF[key] = R.reference(c, R.held(c, prec))
    return _REF[key]


# ---- the cases are what they claim, and meet the conditions of the rule ----------------------------------------------------------
@pytest.mark.parametrize('name', R.CASES)
def test_conditions_of_the_rule(name):
    c = R.case(name)
    assert c['r_max'] <= 0.5 * R.heights(c['box']).min()
    counted = c['types'][(c['types'] >= 0) & (c['types'] < c['n_types'])]
    assert set(counted.tolist()) == set(range(c['n_types'])), 'every type of the case occurs'
    # double: no reference pair within delta of an edge
    ref = ref_of(name, 'd')
    near, total, closest = R.near_edges(c, ref, R.delta(c, R.held(c, 'd'), 'double'))
    print('%s: %d counted pairs below r_max; double: the closest pair to an edge is %.3g delta away' % (name, total, closest))
    assert near == 0
    if name not in ('n1', 'one_group'):
        assert total > 0
    # single: at most 1 % of the counted pairs within delta (the GPU's: four times the measured ratio) of any edge
    ref = ref_of(name, 'f')
    near, total, _ = R.near_edges(c, ref, R.delta(c, R.held(c, 'f'), 'single'))
    print('%s: single: %d of %d pairs within delta of an edge' % (name, near, total))
    if c['single']:
        assert near <= 0.01 * total
    else:
        assert near > 0.01 * total      # why the case runs in double only


def test_the_cases_are_what_they_claim():
    assert R.case('water64')['n_straddling'] >= 1 and R.case('water64_skew')['n_straddling'] >= 1
    c = R.case('n513_unwrapped')
    s = c['pos'] @ np.linalg.inv(c['box'])
    assert s.min() < -2 and s.max() > 3
    c = R.case('cluster')
    cells = np.floor(c['pos'] @ np.linalg.inv(c['box']) * 3).astype(int)
    assert (cells == cells[0]).all() and c['n'] > 256
    c = R.case('faces')
    s = c['pos'] @ np.linalg.inv(c['box']) * np.array([3, 4, 5])
    assert (s == np.rint(s)).any(axis=1).sum() >= 50 and (c['pos'] @ np.linalg.inv(c['box']) == 1.0).any()
    assert set((R.case('raw_types')['types']).tolist()) >= set(range(8, 15))
    assert (R.case('n513')['types'] == R.NOT_COUNTED).sum() > 50
    assert len(R.reference(R.case('one_group'))[0]) == 0
    for name in ('n256', 'n513', 'n513_unwrapped', 'water64_skew', 'eight_types', 'two_cells_skew'):
        b = R.case(name)['box']
        assert np.abs(b - np.diag(np.diag(b))).max() > 1.0
    # the brute force over 27 translations against the plain fractional wrap, below half the smallest height
    c = R.case('n513_unwrapped')
    i, j, r, _ = R.counted_pairs(c)
    d = c['pos'][i] - c['pos'][j]
    s = d @ np.linalg.inv(c['box'])
    w = (s - np.floor(s + 0.5)) @ c['box']
    assert np.abs(np.sqrt((w * w).sum(axis=1)) - r)[r < c['r_max']].max() < 1e-12


# ---- the host program's histograms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.SMALL_CASES)
def test_double_arithmetic_equals_the_reference_histogram(shim, name):
    c = R.case(name)
    got = shim_histogram(shim, c, 'd')
    ref = ref_of(name, 'd')
    assert R.violations(c, ref, got, R.delta(c, R.held(c, 'd'), 'd')) == 0
    assert np.array_equal(got, R.exact_histogram(c, ref))
    if name == 'one_group':
        assert got.sum() == 0


@pytest.mark.parametrize('name', [n for n in R.SMALL_CASES if R.case(n)['single']])
def test_float_arithmetic_meets_the_rule_at_the_recorded_ratio(shim, name):
    c = R.case(name)
    got = shim_histogram(shim, c, 'f')
    ref = ref_of(name, 'f')
    assert R.violations(c, ref, got, R.delta(c, R.held(c, 'f'), 'f')) == 0
    diff = int(np.abs(got.astype(np.int64) - R.exact_histogram(c, ref).astype(np.int64)).sum())
    print('%s: %d counts differ from the exact histogram of %d pairs' % (name, diff, got.sum()))


def test_float_ratio_is_measured_and_within_the_recorded_figure(shim):
    worst = 0.0
    for name in R.SMALL_CASES:
        c = R.case(name)
        pos = R.held(c, 'f')
        i, j, r, _ = R.counted_pairs(c, pos)
        want = {}
        for a, b, x in zip(i.tolist(), j.tolist(), r.tolist()):
            want[(a, b)] = x
        out = np.array(run(shim, 'f', 'r', text=case_input(c, pos)).split(), dtype=np.float64).reshape(-1, 3)
        if len(out) == 0:
            continue
        ref = np.array([want[(int(a), int(b))] for a, b, _ in out])      # (KeyError: a pair the reference does not have below R)
        x = float(np.abs(out[:, 2] - ref).max() / (R.EPS32 * R.scale(c, pos)))
        print('%s: %d pairs, |r_f32 - r_f64| / (eps_f32 S) at most %.3f' % (name, len(out), x))
        worst = max(worst, x)
    print('largest %.3f, recorded %.3f' % (worst, R.SINGLE_RATIO))
    assert worst <= R.SINGLE_RATIO


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def test_every_tile_pair_is_met_exactly_once(shim):
    for nt in range(1, 18):
        rows = np.array(run(shim, 'tiles', str(nt)).split(), dtype=np.int64).reshape(-1, 3)
        assert rows[:, 0].tolist() == list(range(nt * (nt + 1) // 2))
        assert sorted(map(tuple, rows[:, 1:].tolist())) == [(a, b) for a in range(nt) for b in range(a, nt)]
        assert all(R.channel(a, b, nt) == w for w, a, b in rows.tolist())      # the index of rdf_channel, read backwards


def neighbours(g):
    """the unordered pairs of different cells that see each other: along a direction of 3 cells or more the coordinates differ by
    at most one (periodically), along one of fewer by anything"""
    cells = list(itertools.product(*[range(x) for x in g]))
    idx = {c: k for k, c in enumerate(cells)}
    out = set()
    for a in cells:
        for b in cells:
            if a < b and all(n < 3 or (x - y) % n in (0, 1, n - 1) for x, y, n in zip(a, b, g)):
                out.add((idx[a], idx[b]))
    return out


def test_the_half_sweep_meets_every_pair_of_neighbouring_cells_exactly_once(shim):
    for g in itertools.product((1, 2, 3, 5), repeat=3):
        rows = np.array(run(shim, 'sweep', *map(str, g)).split(), dtype=np.int64).reshape(-1, 3)
        own = rows[rows[:, 2] == 0]
        assert sorted(own[:, 0].tolist()) == list(range(g[0] * g[1] * g[2])) and (own[:, 0] == own[:, 1]).all()
        taken = [tuple(sorted(p)) for p in rows[rows[:, 2] == 1][:, :2].tolist()]
        assert len(taken) == len(set(taken)), g
        assert set(taken) == neighbours(g), g
        if min(g) >= 3:      # 13 of the 26 neighbours, for every home cell
            assert (np.bincount(rows[rows[:, 2] == 1][:, 0]) == 13).all() or 3 in g
            if min(g) >= 5:
                assert (np.bincount(rows[rows[:, 2] == 1][:, 0]) == 13).all()


def plan(shim, n, heights, r_max, n_types, n_bins, real_bytes, force):
    out = run(shim, 'plan', str(n), *('%.17g' % h for h in heights), '%.17g' % r_max, str(n_types), str(n_bins), str(real_bytes),
              str(force)).split(None, 1)
    if out[0] == 'error':
        return out[1].strip()
    return dict(zip(('form', 'tiles', 'g0', 'g1', 'g2', 'cells', 'workgroups', 'lds', 'counters'), map(int, out[1].split())))


def test_plan_forms_grids_and_the_lds_cap(shim):
    H = (30.0, 31.0, 32.0)
    p = plan(shim, R.KBRUTE, H, 9.0, 2, 100, 8, 0)
    assert (p['form'], p['tiles'], p['workgroups']) == (1, 16, 136)
    p = plan(shim, R.KBRUTE + 1, H, 9.0, 2, 100, 8, 0)
    assert (p['form'], p['g0'], p['g1'], p['g2'], p['cells'], p['workgroups']) == (2, 3, 3, 3, 27, 27)
    assert plan(shim, R.KBRUTE + 1, H, 9.0, 2, 100, 8, 1)['form'] == 1 and plan(shim, 10, H, 9.0, 2, 100, 8, 2)['form'] == 2
    assert plan(shim, 0, H, 9.0, 2, 100, 8, 0)['form'] == 0
    assert plan(shim, 257, H, 9.0, 2, 100, 4, 1)['workgroups'] == 3 and plan(shim, 513, H, 9.0, 2, 100, 4, 1)['workgroups'] == 6
    for name, grid in R.GRIDS.items():
        c = R.case(name)
        p = plan(shim, c['n'], R.heights(c['box']), c['r_max'], c['n_types'], c['n_bins'], 8, 2)
        assert (p['g0'], p['g1'], p['g2']) == grid, name
    # LDS: the counters, then the staged atoms; at the cap two workgroups share a CU's 160 KB
    for real in (4, 8):
        t, cl = plan(shim, 300, H, 9.0, 1, 16384, real, 1), plan(shim, 300, H, 9.0, 1, 16384, real, 2)
        assert t['lds'] == 65536 + 512 * (3 * real + 4) and cl['lds'] == 65536 + 256 * (3 * real + 4)
        assert 2 * t['lds'] <= 160 * 1024
        assert plan(shim, 300, H, 9.0, 8, 455, real, 1)['counters'] == 16380
        assert 'counters' in plan(shim, 300, H, 9.0, 1, 16385, real, 1) and 'counters' in plan(shim, 300, H, 9.0, 8, 456, real, 2)
    # refusals
    assert 'n_atoms' in plan(shim, -1, H, 9.0, 2, 100, 8, 0)
    assert 'n_types' in plan(shim, 10, H, 9.0, 0, 100, 8, 0) and 'n_types' in plan(shim, 10, H, 9.0, 9, 100, 8, 0)
    assert 'n_bins' in plan(shim, 10, H, 9.0, 2, 0, 8, 0)
    assert 'r_max' in plan(shim, 10, H, 0.0, 2, 100, 8, 0) and 'r_max' in plan(shim, 10, H, -1.0, 2, 100, 8, 0)
    assert 'half' in plan(shim, 10, H, 15.001, 2, 100, 8, 0) and plan(shim, 10, H, 15.0, 2, 100, 8, 0)['form'] == 1
    assert 'half' in plan(shim, 10, H, float('nan'), 2, 100, 8, 0) or 'r_max' in plan(shim, 10, H, float('nan'), 2, 100, 8, 0)
    assert 'force' in plan(shim, 10, H, 9.0, 2, 100, 8, 3)


# ---- the normalisation ----------------------------------------------------------------------------------------------------------
def test_rdf_normalise():
    from admp_amd.md import rdf_channel, rdf_normalise, rdf_tags
    assert [rdf_channel(a, b, 3) for a in range(3) for b in range(a, 3)] == list(range(6)) and rdf_channel(2, 0, 3) == rdf_channel(0, 2, 3)
    assert all(rdf_channel(a, b, 8) == R.channel(a, b, 8) for a in range(8) for b in range(8))
    rng = np.random.default_rng(5)
    N, n_bins, r_max, frames = np.array([64, 128]), 40, 6.0, 7
    counts = rng.integers(0, 500, size=(3, n_bins)).astype(np.uint64)
    V = 1900.0
    r, g, n = rdf_normalise(counts, N, r_max, frames, frames / V)
    edges = np.arange(n_bins + 1) * r_max / n_bins
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    assert np.allclose(r, 0.5 * (edges[1:] + edges[:-1]), rtol=0, atol=1e-14)
    assert set(g) == set(n) == {(0, 0), (0, 1), (1, 0), (1, 1)} and g[(0, 1)] is g[(1, 0)]
    # sum_k g rho_b V_shell is the coordination number: rho_b = N_b / V for a != b, (N_a - 1) / V for a = b (the partners)
    assert np.allclose(np.cumsum(g[(0, 1)] * N[1] / V * shell), n[(0, 1)], rtol=1e-13)
    assert np.allclose(np.cumsum(g[(0, 1)] * N[0] / V * shell), n[(1, 0)], rtol=1e-13)
    assert np.allclose(np.cumsum(g[(0, 0)] * (N[0] - 1) / V * shell), n[(0, 0)], rtol=1e-13)
    assert np.allclose(np.cumsum(g[(1, 1)] * (N[1] - 1) / V * shell), n[(1, 1)], rtol=1e-13)
    # a = b against a != b: the same counts, N_a (N_a - 1) / 2 against N_a N_b pairs, every pair belonging to two atoms
    c2 = np.stack([counts[0], counts[0], counts[0]])
    _, g2, n2 = rdf_normalise(c2, np.array([64, 64]), r_max, frames, frames / V)
    assert np.allclose(g2[(0, 0)] * (64 * 63 / 2), g2[(0, 1)] * (64 * 64), rtol=1e-13)
    assert np.allclose(n2[(0, 0)], 2.0 * n2[(0, 1)], rtol=1e-13)
    # by hand: 2 atoms of one type, one pair in bin 0 of 2 bins to r_max = 2, one frame, V = 10: g = 1 / (1 x 4 pi / 3 x 1 / 10)
    _, g1, n1 = rdf_normalise(np.array([[1, 0]]), [2], 2.0, 1, 0.1)
    assert abs(g1[(0, 0)][0] - 10.0 / (4.0 * np.pi / 3.0)) < 1e-13 and g1[(0, 0)][1] == 0 and n1[(0, 0)].tolist() == [1.0, 1.0]
    # a varying volume: an ideal gas has <counts> = N_pairs V_shell / V per frame, so the sum over the frames normalises to g = 1
    vols = np.array([1000.0, 1500.0, 2300.0])
    ideal = np.stack([sum(p * shell / v for v in vols) for p in (64 * 63 / 2, 64 * 128, 128 * 127 / 2)])
    _, gi, _ = rdf_normalise(ideal, N, r_max, len(vols), (1.0 / vols).sum())
    assert all(np.allclose(x, 1.0, rtol=1e-13) for x in gi.values())
    _, gw, _ = rdf_normalise(ideal, N, r_max, len(vols), len(vols) / vols.mean())      # (the mean volume is NOT exact)
    assert abs(gw[(0, 1)][0] - 1.0) > 1e-3
    # empty channels and no frames give zeros, not NaN
    _, g0, n0 = rdf_normalise(np.zeros((3, 4)), [0, 5], 2.0, 0, 0.0)
    assert all((x == 0).all() for x in list(g0.values()) + list(n0.values()))
    with pytest.raises(ValueError):
        rdf_normalise(np.zeros((2, 4)), [1, 1], 2.0, 1, 1.0)
    # the tags
    tags, nt, per = rdf_tags([0, 1, -1, 1], [7, 7, 9, -4])
    assert tags.dtype == np.int32 and nt == 2 and per.tolist() == [1, 2]
    assert (tags & 15).tolist() == [0, 1, 15, 1] and (tags >> 4).tolist() == [1, 1, 2, 0]
    assert (rdf_tags([0, 0, 3])[0] >> 4).tolist() == [0, 1, 2] and rdf_tags([0, 0, 3])[1] == 4 and rdf_tags([])[1] == 1
    for bad in (([8],), ([0.5],), ([[0]],), ([0, 1], [0]), ([0, 1], [0.5, 1.0])):
        with pytest.raises(ValueError):
            rdf_tags(*bad)


# ---- the rule catches what it must -------------------------------------------------------------------------------------------------
def test_six_perturbed_references_break_the_rule():
    c = R.case('water64')
    pos = R.held(c, 'd')
    dlt = R.delta(c, pos, 'double')
    ref = ref_of('water64', 'd')
    got = R.exact_histogram(c, ref)
    assert R.violations(c, ref, got, dlt) == 0 and all(len(r) > 100 for r in ref)
    dr = c['r_max'] / c['n_bins']
    oo, oh = R.channel(0, 0, 2), R.channel(0, 1, 2)

    def changed(k, new):
        out = list(ref)
        out[k] = np.sort(new)
        return out
    perturbed = {
        'one pair dropped': changed(oh, np.delete(ref[oh], 17)),
        'one pair counted twice': changed(oo, np.append(ref[oo], ref[oo][5])),
        'an excluded intramolecular pair counted': changed(oh, np.append(ref[oh], 0.9572)),
        'two channels swapped': [ref[1], ref[0], ref[2]],
        'all bins shifted by one': [r + dr for r in ref],
    }
    # a wrong image: the first O-O pair seen through the next cell along x instead of the nearest image
    i, j, r, ch = R.counted_pairs(c, pos)
    k = int(np.nonzero(ch == oo)[0][0])
    d = pos[i[k]] - pos[j[k]]
    d = d - np.rint(d @ np.linalg.inv(c['box'])) @ c['box']
    assert abs(np.linalg.norm(d) - r[k]) < 1e-12
    wrong = float(np.linalg.norm(d + c['box'][0] * (1.0 if d[0] > 0 else -1.0)))
    assert wrong > r[k] + dr
    perturbed['a wrong image'] = changed(oo, np.append(np.delete(ref[oo], np.searchsorted(ref[oo], r[k])), wrong))
    assert len(perturbed) == 6
    for what, bad in perturbed.items():
        v = R.violations(c, bad, got, dlt)
        print('%s: %d edges violated' % (what, v))
        assert v > 0, what
