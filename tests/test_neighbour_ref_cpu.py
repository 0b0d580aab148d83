"""The float64 neighbour reference and the inputs of tests/test_gpu_neighbour.py, checked without a GPU
(tests/neighbour_ref.py), and the host-side plan of the cell list (admp_amd/csrc/cell_plan.h, host-compiled).

These are conditions on the INPUTS of the GPU tests, proved on the reference alone, so that the single-precision band
rule cannot hide a failure: few reference pairs lie inside the band, a float32 evaluation of the same arithmetic differs
from the reference only inside it, and in double no pair is close enough to rc for the order of two roundings to matter.
The comparison helpers the GPU tests use are fed mutated references here (a contact pair removed, a pair doubled, a
covalent class changed) and must fail on each."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from admp_amd import systems as S
from tests import neighbour_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostshim', 'cell_plan_shim.cpp')
LIB = os.path.join(HERE, 'hostshim', 'libadmp_cellplanshim.so')
HDR = os.path.join(os.path.dirname(HERE), 'admp_amd', 'csrc', 'cell_plan.h')
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in (SRC, HDR)):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC])
        _lib = ctypes.CDLL(LIB)
        _lib.cell_plan_dims.restype = None
        _lib.cell_plan_dims.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p]
        _lib.cell_plan_partial_words.restype = ctypes.c_int64
        _lib.cell_plan_partial_words.argtypes = [ctypes.c_int]
        _lib.cell_plan_brute_max.restype = ctypes.c_int
    return _lib


def grid_dims(h, rc):
    h = np.ascontiguousarray(h, dtype=np.float64)
    n = np.zeros(3, dtype=np.int32)
    lib().cell_plan_dims(h.ctypes.data_as(ctypes.c_void_p), float(rc), n.ctypes.data_as(ctypes.c_void_p))
    return [int(x) for x in n]


def is_orthorhombic(box):
    return np.abs(box - np.diag(np.diag(box))).max() == 0


@pytest.mark.parametrize('name', R.PAIRLIST_CASES)
def test_pairlist_case_inputs(name):
    c = R.pairlist_case(name)
    pos, box, rc, ref, r = c['pos'], c['box'], c['rc'], c['ref_pairs'], c['ref_r']
    assert (rc <= 0.5 * R.heights(box) * (1 + 1e-12)).all()
    assert (c['precs'] == ('double',)) == (name in R.DOUBLE_ONLY)
    assert (ref[:, 0] < ref[:, 1]).all() and len(R.as_set(ref)) == len(ref)
    if not c['exact']:
        # double: nothing within 1e-9 of rc on either side (pairs just outside come from a slightly larger sweep)
        _, r_wide = R.brute_pairs(pos, box, rc + 2e-9)
        assert not (np.abs(r_wide - rc) < 1e-9).any()
        if is_orthorhombic(box):
            assert R.as_set(S.build_pairs(pos, box, rc)) == R.as_set(ref)
    else:
        s = R.as_set(ref)
        assert tuple(sorted(c['absent'])) not in s and tuple(sorted(c['present'])) in s
        assert R.pair_distances(pos, box, np.array([c['absent']]))[0] == rc
    if 'single' in c['precs']:
        w = R.band(pos, box)
        inside = int((np.abs(r - rc) <= w).sum())
        assert inside <= 0.005 * max(len(ref), 1) or len(ref) == 0, (inside, len(ref))
        diff = sorted(R.as_set(R.emulate_f32(pos, box, rc)) ^ R.as_set(ref))
        if diff:
            off = np.abs(R.pair_distances(pos, box, np.array(diff)) - rc)
            assert off.max() <= w, (diff[int(off.argmax())], off.max(), w)


def test_pairlist_cases_reach_their_cell_regimes():
    """the cell counts the table of the issue names, through the host-compiled plan"""
    want = {'two_cells': [2, 2, 2], 'three_cells': [3, 4, 6], 'mixed_cells': [2, 3, 8], 'multiple_rc': [4, 4, 4],
            'faces': [4, 4, 4], 'tri_b': [2, 2, 2], 'block': [3, 3, 3], 'clamp1024': [1024, 7, 7], 'halving': [256, 256, 256]}
    for name, n in want.items():
        c = R.pairlist_case(name)
        assert grid_dims(R.heights(c['box']), c['rc']) == n, name
    c = R.pairlist_case('multiple_rc')
    assert (R.heights(c['box']) / 4 == c['rc']).all()                    # cell width equals rc exactly
    assert len(R.pairlist_case('na1')['ref_pairs']) == 0 and len(R.pairlist_case('two_far')['ref_pairs']) == 0
    c = R.pairlist_case('far50')
    assert np.abs(c['pos']).max() > 900 and c['precs'] == ('double',)
    assert np.abs(R.pairlist_case('far3')['pos']).max() < 81


def test_cell_plan_grid_and_partial_words():
    """every n_d in 2..1024, n_d <= floor(height_d / rc) (cell width >= rc), at most 2^26 cells; the partial-count buffer
    holds what k_brute_rows (16 words per row, rows 0..na-1, up to kBruteMax atoms) and k_cell_rows (4 per row) index"""
    rng = np.random.default_rng(7)
    hs = [2.0, 8.0, 9.99, 10.0, 15.0, 20.0, 31.0, 100.0, 1000.0, 4096.0, 5000.0, 1e5, 3e6]
    trials = [(np.array([a, b, c]), rc) for a in hs for b in hs[::3] for c in hs[::4] for rc in (1.0, 2.5, 4.0, 5.0)]
    trials += [(rng.uniform(2, 6000, 3), rng.uniform(0.5, 12.0)) for _ in range(2000)]
    seen_clamp = seen_halve = 0
    for h, rc in trials:
        if rc > 0.5 * h.min():
            continue
        n = grid_dims(h, rc)
        for d in range(3):
            assert 2 <= n[d] <= 1024, (h, rc, n)
            assert n[d] <= np.floor(h[d] / rc), (h, rc, n)
        assert n[0] * n[1] * n[2] <= 2 ** 26, (h, rc, n)
        raw = [min(int(np.floor(h[d] / rc)), 1024) for d in range(3)]
        seen_clamp += any(np.floor(h[d] / rc) > 1024 for d in range(3))
        seen_halve += n != raw
        if raw[0] * raw[1] * raw[2] <= 2 ** 26:
            assert n == raw, (h, rc, n)                                    # the plain floor(height / rc) rule
    assert seen_clamp > 10 and seen_halve > 10
    assert grid_dims([20.0, 20.0, 20.0], 10.0) == [2, 2, 2] and grid_dims([15.0, 20.0, 31.0], 5.0) == [3, 4, 6]
    L = lib()
    bmax = L.cell_plan_brute_max()
    assert bmax == 4096
    for na in range(1, 10001):
        indexed = 16 * na if na <= bmax else 4 * na       # deg16[16 * i + l], l < 16 ; deg4[4 * i + l], l < 4 ; i < na
        assert L.cell_plan_partial_words(na) >= indexed, na
    # not monotonic in na: what the capacity of CellScratch has to track in words
    assert L.cell_plan_partial_words(2000) > L.cell_plan_partial_words(5000)


@pytest.mark.parametrize('name', R.TABLE_SYSTEMS)
def test_table_system_inputs(name):
    s = R.table_system(name)
    pos, box, rc, ref, r = s['pos'], s['box'], s['rc'], s['ref_pairs'], s['ref_r']
    assert (rc <= 0.5 * R.heights(box)).all()
    _, r_wide = R.brute_pairs(pos, box, rc + 2e-9)
    assert not (np.abs(r_wide - rc) < 1e-9).any()
    if len(r):
        assert r.min() >= (0.75 if name == 'sort_paths' else 1.0)
    inside = int((np.abs(r - rc) <= R.band(pos, box)).sum())
    assert inside <= 0.005 * max(len(ref), 1)
    a, b, q, c6 = s['params']
    assert a.min() > 0 and b.min() > 0 and len(a) == len(pos)
    assert s['cov'].max() <= 7
    if name.startswith('stars'):
        assert (np.diff(s['cov'].tocsr().indptr) == 8).all()                # eight covalent partners on every atom
        nb = np.asarray(s['cov'].tocsr()[ref[:, 0], ref[:, 1]]).ravel()
        assert (nb == 1).sum() == 8 * len(pos) // 9 and (nb == 2).sum() == 28 * len(pos) // 9    # all of them within rc
    if name == 'dilute':
        assert len(ref) == 0 and len(R.brute_pairs(pos, box, 25.0)[0]) > 100
    if name == 'switch65':
        deg = np.bincount(ref.ravel(), minlength=len(pos))
        assert (deg[:65] == 64).all() and (deg[65:] == 65).all()           # either side of the register path's limit
    if name == 'sort_paths':
        deg = np.bincount(ref.ravel(), minlength=len(pos))
        assert (deg[:343] >= 342).all() and 32 * 342 > 8192                 # a workgroup's 32 rows outgrow the LDS segment
        assert (deg[343:543] <= 64).all() and deg[343:543].min() >= 8        # register path
        assert ((deg[543:] >= 65) & (deg[543:] <= 256)).all()                # general path, LDS


def test_emulated_float32_flips_stay_in_band_when_shifted():
    """the margin quoted for the band rule: 1500 uniform atoms, cubic and skewed cells, shifted by +-3 lattice vectors"""
    rng = np.random.default_rng(11)
    for box in (np.diag([30.0] * 3), np.array([[30.0, 0, 0], [9.0, 28.0, 0], [-7.0, 6.0, 29.0]])):
        pos = rng.uniform(0, 1, (1500, 3)) @ box + rng.integers(-3, 4, (1500, 3)) @ box
        ref, r = R.brute_pairs(pos, box, 6.0)
        diff = sorted(R.as_set(R.emulate_f32(pos, box, 6.0)) ^ R.as_set(ref))
        w = R.band(pos, box)
        if diff:
            assert np.abs(R.pair_distances(pos, box, np.array(diff)) - 6.0).max() <= w
        assert (np.abs(r - 6.0) <= w).sum() <= 0.005 * len(ref)


# ---- sensitivity: the helpers of the GPU tests must reject a list that is wrong by one pair ----------------------------------
def test_helpers_fail_on_one_pair_removed_or_doubled():
    c = R.pairlist_case('na257')
    pos, box, rc, ref, r = c['pos'], c['box'], c['rc'], c['ref_pairs'], c['ref_r']
    for prec in ('double', 'single'):
        assert R.check_pair_list(ref, pos, box, rc, ref, prec) == 0.0
        k = int(r.argmin())                                                # a contact pair: far from rc
        with pytest.raises(AssertionError):
            R.check_pair_list(np.delete(ref, k, axis=0), pos, box, rc, ref, prec)
        with pytest.raises(AssertionError):
            R.check_pair_list(np.insert(ref, k, ref[k], axis=0), pos, box, rc, ref, prec)
        with pytest.raises(AssertionError):                                # the old rule let two such pairs through
            R.check_pair_list(np.delete(ref, [k, k + 1], axis=0), pos, box, rc, ref, prec)
        with pytest.raises(AssertionError):
            R.check_pair_list(ref[::-1], pos, box, rc, ref, prec)           # not grouped by i
        with pytest.raises(AssertionError):
            R.check_pair_list(ref[:, ::-1], pos, box, rc, ref, prec)        # i > j


def test_energy_helper_fails_on_one_pair_or_one_class():
    """check_tt against the reference of a list with one contact pair removed, one pair doubled, one covalent class
    changed: each must fail, in both precisions' tolerances"""
    s = R.table_system('stars40')
    pairs, r = s['ref_pairs'], s['ref_r']
    ref = R.tt_reference(s, pairs)
    nb = np.asarray(s['cov'].tocsr()[pairs[:, 0], pairs[:, 1]]).ravel()
    k = int(np.argmin(np.where(nb == 0, r, np.inf)))                         # closest non-bonded pair (full weight)
    slack = R.tt_band_slack(s, pairs, r, s['rc'])
    n_band = int((np.abs(r - s['rc']) <= R.band(s['pos'], s['box'])).sum())

    def as_got(x, n):
        return dict(E=x['E'], grad=x['grad'], dm=x['dm'], n_pairs=n)
    for prec in ('double', 'single'):
        kw = dict(slack=slack if prec == 'single' else (0, 0, 0), n_pairs_ref=len(pairs), n_band=n_band)
        R.check_tt(as_got(ref, len(pairs)), ref, prec, **kw)
        removed = R.tt_reference(s, np.delete(pairs, k, axis=0))
        with pytest.raises(AssertionError):
            R.check_tt(as_got(removed, len(pairs)), ref, prec, **kw)        # energy, gradient (count held right)
        with pytest.raises(AssertionError):
            R.check_tt(as_got(ref, len(pairs) - 1 - n_band), ref, prec, **kw)   # count alone
        doubled = R.tt_reference(s, np.insert(pairs, k, pairs[k], axis=0))
        with pytest.raises(AssertionError):
            R.check_tt(as_got(doubled, len(pairs)), ref, prec, **kw)
        # one entry's covalent class changed: a bonded centre-leaf pair (class 1, mScale 0.1) read as class 2 (0.3)
        kb = int(np.nonzero(nb == 1)[0][0])
        i, j = pairs[kb]
        cov2 = s['cov'].tolil(copy=True)
        cov2[i, j] = 2
        cov2[j, i] = 2
        wrong = R.tt_reference(dict(s, cov=cov2.tocsr()), pairs)
        with pytest.raises(AssertionError):
            R.check_tt(as_got(wrong, len(pairs)), ref, prec, **kw)
        with pytest.raises(AssertionError):                                  # seen by dE/dmScales alone as well
            R.check_tt(dict(E=ref['E'], grad=ref['grad'], dm=wrong['dm'], n_pairs=len(pairs)), ref, prec, **kw)
