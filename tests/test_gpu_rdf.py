"""Radial distribution functions on the GPU (admp_amd.md.RdfRecorder; admp_md_rdf = k_rdf_tiles / cell_bin_pack + k_rdf_cells,
rdf_kernels.hip) against the float64 reference of tests/rdf_ref.py, on the positions the device tensors actually hold.  Both
precisions throughout, except where a case says otherwise (bins_16384: its bins are narrower than the single-precision delta).

The acceptance rule is rdf_ref.violations: for every channel and every bin edge e_k, C_ref(e_k - delta) <= C_got(k) <=
C_ref(e_k + delta) on cumulative counts, delta = rho eps S.  A double handle has rho = 64, and since no reference pair lies within
delta of an edge (tests/test_rdf_cpu.py checks it) its histogram must EQUAL the reference's.  A single handle has rho = 4 x 1.11:
the host program of rdf_math.h in float arithmetic is at most 1.104 eps_f32 S from the reference on these cases
(tests/test_rdf_cpu.py measures it), recorded as rdf_ref.SINGLE_RATIO = 1.11, and the factor 4 covers another contraction order
on the device.  A grid direction of ONE cell cannot be asked for (r_max <= half a height gives two cells or more: the case
two_cells has r_max at 0.499 of the height); the sweep's rule for it is checked on the host (tests/test_rdf_cpu.py).  -s prints, per case, the form, the counts that differ from the exact histogram, and the wall time of the record."""
import ctypes
import re
import time

import numpy as np
import pytest

from tests import rdf_ref as R
from tests.test_gpu_md_langevin import run_driver

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -5      # include/admp_hip.h
TILES, CELLS = 1, 2
# every case but the histogram shapes (test_histogram_shapes) and the two of the auto choice (test_auto_choice)
FORM_CASES = tuple(n for n in R.SMALL_CASES if not n.startswith('bins_'))


@pytest.fixture(params=['double', 'single'])
def prec(request):
    from admp_amd import settings
    old = settings.PRECISION
    settings.PRECISION = request.param
    try:
        yield request.param
    finally:
        settings.PRECISION = old


def owner():
    """any object with a handle serves: the observable needs neither a topology nor pairs"""
    from admp_amd.md import HarmonicBonded
    return HarmonicBonded(1, [], [], [], [])


def dev(o, a):
    import torch
    return torch.as_tensor(np.array(a), dtype=o._dtype, device=o._device).contiguous()


_REF = {}


def ref_of(name, prec):
    """the reference of a case at the positions a handle of that precision holds; computed once, shared, never changed"""
    if (name, prec) not in _REF:
        c = R.case(name)
        _REF[(name, prec)] = R.reference(c, R.held(c, prec))
    return _REF[(name, prec)]


def recorder(o, c):
    """the recorder of a case; its tags must be the case's (raw_types: types 8 .. 14 cannot be asked for, so they are written)"""
    import torch
    from admp_amd.md import RdfRecorder
    t = np.where(c['types'] >= 8, -1, c['types'])
    rec = RdfRecorder(o, t, c['r_max'], c['n_bins'], groups=c['groups'])
    assert rec.n_types == c['n_types'] and rec.channels == c['n_types'] * (c['n_types'] + 1) // 2
    if c['name'] == 'raw_types':
        assert (rec._tags.cpu().numpy() != c['tags']).any()
        rec._tags = torch.as_tensor(c['tags']).to(o._device)
    assert np.array_equal(rec._tags.cpu().numpy(), c['tags'])
    return rec


def record(rec, o, c, force):
    import torch
    pos = dev(o, c['pos'])
    rec.force = force
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec.record(pos, c['box'])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def check(c, prec, got, label):
    ref = ref_of(c['name'], prec)
    dlt = R.delta(c, R.held(c, prec), prec)
    exact = R.exact_histogram(c, ref)
    diff = int(np.abs(got.astype(np.int64) - exact.astype(np.int64)).sum())
    bad = R.violations(c, ref, got, dlt)
    print('%s %s %s: %d pairs counted, %d counts differ from the exact histogram, %d edges violated' % (c['name'], prec, label, got.sum(), diff, bad))
    assert bad == 0
    if prec == 'double':
        assert diff == 0
    return ref, dlt


def run_form(prec, name, force):
    c = R.case(name)
    o = owner()
    rec = recorder(o, c)
    wall = record(rec, o, c, force)
    info = rec.info()
    print('%s: %s form, %d workgroups, %d B of LDS, %.1f ms' % (name, info['form'], info['workgroups'], info['lds_bytes'], wall * 1e3))
    got = rec.counts()
    assert got.dtype == np.uint64 and got.shape == (rec.channels, c['n_bins']) and rec.frames == 1
    check(c, prec, got, info['form'])
    return c, rec, info, got


# ---- 1. the tile form at its edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FORM_CASES)
def test_tile_form(prec, name):
    c, rec, info, got = run_form(prec, name, TILES)
    nt = (c['n'] + 255) // 256
    assert info['form'] == 'tiles' and info['tiles'] == nt and info['workgroups'] == nt * (nt + 1) // 2
    if name == 'one_group':
        assert got.sum() == 0
    if name in ('n1',):
        assert got.sum() == 0


# ---- 2. the cell form, forced -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FORM_CASES)
def test_cell_form(prec, name):
    c, rec, info, got = run_form(prec, name, CELLS)
    assert info['form'] == 'cells' and info['workgroups'] == info['cells']
    if name in R.GRIDS:
        assert info['cells'] == int(np.prod(R.GRIDS[name]))
    if name == 'one_group':
        assert got.sum() == 0


# ---- 3. the two forms of one case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['water64_skew', 'n513', 'two_cells', 'faces', 'cluster'])
def test_forms_agree(prec, name):
    """each satisfies the rule (tests 1 and 2); their totals per channel differ by no more than the pairs the reference has within
    delta of r_max, the only ones the two may bin differently into or out of the last bin"""
    c = R.case(name)
    o = owner()
    tot = []
    for force in (TILES, CELLS):
        rec = recorder(o, c)
        record(rec, o, c, force)
        tot.append(rec.counts().astype(np.int64).sum(axis=1))
        ref, dlt = check(c, prec, rec.counts(), rec.info()['form'])
    band = np.array([int(((r >= c['r_max'] - dlt) & (r < c['r_max'] + dlt)).sum()) for r in ref])
    print('%s %s: totals %s against %s, last band %s' % (name, prec, tot[0].tolist(), tot[1].tolist(), band.tolist()))
    assert (np.abs(tot[0] - tot[1]) <= band).all()


# ---- 4. the auto choice ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, form', [('n4096', 'tiles'), ('n4097', 'cells')])
def test_auto_choice(prec, name, form):
    c, rec, info, got = run_form(prec, name, 0)
    assert info['form'] == form
    if form == 'cells':
        assert info['cells'] == int(np.prod(R.GRIDS[name]))
    else:
        assert info['tiles'] == 16 and info['workgroups'] == 136


# ---- 5. histogram shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('force', [TILES, CELLS])
def test_histogram_shapes(prec, force):
    from admp_amd.md import RdfRecorder
    for name in ('bins_1', 'bins_16384', 'bins_36x455'):
        c = R.case(name)
        if prec == 'single' and not c['single']:
            continue                     # (the case says so: its bins are narrower than the single-precision delta)
        _, rec, info, got = run_form(prec, name, force)
        assert rec.channels * rec.n_bins == {'bins_1': 3, 'bins_16384': 16384, 'bins_36x455': 16380}[name]
        assert info['lds_bytes'] >= 4 * rec.channels * rec.n_bins
    # one counter more is refused: by the class, and by the library
    o = owner()
    with pytest.raises(ValueError, match='16384'):
        RdfRecorder(o, np.zeros(5, dtype=int), 3.0, 16385)
    with pytest.raises(ValueError, match='16384'):
        RdfRecorder(o, np.arange(8), 3.0, 456)
    c = R.case('bins_36x455')
    rec = recorder(o, c)
    rec.n_bins = 456
    with pytest.raises(ValueError, match='16384'):
        rec.record(dev(o, c['pos']), c['box'])
    rec.n_bins = 455
    assert rec.frames == 0 and rec.counts().sum() == 0


# ---- 6. accumulation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('force', [TILES, CELLS])
def test_accumulation(prec, force):
    import torch
    c = R.case('water64_skew')
    o = owner()
    rec = recorder(o, c)
    rec.force = force
    a = dev(o, c['pos'])
    b = dev(o, c['pos'] + 0.05 * np.random.default_rng(3).normal(size=c['pos'].shape))
    rec.record(a, c['box'])
    one = rec.counts().copy()
    assert one.sum() > 0
    rec.record(a, c['box'])
    assert np.array_equal(rec.counts(), 2 * one) and rec.frames == 2
    rec.reset()
    assert rec.counts().sum() == 0 and rec.frames == 0 and rec.sum_inv_volume == 0.0
    rec.record(b, c['box'])
    other = rec.counts().copy()
    assert not np.array_equal(other, one)
    rec.record(a, c['box'])
    assert np.array_equal(rec.counts(), one + other)
    assert abs(rec.sum_inv_volume - 2.0 / abs(np.linalg.det(c['box']))) < 1e-15
    # a repeated run: bit for bit, on a fresh handle too
    rec2 = recorder(owner(), c)
    rec2.force = force
    rec2.record(b, c['box'])
    rec2.record(a, c['box'])
    assert np.array_equal(rec2.counts(), rec.counts())
    # a non-default torch stream
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rec.reset()
        rec.record(a, c['box'])
        rec.record(b, c['box'])
    s.synchronize()
    assert np.array_equal(rec.counts(), one + other)
    # g(r) and the coordination numbers of the recorder are rdf_normalise of its counts
    from admp_amd.md import rdf_normalise
    r, g, n = rec.rdf()
    r2, g2, n2 = rdf_normalise(rec.counts(), [64, 128], c['r_max'], 2, 2.0 / abs(np.linalg.det(c['box'])))
    assert np.array_equal(r, r2) and all(np.allclose(g[k], g2[k], rtol=1e-14) and np.array_equal(n[k], n2[k]) for k in g)
    assert n[(0, 0)][-1] > 1.0 and n[(0, 1)][-1] == 2.0 * n[(1, 0)][-1]      # twice as many H around an O as O around an H


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(prec):
    import torch
    from admp_amd import _lib
    from admp_amd.md import RdfRecorder
    c = R.case('water64')
    o = owner()
    L, h = o._L, o._h
    rec = recorder(o, c)
    pos = dev(o, c['pos'])
    rec.record(pos, c['box'])
    one = rec.counts().copy()
    rec.reset()
    hist, tags = rec._hist, rec._tags
    info = (ctypes.c_int64 * 4)()
    box = _lib.darr(c['box'])
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    good = [c['n'], P(pos), box, P(tags), 2, c['r_max'], c['n_bins'], P(hist), 0, info]
    o._use_current_stream()
    n_good = 0

    def refused(k, value, code=E_ARG):
        nonlocal n_good
        a = list(good)
        a[k] = value
        assert L.admp_md_rdf(h, *a) == code, (k, value)
        assert L.admp_last_error(h)
        assert L.admp_md_rdf(h, *good) == 0               # the handle serves a valid call after every refusal
        n_good += 1

    for k in (1, 2, 3, 7):                                  # every required pointer
        refused(k, None)
    refused(0, -1)
    for v in (0, 9, -3):
        refused(4, v)
    for v in (0, -1):
        refused(6, v)
    refused(6, 16384 // 3 + 1)                              # 3 channels x 5462 bins: one row of counters too many
    h_min = float(R.heights(c['box']).min())
    for v in (0.0, -1.0, 0.5001 * h_min, float('nan'), float('inf')):
        refused(5, v)
    refused(8, 3)
    refused(8, -1)
    for bad in (np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]]), np.zeros((3, 3)), c['box'] + np.diag([0.0, np.nan, 0.0]),
                c['box'] + np.diag([0.0, np.inf, 0.0])):
        refused(2, _lib.darr(bad))
    a = list(good)
    a[5] = 0.5 * h_min * (1 - 1e-12)                        # up to half the smallest height is served
    a[6] = 1
    a[7] = P(torch.zeros(3, dtype=torch.int64, device=o._device))
    assert L.admp_md_rdf(h, *a) == 0
    torch.cuda.synchronize()
    assert np.array_equal(rec.counts(), n_good * one)       # nothing but the valid calls was counted
    # no atoms: nothing launched, NULL positions and tags pass, info says so
    a = list(good)
    a[0], a[1], a[3] = 0, None, None
    assert L.admp_md_rdf(h, *a) == 0 and list(info) == [0, 0, 0, 0]
    empty = RdfRecorder(o, np.zeros(0, dtype=int), 3.0, 10)
    empty.record(dev(o, np.zeros((0, 3))), c['box'])
    assert empty.counts().sum() == 0 and empty.info()['form'] == 'none' and empty.frames == 1
    torch.cuda.synchronize()
    assert np.array_equal(rec.counts(), n_good * one)
    # a slab-decomposed handle: ADMP_E_STATE, before any other argument
    slab = owner()
    _lib.check(slab._h, L.admp_slab_configure(slab._h, 0, 2), 'admp_slab_configure')
    slab._use_current_stream()
    assert L.admp_md_rdf(slab._h, *good) == E_STATE and b'single-rank' in L.admp_last_error(slab._h)
    a = list(good)
    a[1] = None
    assert L.admp_md_rdf(slab._h, *a) == E_STATE
    with pytest.raises(_lib.AdmpHipError, match='single-rank'):
        recorder(slab, c).record(pos, c['box'])
    torch.cuda.synchronize()
    assert np.array_equal(rec.counts(), n_good * one)
    # Python: the library reads raw pointers
    other = torch.float32 if o._dtype == torch.float64 else torch.float64
    for bad in (pos.to(other), pos[:-1], pos.cpu(), torch.stack([pos, pos], dim=1)[:, 0], c['pos']):
        with pytest.raises(ValueError):
            rec.record(bad, c['box'])
    with pytest.raises(ValueError):
        rec.record(pos, np.zeros((3, 3)))                   # the library's refusal of the box
    with pytest.raises(ValueError):
        rec.record(pos, c['box'] * 0.9)                     # r_max = 0.49 of the smallest height no longer fits
    for args in (([8], 3.0, 10), ([0.5], 3.0, 10), ([0, 1], 0.0, 10), ([0, 1], float('nan'), 10), ([0, 1], 3.0, 0), ([0, 1], 3.0, 2.5)):
        with pytest.raises(ValueError):
            RdfRecorder(o, *args)
    with pytest.raises(ValueError):
        RdfRecorder(o, [0, 1], 3.0, 10, groups=[0])
    assert rec.frames == 0                                  # (reset above; the raw calls do not count frames)
    rec.record(pos, c['box'])                               # and the recorder serves a valid call
    assert np.array_equal(rec.counts(), (n_good + 1) * one) and rec.frames == 1


# ---- 8. a driver end to end ---------------------------------------------------------------------------------------------------------
def test_nvt_driver_reports_the_rdf():
    """64 waters, 20 steps, a frame every 5: the lines are there, 4 frames were counted, g_OO is zero below 2 A"""
    out = run_driver('nvt_water.py', '--waters', '64', '--steps', '20', '--rdf', '5')
    m = re.search(r'# rdf over (\d+) frames: r_max ([0-9.]+) A, (\d+) bins of ([0-9.]+) A, (\w+) form, (\d+) workgroups', out)
    assert m, out[-1500:]
    print(m.group(0))
    assert int(m.group(1)) == 4 and m.group(5) == 'tiles' and int(m.group(6)) == 1
    assert abs(float(m.group(4)) - 0.05) < 2e-3 and 5.0 < float(m.group(2)) <= 10.0
    m = re.search(r'# g_OO: first maximum ([0-9.]+) at ([0-9.]+) A, first minimum ([0-9.]+) at ([0-9.]+) A, O-O coordination number up '
                  r'to the minimum ([0-9.]+); g_OO is zero below ([0-9.]+) A', out)
    assert m, out[-1500:]
    print(m.group(0))
    peak, r_peak, low, r_low, n_oo, zero_below = (float(x) for x in m.groups())
    assert zero_below >= 2.0
    assert 2.0 < r_peak < 3.6 and r_low > r_peak and peak > 1.0 and low < peak and 0.5 < n_oo < 20.0
    m = re.search(r'# g_OH: first intermolecular maximum ([0-9.]+) at ([0-9.]+) A', out)
    assert m, out[-1500:]
    print(m.group(0))
    assert 1.3 < float(m.group(2)) < 2.5
