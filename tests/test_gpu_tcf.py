"""Time correlation functions on the GPU (admp_amd.md.CorrelationRecorder; admp_md_tcf = k_tcf_push, k_tcf_lags, k_tcf_fold of
tcf_kernels.hip) against the float64 reference of tests/tcf_ref.py on the frames the device tensors actually hold, both
precisions.  The acceptance bar is the one tcf_ref derives and tests/test_tcf_cpu.py holds the host restatement to: the GPU does
the same double arithmetic.  -s prints err / bar, the workgroups of the lag kernel and the wall time per case."""
import ctypes
import re
import time

import numpy as np
import pytest

from tests import tcf_ref as R
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


def owner():
    """any object with a handle serves: the observable needs neither a topology nor pairs"""
    from admp_amd.md import HarmonicBonded
    return HarmonicBonded(1, [], [], [], [])


def dev(o, a):
    import torch
    return torch.as_tensor(np.array(a), dtype=o._dtype, device=o._device).contiguous()


_REF = {}


def ref_of(name, prec, frames=None):
    """the reference of the first `frames` frames of a case as a handle of that precision holds them; computed once, never changed"""
    if (name, prec, frames) not in _REF:
        c = R.case(name)
        _REF[(name, prec, frames)] = R.reference(c, *R.held(c, prec, frames))
    return _REF[(name, prec, frames)]


def recorder(o, c, tile_atoms=256):
    from admp_amd.md import CorrelationRecorder
    rec = CorrelationRecorder(o, c['types'], c['n_lags'], c['dt'], tile_atoms=tile_atoms)
    assert rec.n_types == c['n_types'] and rec.n_slots == rec.n_tiles * tile_atoms
    return rec


def frames_on(o, c):
    return [(dev(o, p), dev(o, v), b) for p, v, b in zip(c['pos'], c['vel'], c['box'])]


def feed(rec, frames, start, stop):
    for p, v, b in frames[start:stop]:
        rec.record(p, v, b)


def check(name, prec, rec, frames, label='', ref_name=None, other_input=False):
    ref = ref_of(ref_name or name, prec, frames)
    s = rec.sums()
    ratio = R.worst_ratio(ref, prec, s['msd'], s['vacf'], other_input)
    print('%s %s %s %d frames: err / bar = %.3g' % (name, prec, label, frames, ratio))
    assert ratio <= 1.0
    assert np.array_equal(s['origins'], np.maximum(0, frames - np.arange(rec.n_lags))) and np.array_equal(s['origins'], ref['origins'])
    assert (s['msd'][:, 0] == 0).all() and (s['msd'][:, frames:] == 0).all() and (s['vacf'][:, frames:] == 0).all()
    return ref


# ---- 1. every case, two tile sizes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile_atoms', [64, 256])
@pytest.mark.parametrize('name', R.CASES)
def test_cases_within_the_bar(prec, name, tile_atoms):
    import torch
    c = R.case(name)
    o = owner()
    rec = recorder(o, c, tile_atoms)
    frames = frames_on(o, c)
    done = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for stop in R.checkpoints(c):
        feed(rec, frames, done, stop)
        done = stop
        ref = check(name, prec, rec, stop, 'tile %d' % tile_atoms)
        info = rec.info()
        lags_now = min(stop - 1, c['n_lags'] - 1) + 1
        assert info['lags'] == lags_now and info['lags_per_workgroup'] == R.LAGS_PER_WORKGROUP
        assert info['workgroups'] == rec.n_tiles * -(-lags_now // R.LAGS_PER_WORKGROUP)
        assert info['scratch_bytes'] == 2 * rec.n_tiles * c['n_lags'] * 8 and info['large_jumps'] == ref['jumps']
    print('%s: %d tiles, %d workgroups at the end, %.1f ms for %d frames and %d reads' % (name, rec.n_tiles, info['workgroups'],
          (time.perf_counter() - t0) * 1e3, done, len(R.checkpoints(c))))
    assert rec.frames == done


# ---- 1b. more than one slot per lane -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile_atoms', [320, 512, 768, 1024])
def test_tiles_above_256_slots(prec, tile_atoms):
    """a lane holds 2, 2, 3 and 4 slots 256 apart; 320: the last of them only in the first wave; the result meets the same bar and
    (the order of a tile's sum differs) need not equal the 256-slot one bit for bit"""
    for name in ('types_gap', 'n257'):
        c = R.case(name)
        o = owner()
        rec = recorder(o, c, tile_atoms)
        fr = frames_on(o, c)
        feed(rec, fr, 0, len(fr))
        check(name, prec, rec, len(fr), 'tile %d' % tile_atoms)
        assert rec.info()['workgroups'] == rec.n_tiles and rec.n_tiles == (2 if name == 'types_gap' else 1)


# ---- 2. bit repeatability -----------------------------------------------------------------------------------------------------------------
def test_bit_repeatable_and_recorders_do_not_disturb_each_other(prec):
    import torch
    a, b = R.case('types_gap'), R.case('lags_7')
    o1, o2 = owner(), owner()
    fa1, fb1, fa2 = frames_on(o1, a), frames_on(o1, b), frames_on(o2, a)
    ra1, rb1, ra2 = recorder(o1, a, 64), recorder(o1, b, 256), recorder(o2, a, 64)
    for f in range(max(len(fa1), len(fb1))):                   # two recorders interleaved on one handle
        if f < len(fa1):
            ra1.record(*fa1[f])
        if f < len(fb1):
            rb1.record(*fb1[f])
    feed(ra2, fa2, 0, len(fa2))                                # the same frames on a fresh handle, alone
    alone = recorder(o2, b, 256)
    feed(alone, frames_on(o2, b), 0, len(fb1))
    torch.cuda.synchronize()
    assert torch.equal(ra1._acc.cpu(), ra2._acc.cpu()) and torch.equal(rb1._acc.cpu(), alone._acc.cpu())
    assert torch.equal(ra1._ring.cpu(), ra2._ring.cpu()) and torch.equal(ra1._unwrapped.cpu(), ra2._unwrapped.cpu())
    check('types_gap', prec, ra1, len(fa1), 'interleaved')
    check('lags_7', prec, rb1, len(fb1), 'interleaved')
    # a non-default torch stream
    s = torch.cuda.Stream()
    again = recorder(o1, a, 64)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        feed(again, fa1, 0, len(fa1))
    s.synchronize()
    assert torch.equal(again._acc.cpu(), ra1._acc.cpu())


# ---- 3. wrapped and unwrapped ----------------------------------------------------------------------------------------------------------------
def test_wrapped_and_unwrapped_meet_the_same_reference(prec):
    o = owner()
    got = {}
    for name in ('wrapped_triclinic', 'unwrapped_triclinic'):
        c = R.case(name)
        rec = recorder(o, c)
        fr = frames_on(o, c)
        feed(rec, fr, 0, len(fr))
        check(name, prec, rec, len(fr), 'against the unwrapped reference', ref_name='unwrapped_triclinic',
              other_input=name.startswith('wrapped'))
        got[name] = rec.info()['large_jumps']
    if prec == 'double':
        assert got == {'wrapped_triclinic': 0, 'unwrapped_triclinic': 0}
    assert R.case('wrapped_triclinic')['crossings'] >= 10


# ---- 4. accumulation and reset -------------------------------------------------------------------------------------------------------------
def test_accumulators_are_added_to_and_reset_starts_over(prec):
    import torch
    c = R.case('npt')
    o = owner()
    fr = frames_on(o, c)
    rec = recorder(o, c, 64)
    feed(rec, fr, 0, len(fr))
    first = rec._acc.clone()
    ring = rec._ring.clone()
    assert rec.frames == len(fr) and first.abs().sum() > 0
    # pre-filled accumulators: every record adds; each of the `frames` additions rounds relative to the word it writes
    filled = recorder(o, c, 64)
    pre = torch.linspace(-3.0, 5.0, filled._acc.numel(), dtype=torch.float64, device=o._device)
    filled._acc.copy_(pre)
    feed(filled, fr, 0, len(fr))
    ref = ref_of('npt', prec)
    got = (filled._acc - pre).cpu().numpy().reshape(2, c['n_types'], c['n_lags'])
    slack = (len(fr) + 1) * R.U * (np.abs(pre.cpu().numpy()).max() + np.abs(np.stack([ref['msd'], ref['vacf_abs']])))
    err = np.abs(got - np.stack([ref['msd'], ref['vacf']]))
    assert (err <= R.bar(ref, prec) + slack).all()
    assert (filled._acc != pre).any()
    # reset: frames 0, accumulators and jump word zero, and the next record re-initialises the state: the second run equals the first
    rec._jumps.fill_(7)
    rec.reset()
    assert rec.frames == 0 and rec._acc.abs().sum().item() == 0 and rec.info()['large_jumps'] == 0
    assert rec.sums()['origins'].sum() == 0
    feed(rec, fr, 0, len(fr))
    torch.cuda.synchronize()
    assert torch.equal(rec._acc, first) and torch.equal(rec._ring, ring)
    check('npt', prec, rec, len(fr), 'after reset')


# ---- 5. the jump counter ----------------------------------------------------------------------------------------------------------------------
def test_jump_counter_equals_the_reference(prec):
    c = R.case('jumps')
    o = owner()
    rec = recorder(o, c)
    fr = frames_on(o, c)
    feed(rec, fr, 0, 4)
    assert rec.info()['large_jumps'] == 0
    feed(rec, fr, 4, len(fr))
    assert rec.info()['large_jumps'] == ref_of('jumps', prec)['jumps'] == 5
    check('jumps', prec, rec, len(fr))                           # the jumps are applied all the same


# ---- 6. the contract ----------------------------------------------------------------------------------------------------------------------------
def test_contract(prec):
    import torch
    from admp_amd import _lib
    c = R.case('types_gap')
    o = owner()
    L, h = o._L, o._h
    fr = frames_on(o, c)
    rec = recorder(o, c, 64)
    feed(rec, fr, 0, 3)
    info = (ctypes.c_int64 * 4)()
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    pos, vel, box = fr[3][0], fr[3][1], _lib.darr(fr[3][2])
    good = [rec.n_atoms, P(pos), P(vel), box, rec.n_slots, P(rec._slot_atom), rec.n_tiles, P(rec._tile_type), 64, rec.n_types, rec.n_lags,
            3, P(rec._ring), P(rec._unwrapped), P(rec._last), P(rec._jumps), P(rec._acc), info]
    owned = ('_ring', '_unwrapped', '_last', '_jumps', '_acc')
    torch.cuda.synchronize()
    before = {k: getattr(rec, k).clone() for k in owned}
    o._use_current_stream()

    def unchanged():
        torch.cuda.synchronize()
        return all(torch.equal(getattr(rec, k), before[k]) for k in owned)

    def refused(k, value, code=E_ARG, handle=h):
        a = list(good)
        a[k] = value
        for i in range(4):
            info[i] = -7
        assert L.admp_md_tcf(handle, *a) == code, (k, value)
        assert L.admp_last_error(handle)
        assert unchanged(), (k, value)

    for k in (3, 16, 12, 13, 14, 15):                       # box, accumulator, ring, state, jump word
        refused(k, None)
    for k in (1, 2, 5, 7):                                  # positions, velocities, tables
        refused(k, None)
    for k in (0, 4, 6):                                     # negative counts
        refused(k, -1)
    refused(4, rec.n_slots - 1)                             # n_slots != n_tiles * tile_atoms
    refused(6, rec.n_tiles + 1)
    for v in (0, 32, 63, 100, 1088, -64):
        refused(8, v)
    for v in (0, 9, -1):
        refused(9, v)
    for v in (0, -1):
        refused(10, v)
    refused(11, -1)
    b3 = np.asarray(fr[3][2])
    for bad in (np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]]), np.zeros((3, 3)), b3 + np.diag([0.0, np.nan, 0.0]),
                b3 + np.diag([0.0, np.inf, 0.0])):
        refused(3, _lib.darr(bad))
    # a slab-decomposed handle: ADMP_E_STATE, before any other argument
    slab = owner()
    _lib.check(slab._h, L.admp_slab_configure(slab._h, 0, 2), 'admp_slab_configure')
    slab._use_current_stream()
    refused(0, rec.n_atoms, code=E_STATE, handle=slab._h)
    assert b'single-rank' in L.admp_last_error(slab._h)
    refused(12, None, code=E_STATE, handle=slab._h)
    with pytest.raises(_lib.AdmpHipError, match='single-rank'):
        recorder(slab, c, 64).record(*fr[0])
    # no slots: nothing launched, NULL positions, velocities and tables pass, info says so
    a = list(good)
    a[1] = a[2] = a[5] = a[7] = None
    a[4] = a[6] = 0
    assert L.admp_md_tcf(h, *a) == 0 and list(info) == [0, R.LAGS_PER_WORKGROUP, 0, 0] and unchanged()
    from admp_amd.md import CorrelationRecorder
    empty = CorrelationRecorder(o, np.array([-1, -1, -4]), 4, 1.0)
    empty.record(dev(o, np.zeros((3, 3))), dev(o, np.ones((3, 3))), b3)
    assert empty.frames == 1 and empty.info()['workgroups'] == 0 and empty.sums()['vacf'].sum() == 0 and unchanged()
    # device contents are not trusted: out-of-range entries count nothing and touch nothing
    n_slots, n_tiles = rec.n_slots, rec.n_tiles
    wild_slots = torch.tensor([rec.n_atoms, -1, 2 ** 31 - 1, -2 ** 31] * (n_slots // 4), dtype=torch.int32, device=o._device)
    a = list(good)
    a[5] = P(wild_slots)
    assert L.admp_md_tcf(h, *a) == 0 and unchanged()
    wild_tiles = torch.tensor(([rec.n_types, -1, 8, 2 ** 31 - 1, -2 ** 31, 15] * n_tiles)[:n_tiles], dtype=torch.int32, device=o._device)
    a = list(good)
    a[7] = P(wild_tiles)
    acc0 = rec._acc.clone()
    assert L.admp_md_tcf(h, *a) == 0                        # (the push runs: the slots are valid; nothing is counted)
    torch.cuda.synchronize()
    assert torch.equal(rec._acc, acc0)
    # ... after which the valid call of frame 3 repeats the push with the same values, and the run goes on to the reference
    assert L.admp_md_tcf(h, *good) == 0 and list(info)[0] == n_tiles and list(info)[2] == 4
    rec.frames = 4
    feed(rec, fr, 4, len(fr))
    check('types_gap', prec, rec, len(fr), 'after the refusals')
    # Python: the library reads raw pointers
    other = torch.float32 if o._dtype == torch.float64 else torch.float64
    for bad in (pos.to(other), pos[:-1], pos.cpu(), torch.stack([pos, pos], dim=1)[:, 0], c['pos'][0]):
        with pytest.raises(ValueError):
            rec.record(bad, vel, b3)
        with pytest.raises(ValueError):
            rec.record(pos, bad, b3)
    with pytest.raises(ValueError, match='admp_md_tcf'):
        rec.record(pos, vel, np.zeros((3, 3)))              # the library's refusal of the box
    with pytest.raises(ValueError, match='bytes'):
        CorrelationRecorder(o, c['types'], 4096, 1.0, max_ring_bytes=10 ** 6)
    assert rec.frames == len(fr)


# ---- 7. a driver end to end ---------------------------------------------------------------------------------------------------------------------
def test_nvt_driver_reports_the_msd(tmp_path):
    """64 waters, 40 steps, a frame every 2 steps into 8 lags: the closing lines parse, the file has 8 rows"""
    path = str(tmp_path / 'msd.txt')
    out = run_driver('nvt_water.py', '--waters', '64', '--steps', '40', '--msd', '2', '--msd-lags', '8', '--msd-out', path)
    m = re.search(r'# msd over (\d+) frames every ([0-9.]+) fs: (\d+) lags, (\d+) workgroups, large_jumps (\d+)', out)
    assert m, out[-1500:]
    print(m.group(0))
    assert int(m.group(1)) == 20 and abs(float(m.group(2)) - 1.0) < 1e-9 and int(m.group(3)) == 8 and int(m.group(5)) == 0
    m = re.search(r'# D_O: Einstein ([-+0-9.e]+) \(fit over ([0-9.]+)\.\.([0-9.]+) fs\), Green-Kubo ([-+0-9.e]+), in 1e-5 cm\^2/s', out)
    assert m, out[-1500:]
    print(m.group(0))
    assert np.isfinite(float(m.group(1))) and np.isfinite(float(m.group(4))) and float(m.group(2)) == 4.0 and float(m.group(3)) == 7.0
    rows = np.loadtxt(path)
    assert rows.shape == (8, 5) and np.allclose(rows[:, 0], np.arange(8.0))
    assert rows[0, 1] == 0 and rows[0, 2] == 0 and rows[0, 3] > 0 and rows[0, 4] > 0      # msd_O[0] = 0, vacf_O[0] > 0
    assert (rows[1:, 1] > 0).all() and (rows[1:, 2] > 0).all()
