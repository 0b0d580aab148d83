"""The arithmetic and the plan of the time correlation functions on the host (admp_amd/csrc/tcf_math.h, tcf_plan.h: the text the
kernels of tcf_kernels.hip compile; tests/tcf_shim/main.cpp) against the float64 reference of tests/tcf_ref.py, whose docstring
derives the acceptance bar, and the pure-numpy layout, normalisation and reductions of admp_amd.md.  -s prints err / bar of the host
restatement for every case: it must stay <= 1, or the error model is wrong."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import tcf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ROOT + '/admp_amd/csrc'
SHIM = ROOT + '/tests/tcf_shim/main.cpp'


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the headers cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('tcf_shim') / 'tcf_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I', CSRC, '-o', exe, SHIM])
    return exe


def run(shim, *args, text=None):
    return subprocess.run([shim, *[str(a) for a in args]], input=text, capture_output=True, text=True, check=True).stdout


_REF = {}


def ref_of(name, prec, frames=None):
    """the reference of the first `frames` frames of a case as a handle of that precision holds them; computed once"""
    key = (name, prec, frames)
    if key not in _REF:
        c = R.case(name)
        _REF[key] = R.reference(c, *R.held(c, prec, frames))
    return _REF[key]


def shim_sums(shim, c, prec, tile_atoms, frames=None, pos=None):
    from admp_amd.md import tcf_layout
    slot_atom, tile_type, n_types, _ = tcf_layout(c['types'], tile_atoms)
    p, v = R.held(c, prec, frames)
    p = p if pos is None else pos
    nt = c['n_types']
    lines = ['%d %d %d %d %d %d' % (len(c['types']), nt, c['n_lags'], tile_atoms, len(tile_type), len(p)),
             ' '.join(str(x) for x in slot_atom), ' '.join(str(x) for x in tile_type)]
    for f in range(len(p)):
        lines.append(' '.join('%.17g' % x for x in c['box'][f].reshape(-1)))
        lines += ['%.17g %.17g %.17g %.17g %.17g %.17g' % (*a, *b) for a, b in zip(p[f], v[f])]
    out = run(shim, prec, 'sums', text='\n'.join(lines) + '\n').split()
    acc = np.array(out[:-1], dtype=np.float64).reshape(2, nt, c['n_lags'])
    return acc[0], acc[1], int(out[-1])


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile_atoms', [64, 256, 320])
def test_layout_against_a_restatement(tile_atoms):
    from admp_amd.md import tcf_layout
    for name in ('n1', 'n255', 'n256', 'n257', 'types_gap', 'wrapped_triclinic'):
        types = R.case(name)['types']
        slot_atom, tile_type, n_types, counts = tcf_layout(types, tile_atoms)
        want_slots, want_tiles = R.layout(types, tile_atoms)
        assert slot_atom.dtype == np.int32 and tile_type.dtype == np.int32
        assert np.array_equal(slot_atom, want_slots) and np.array_equal(tile_type, want_tiles)      # every padding slot included
        assert len(slot_atom) == len(tile_type) * tile_atoms
        assert counts.tolist() == [int((types == a).sum()) for a in range(n_types)]
    # an empty type has no tile and no slot; the sort is stable
    slot_atom, tile_type, n_types, counts = tcf_layout(R.case('types_gap')['types'], 64)
    assert n_types == 3 and counts.tolist() == [1, 0, 300] and tile_type.tolist() == [0, 2, 2, 2, 2, 2]
    assert (slot_atom[1:64] == -1).all() and (np.diff(slot_atom[64:364]) > 0).all() and (slot_atom[364:] == -1).all()
    # nothing counted, nothing at all
    for types in (np.array([-1, -2]), np.zeros(0, dtype=int)):
        slot_atom, tile_type, n_types, counts = tcf_layout(types, 256)
        assert len(slot_atom) == 0 and len(tile_type) == 0 and n_types == 1 and counts.tolist() == [0]
    for bad in (32, 100, 1088, 2.5):
        with pytest.raises(ValueError):
            tcf_layout([0, 1], bad)
    for bad in ([8], [0.5], [[0, 1]]):
        with pytest.raises(ValueError):
            tcf_layout(bad)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def test_ring_slots_and_lags_reached(shim):
    for L in (1, 4, 7, 33):
        rows = np.array(run(shim, 'slots', 2 * L + 3, L).split(), dtype=np.int64).reshape(-1, 3)
        want = [(f, k, (f - k) % L) for f in range(2 * L + 3) for k in range(min(f, L - 1) + 1)]
        assert rows.tolist() == [list(w) for w in want]
        # the slot a frame is written to is the slot of the oldest frame the ring still holds: lag L would read the new frame
        assert all((f - L) % L == f % L for f in range(L, 2 * L + 3))


@pytest.mark.parametrize('tile_atoms', [64, 192, 256, 320, 512, 1024])
def test_plan_against_the_rule(shim, tile_atoms):
    for n_tiles, L, frame in ((1, 1, 0), (3, 7, 3), (3, 7, 100), (5, 33, 32), (2, 65, 31), (384, 512, 10 ** 12)):
        out = run(shim, 'plan', 1000, n_tiles * tile_atoms, n_tiles, tile_atoms, 2, L, frame).split()
        assert out[0] == 'ok', out
        threads, spl, lags_now, blocks, wgs, slot, scratch = (int(x) for x in out[1:])
        assert threads == min(256, tile_atoms) and spl == -(-tile_atoms // 256) and threads * spl >= tile_atoms
        assert lags_now == min(frame, L - 1) + 1 and blocks == -(-lags_now // R.LAGS_PER_WORKGROUP)
        assert wgs == n_tiles * blocks and slot == frame % L and scratch == 2 * n_tiles * L * 8


def test_plan_refusals(shim):
    good = [100, 512, 2, 256, 2, 8, 0]

    def refused(k, v, text):
        a = list(good)
        a[k] = v
        out = run(shim, 'plan', *a)
        assert out.startswith('error') and text in out, (k, v, out)

    assert run(shim, 'plan', *good).startswith('ok')
    refused(0, -1, 'negative')
    refused(1, -512, 'negative')
    refused(2, -2, 'negative')
    refused(1, 511, 'n_tiles * tile_atoms')
    refused(2, 3, 'n_tiles * tile_atoms')
    for v in (0, 32, 100, 257, 1088):
        refused(3, v, 'multiple of 64')
    for v in (0, 9, -1):
        refused(4, v, '1..8')
    for v in (0, -3):
        refused(5, v, 'n_lags')
    refused(6, -1, 'frame')
    assert run(shim, 'plan', 0, 0, 0, 256, 1, 4, 0).split()[5] == '0'      # no slots: no workgroups


# ---- the cases are what they claim ------------------------------------------------------------------------------------------------------
def test_the_cases_are_what_they_claim():
    for name in R.CASES:
        c = R.case(name)
        assert len(c['types']) <= 700 and len(c['pos']) <= 140
    assert R.case('wrapped_triclinic')['crossings'] >= 10
    w, u = R.case('wrapped_triclinic'), R.case('unwrapped_triclinic')
    s = w['pos'] @ np.linalg.inv(R.SKEW)
    assert s.min() >= -1e-12 and s.max() <= 1 + 1e-12 and np.abs(w['pos'] - u['pos']).max() > 5.0
    shift = (w['pos'] - u['pos']) @ np.linalg.inv(R.SKEW)
    assert np.abs(shift - np.round(shift)).max() < 1e-12                       # the same trajectory up to lattice vectors
    for L in (1, 7, 33, 65):
        assert L % R.LAGS_PER_WORKGROUP != 0 and R.LAGS_PER_WORKGROUP % L != 0 or L == 1
    c = R.case('npt')
    assert np.allclose(c['box'][5], c['box'][0] * 1.001 ** 5, rtol=1e-14)
    c = R.case('types_gap')
    assert [(c['types'] == a).sum() for a in range(3)] == [1, 0, 300] and (c['types'] < 0).sum() == 40
    assert (np.diff(np.nonzero(c['types'] == 2)[0]) > 1).any()


def test_jump_margins_and_count():
    c = R.case('jumps')
    for prec in 'df':
        pos, vel = R.held(c, prec)
        _, jump, frac = R.unwrap(pos, c['box'])
        assert np.abs(np.abs(frac) - 0.25).min() >= 1e-3                       # no component near the threshold
        assert jump.sum() == 5 and jump[4, :5].all() and ref_of('jumps', prec)['jumps'] == 5
        big = np.abs(frac[4, :5]).max(axis=1)
        assert np.allclose(np.sort(big), [0.3, 0.3, 0.3, 0.4, 0.4], atol=0.05) and np.abs(frac[:, 5:]).max() < 0.1
    for name in R.CASES:
        if name != 'jumps':
            assert ref_of(name, 'd')['jumps'] == 0


def test_ballistic_values_check_the_reference():
    """constant velocities: MSD[k] = <v^2> (k dt)^2 and VACF[k] = <v^2>, whatever the cell: the analytic sums against the reference,
    within the bar for another input (the positions p0 + v f dt are rounded once each)"""
    c = R.case('ballistic')
    s = c['pos'] @ np.linalg.inv(c['box'][0])
    assert ((s < 0) | (s > 1)).any(axis=(0, 2)).sum() >= 3                     # atoms leave the cell
    ref = ref_of('ballistic', 'd')
    v2 = (c['vel'][0] ** 2).sum()
    k = np.arange(c['n_lags'])
    msd = ref['origins'] * v2 * (k * c['dt']) ** 2
    vacf = ref['origins'] * v2 * np.ones(len(k))
    ratio = R.worst_ratio(ref, 'd', msd[None], vacf[None], other_input=True)
    print('ballistic: analytic against the reference, err / bar = %.3g' % ratio)
    assert ratio <= 1.0
    assert abs(ref['msd'][0, 3] / (ref['origins'][3] * v2 * 36.0) - 1.0) < 1e-9   # (and not only within a loose bar)


# ---- the host restatement against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['d', 'f'])
@pytest.mark.parametrize('name', R.CASES)
def test_shim_sums_within_the_bar(shim, name, prec):
    c = R.case(name)
    for tile_atoms in (64, 256):
        for frames in R.checkpoints(c):
            ref = ref_of(name, prec, frames)
            msd, vacf, jumps = shim_sums(shim, c, prec, tile_atoms, frames)
            ratio = R.worst_ratio(ref, prec, msd, vacf)
            print('%s %s tile %d, %d frames: err / bar = %.3g, jumps %d' % (name, prec, tile_atoms, frames, ratio, jumps))
            assert ratio <= 1.0
            assert jumps == ref['jumps']
            assert (msd[:, 0] == 0).all() and (msd[:, frames:] == 0).all() and (vacf[:, frames:] == 0).all()


@pytest.mark.parametrize('prec', ['d', 'f'])
@pytest.mark.parametrize('tile_atoms', [320, 512, 768, 1024])
def test_shim_sums_with_several_slots_per_lane(shim, prec, tile_atoms):
    for name in ('types_gap', 'n257'):
        c = R.case(name)
        msd, vacf, jumps = shim_sums(shim, c, prec, tile_atoms)
        ratio = R.worst_ratio(ref_of(name, prec, len(c['pos'])), prec, msd, vacf)
        print('%s %s tile %d: err / bar = %.3g' % (name, prec, tile_atoms, ratio))
        assert ratio <= 1.0 and jumps == 0


@pytest.mark.parametrize('prec', ['d', 'f'])
def test_wrapped_and_unwrapped_meet_the_same_reference(shim, prec):
    w = R.case('wrapped_triclinic')
    ref = ref_of('unwrapped_triclinic', prec)
    msd, vacf, jumps = shim_sums(shim, w, prec, 256)
    ratio = R.worst_ratio(ref, prec, msd, vacf, other_input=True)
    print('wrapped against the unwrapped reference, %s: err / bar = %.3g' % (prec, ratio))
    assert ratio <= 1.0 and jumps == 0


# ---- normalisation and reductions ------------------------------------------------------------------------------------------------------
def test_normalise():
    from admp_amd.md import tcf_normalise
    rng = np.random.default_rng(0)
    sums = {'msd': rng.random((3, 5)), 'vacf': rng.normal(size=(3, 5)), 'origins': np.array([7, 6, 5, 0, 0])}
    t, msd, vacf = tcf_normalise(sums, [4, 0, 10], 2.5)
    assert np.array_equal(t, 2.5 * np.arange(5))
    assert np.allclose(msd[0][:3], sums['msd'][0, :3] / (4 * np.array([7, 6, 5])), rtol=1e-15) and (msd[0][3:] == 0).all()
    assert (msd[1] == 0).all() and (vacf[1] == 0).all()
    assert np.allclose(vacf[2][:3], sums['vacf'][2, :3] / (10 * np.array([7, 6, 5])), rtol=1e-15) and (vacf[2][3:] == 0).all()
    with pytest.raises(ValueError):
        tcf_normalise(sums, [4, 10], 2.5)


def test_diffusion_einstein_is_exact_on_a_line():
    from admp_amd.md import DIFFUSION_1E5_CM2_S, diffusion_einstein
    t = 2.0 * np.arange(64)
    D, c = 2.3e-4, 0.37
    got = diffusion_einstein(t, 6.0 * D * t + c, t[32], t[-1])
    assert abs(got / D - 1.0) < 1e-12
    assert DIFFUSION_1E5_CM2_S == 1e4                                          # 1 A^2/fs = 0.1 cm^2/s
    with pytest.raises(ValueError):
        diffusion_einstein(t, t, 5.0, 5.5)


def test_diffusion_green_kubo_on_an_exponential():
    """vacf = <v^2> exp(-t / tau): the integral to T is <v^2> tau (1 - exp(-T / tau)); the composite trapezoid rule with step h is
    off by at most (T / 12) h^2 max |f''| = (T / 12) h^2 <v^2> / tau^2"""
    from admp_amd.md import diffusion_green_kubo
    v2, tau, h, n = 3.0e-4, 40.0, 2.0, 200
    t = h * np.arange(n)
    T = t[-1]
    D, running = diffusion_green_kubo(t, v2 * np.exp(-t / tau))
    exact = v2 * tau * (1.0 - np.exp(-T / tau)) / 3.0
    bound = T / 12.0 * h * h * v2 / tau ** 2 / 3.0
    print('Green-Kubo: error %.3g, trapezoid bound %.3g' % (abs(D - exact), bound))
    assert abs(D - exact) <= bound and D == running[-1] and running[0] == 0.0 and len(running) == n
    D_half, _ = diffusion_green_kubo(t, v2 * np.exp(-t / tau), t_max=t[100])
    assert D_half == running[100]


def test_vdos_peaks_where_the_cosine_is():
    from admp_amd.md import LIGHT_CM_PER_FS, vdos
    L, dt = 512, 1.0
    t = dt * np.arange(L)
    for wavenumber in (3400.0, 1650.0, 620.0):
        nu = wavenumber * LIGHT_CM_PER_FS                                      # 1/fs
        for window in ('hann', None):
            w, S = vdos(t, 0.7 * np.cos(2.0 * np.pi * nu * t), window=window)
            width = w[1] - w[0]
            assert abs(width - 1.0 / (2 * L * dt) / LIGHT_CM_PER_FS) < 1e-9 * width and len(w) == L
            assert abs(w[int(np.argmax(S))] - wavenumber) <= 0.5 * width       # the bin that holds the frequency
    with pytest.raises(ValueError):
        vdos(t, np.zeros(L))


def test_max_ring_bytes_raises():
    """the constructor computes the ring's size before it allocates anything: a stand-in owner without a device serves"""
    import types as _types

    import torch
    from admp_amd.md import CorrelationRecorder
    owner = _types.SimpleNamespace(_dtype=torch.float32, _device=torch.device('cpu'))
    with pytest.raises(ValueError, match=r'%d bytes' % (512 * 6 * 1024 * 4)):
        CorrelationRecorder(owner, np.zeros(1000, dtype=int), 512, 2.0, max_ring_bytes=512 * 6 * 1024 * 4 - 1)
    owner._dtype = torch.float64
    with pytest.raises(ValueError, match=r'%d bytes' % (4096 * 6 * 98304 * 8)):
        CorrelationRecorder(owner, np.tile([0, 1, 1], 32768), 4096, 2.0)      # 18 GiB against the default 2 GiB
    for bad in (0, 2.5, -1):
        with pytest.raises(ValueError):
            CorrelationRecorder(owner, [0], bad, 2.0)
    with pytest.raises(ValueError):
        CorrelationRecorder(owner, [0], 4, 0.0)
