"""The control rule of the FIRE minimiser (admp_amd/csrc/md_fire_math.h) without a GPU: the header, compiled by the host compiler
into a stand-alone program (tests/fire_shim/main.cpp), against the numpy restatement of tests/fire_ref.py on a table of cases
that takes every branch; the restatement's step length against the cap it promises; and the restatement alone on the harmonic
well that tests/test_gpu_md_fire.py gives to the kernels."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import fire_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, 'tests', 'fire_shim', 'main.cpp')
CSRC = os.path.join(ROOT, 'admp_amd', 'csrc')
EPS = float(np.finfo(np.float64).eps)

P = R.DEFAULTS
#          dt    alpha n_pos dtv_last fmax iter uphill flags
MID = (1.3, 0.21, 7.0, 0.9, 3.0, 41.0, 5.0, 0.0)
LATE = (1.3, 0.21, 20.0, 0.9, 3.0, 41.0, 5.0, 0.0)
# name: (state, (Fv, FF, vv, vmax, fmax, amax), params, ftol, what the restatement must show for the case to be the one named)
CASES = {
    'downhill before the delay': (MID, (2.0, 50.0, 1e-4, 2e-3, 4.0, 1e-6), P, 0.0,
                                  lambda s, c: s[R.NPOS] == 8 and s[R.DT] == 1.3 and s[R.ALPHA] == 0.21 and c[3] == 1.3),
    'downhill after the delay': (LATE, (2.0, 50.0, 1e-4, 2e-3, 4.0, 1e-6), P, 0.0,
                                 lambda s, c: s[R.NPOS] == 21 and s[R.DT] == 1.3 * 1.1 and s[R.ALPHA] == 0.21 * 0.99 and c[0] == 1.0 - 0.21),
    'dt clipped at dt_max': ((4.8,) + LATE[1:], (2.0, 50.0, 1e-4, 2e-3, 4.0, 1e-6), P, 0.0,
                             lambda s, c: s[R.DT] == 5.0 and c[3] == 5.0),
    'uphill with shrink': (MID, (-2.0, 50.0, 1e-4, 2e-3, 4.0, 1e-6), P, 0.0,
                           lambda s, c: s[R.DT] == 0.65 and s[R.NPOS] == 0 and s[R.UPHILL] == 6 and c[:3] == (0.0, 0.0, 0.45)
                           and s[R.ALPHA] == 0.25),
    'uphill at dt_min': ((0.015,) + MID[1:], (-2.0, 50.0, 1e-4, 2e-3, 4.0, 1e-6), P, 0.0,
                         lambda s, c: s[R.DT] == 0.015 and s[R.UPHILL] == 6),
    'uphill on zero Fv': (MID, (0.0, 50.0, 0.0, 0.0, 4.0, 1e-6), P, 0.0, lambda s, c: s[R.UPHILL] == 6 and c[0] == 0.0),
    'cap binding with vb = 0': (MID, (-2.0, 5e13, 1e-4, 2e-3, 4e6, 4e2), P, 0.0,
                                lambda s, c: c[3] < 0.65 and abs(c[3] ** 2 * 4e2 / 0.1 - 1.0) < 1e-14),
    'cap binding with vb > 0': (MID, (2.0, 50.0, 4.0, 1.5, 4.0, 1e-2), P, 0.0,
                                lambda s, c: c[3] < 1.3 and s[R.DTV_LAST] == c[3]),
    'FF = 0': (MID, (0.0, 0.0, 1e-4, 2e-3, 0.0, 0.0), P, 0.0, lambda s, c: s[R.FLAGS] == R.DONE and s[R.FMAX] == 0.0),
    'FF underflown, downhill': (MID, (1e-300, 0.0, 1e-4, 2e-3, 1e-170, 1e-174), P, 0.0, lambda s, c: c[1] == 0.0 and c[0] == 1.0 - 0.21),
    'fmax <= ftol': (MID, (2.0, 50.0, 1e-4, 2e-3, 4.0, 1e-6), P, 4.0,
                     lambda s, c: s[R.FLAGS] == R.DONE and s[R.ITER] == 41 and s[R.FMAX] == 4.0 and c == (0.0,) * 4),
    'done before, larger force now': (MID[:7] + (R.DONE,), (2.0, 50.0, 1e-4, 2e-3, 4.0, 1e-6), P, 3.0,
                                      lambda s, c: s[R.FLAGS] == 0.0 and s[R.ITER] == 42),
    'a NaN word': (MID, (2.0, float('nan'), 1e-4, 2e-3, 4.0, 1e-6), P, 0.0,
                   lambda s, c: s[R.FLAGS] == R.FAILED and s[R.ITER] == 41 and c == (0.0,) * 4),
    'an infinite word': (MID, (2.0, 50.0, 1e-4, 2e-3, float('inf'), 1e-6), P, 0.0, lambda s, c: s[R.FLAGS] == R.FAILED),
    'failed before, clean words now': (MID[:7] + (R.FAILED,), (2.0, 50.0, 1e-4, 2e-3, 4.0, 1e-6), P, 0.0,
                                       lambda s, c: s[R.FLAGS] == R.FAILED and s[R.ITER] == 41 and s[R.FMAX] == 3.0),
    'fresh state, first call': (tuple(R.fresh_state()), (0.0, 50.0, 0.0, 0.0, 4.0, 1e-6), P, 0.0,
                                lambda s, c: s[R.DT] == 0.25 and c[2] == 0.0 and c[3] == 0.25),
    'no force on a massive atom, at rest': (MID, (-1e-30, 1e-20, 0.0, 0.0, 1e-10, 0.0), P, 0.0, lambda s, c: c[3] == 0.65),
    'other parameters': (MID[:2] + (3.0,) + MID[3:], (2.0, 50.0, 1e-4, 2e-3, 4.0, 1e-6), (0.5, 2.0, 0.1, 0.05, 2.0, 1.7, 0.3, 0.1, 0.5),
                         0.0, lambda s, c: s[R.DT] == 2.0 and s[R.ALPHA] == 0.105),
}


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the header cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('fire_shim') / 'fire_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, '-o', exe, SHIM])
    return exe


@pytest.mark.parametrize('name', list(CASES))
def test_restatement_takes_the_branch_the_case_names(name):
    state, sums, par, ftol, shows = CASES[name]
    out, coef, moves = R.control(state, sums, par, ftol)
    assert shows(out, tuple(coef)), (out, coef)
    assert moves == (out[R.ITER] == state[R.ITER] + 1)


@pytest.mark.parametrize('name', list(CASES))
def test_header_agrees_with_the_restatement(shim, name):
    """1e-14 relative on every word of the new state and every coefficient (the same few operations in the same order: the two
    differ by the compiler's contraction of a product into a sum at the most)"""
    state, sums, par, ftol, _ = CASES[name]
    out, coef, moves = R.control(state, sums, par, ftol)
    args = ['%.17g' % x for x in tuple(state) + tuple(sums) + tuple(par) + (ftol,)]
    got = [float(x) for x in subprocess.run([shim] + args, capture_output=True, text=True, check=True).stdout.split()]
    assert len(got) == 13
    assert int(got[0]) == int(moves)
    want = np.concatenate([out, coef])
    err = np.abs(np.array(got[1:]) - want)
    assert np.all(err <= 1e-14 * np.abs(want)), (got, want)


def test_closed_form_step_respects_the_cap():
    """dtv vb + dtv^2 amax <= max_step (1 + 4 eps) over twelve decades of vb and amax, downhill (vb > 0) and uphill (vb = 0),
    and dtv = dt exactly where the cap does not bind"""
    rng = np.random.default_rng(3)
    bound = 0
    for _ in range(4000):
        vmax, fmax = 10.0 ** rng.uniform(-6, 6, size=2)
        amax = fmax * 10.0 ** rng.uniform(-6, 0)
        downhill = rng.random() < 0.5
        vv, FF = vmax * vmax * rng.uniform(1, 50), fmax * fmax * rng.uniform(1, 50)
        Fv = (1.0 if downhill else -1.0) * 0.3 * np.sqrt(vv * FF)
        state = (10.0 ** rng.uniform(-2, 0.69), 0.2, 3.0, 0.5, 1.0, 9.0, 1.0, 0.0)
        out, (a, b, _, dtv), moves = R.control(state, (Fv, FF, vv, vmax, fmax, amax), P, 0.0)
        assert moves
        vb = a * vmax + b * fmax
        assert (vb > 0) == downhill
        assert dtv * vb + dtv * dtv * amax <= P[3] * (1.0 + 4.0 * EPS)
        assert 0.0 < dtv <= out[R.DT]
        if dtv < out[R.DT]:
            bound += 1
            assert dtv * vb + dtv * dtv * amax >= P[3] * (1.0 - 16.0 * EPS)      # the LARGEST such step, to rounding
    assert 400 < bound < 3600      # both regimes were visited


@pytest.mark.parametrize('unit_masses', [False, True])
def test_restatement_converges_on_the_harmonic_well(unit_masses):
    """n = 1000, ftol 1e-8: done within the 1000 iterations the GPU test allows, |x - x0| <= ftol / k_min at the end"""
    x0, k, masses, x = R.harmonic_well(1000, unit_masses)
    v, state, ftol = np.zeros_like(x), R.fresh_state(), 1e-8
    for it in range(1000):
        x, v, state = R.step(x, v, k * (x - x0), 1.0 / masses, state, ftol=ftol)
        if state[R.FLAGS] == R.DONE:
            break
    print('done after %d iterations (%d uphill), fmax %.2e' % (state[R.ITER], state[R.UPHILL], state[R.FMAX]))
    assert state[R.FLAGS] == R.DONE
    assert np.sqrt(((x - x0) ** 2).sum(1)).max() <= ftol / k.min()
