"""The rule of the stochastic velocity-rescaling thermostat (admp_amd/csrc/md_vrescale_math.h) without a GPU: the header, compiled
by the host compiler into a stand-alone program (tests/vrescale_shim/main.cpp), against the numpy restatement of
tests/vrescale_ref.py on a table of cases that takes every branch; the restatement's noise against the chi-square distribution it
promises; and the restatement's chain of kinetic energies against the canonical mean and variance."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import vrescale_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, 'tests', 'vrescale_shim', 'main.cpp')
CSRC = os.path.join(ROOT, 'admp_amd', 'csrc')

KT = R.KB * 300.0 * R.ACC
SEED = 12345
NFS = (1, 2, 3, 4, 7, 300, 1943, 3145725)
FRESH = tuple(R.fresh_state())
#        K_before K_after alpha heat  applications tries reserved flags
USED = (3.1e-3, 2.9e-3, 0.97, -4.0e-3, 17.0, 2.0, 0.0, 0.0)
WAS_FAILED = USED[:7] + (R.FAILED,)


def _k(nf, x=1.3):
    return x * nf * 0.5 * KT


# name: (prec, state, K, n_dof, kT_acc, c, seed, step, what the restatement must show for the case to be the one named)
CASES = {}
for _nf in (1, 2, 3, 4, 7, 1943, 3145725):
    for _c in (0.0, 0.7, 1.0):
        CASES['Nf %d, c %g' % (_nf, _c)] = (
            8, USED, _k(_nf), _nf, KT, _c, SEED, 5,
            (lambda s, a, ok, c=_c, nf=_nf: ok and s[R.APPLICATIONS] == 18 and (a == 1.0 and s[R.TRIES] == 0 and s[R.K_AFTER] == s[R.K_BEFORE]
                                                                              if c == 1.0 else a != 1.0 and (s[R.TRIES] >= 1) == (nf >= 3))))
CASES.update({
    'single precision rounds alpha before K_after': (
        4, USED, _k(7), 7, KT, 0.7, SEED, 5,
        lambda s, a, ok: ok and s[R.ALPHA] == a and float(np.float32(a)) != a and s[R.K_AFTER] == float(np.float32(a)) ** 2 * _k(7)),
    'K = 0': (8, USED, 0.0, 7, KT, 0.7, SEED, 5,
              lambda s, a, ok: ok and a == 1.0 and s[R.K_BEFORE] == 0.0 and s[R.K_AFTER] == 0.0 and s[R.HEAT] == USED[R.HEAT]
              and s[R.APPLICATIONS] == 18 and s[R.TRIES] == 0),
    'T = 0': (8, USED, _k(7), 7, 0.0, 0.49, SEED, 5, lambda s, a, ok: ok and abs(a - 0.7) < 1e-15 and s[R.TRIES] >= 1),
    'T = 0 and c = 0': (8, USED, _k(7), 7, 0.0, 0.0, SEED, 5, lambda s, a, ok: ok and a == 0.0 and s[R.K_AFTER] == 0.0),
    'a draw of two tries': (8, FRESH, _k(3), 3, KT, 0.7, SEED, 31, lambda s, a, ok: ok and s[R.TRIES] >= 2),
    'fresh state': (8, FRESH, _k(4), 4, KT, 0.9, SEED, 0, lambda s, a, ok: ok and s[R.APPLICATIONS] == 1 and s[R.HEAT] == s[R.K_AFTER] - s[R.K_BEFORE]),
    'NaN K': (8, USED, float('nan'), 7, KT, 0.7, SEED, 5, lambda s, a, ok: not ok and s[R.FLAGS] == R.FAILED and tuple(s[:7]) == USED[:7]),
    'infinite K': (8, USED, float('inf'), 7, KT, 0.7, SEED, 5, lambda s, a, ok: not ok and s[R.FLAGS] == R.FAILED and tuple(s[:7]) == USED[:7]),
    'failed before, clean K now': (8, WAS_FAILED, _k(7), 7, KT, 0.7, SEED, 5,
                                   lambda s, a, ok: not ok and tuple(s) == WAS_FAILED),
    'a K so small that the factor overflows': (8, USED, 1e-320, 7, KT, 0.7, SEED, 5,
                                               lambda s, a, ok: not ok and s[R.FLAGS] == R.FAILED and tuple(s[:7]) == USED[:7]),
    'step above 2^32': (8, USED, _k(300), 300, KT, 0.95, 2 ** 40 + 3, 2 ** 33 + 11, lambda s, a, ok: ok and s[R.TRIES] >= 1),
    'seed and step at their top': (4, USED, _k(2, 0.4), 2, KT, 0.2, 2 ** 64 - 1, 2 ** 64 - 1, lambda s, a, ok: ok and s[R.TRIES] == 0),
})


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the header cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('vrescale_shim') / 'vrescale_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, '-o', exe, SHIM])
    return exe


def _real(prec):
    return np.float32 if prec == 4 else np.float64


@pytest.mark.parametrize('name', list(CASES))
def test_restatement_takes_the_branch_the_case_names(name):
    prec, state, K, nf, kT, c, seed, step, shows = CASES[name]
    out, alpha, ok = R.rule(state, K, nf, kT, c, seed, step, _real(prec))
    assert shows(out, alpha, ok), (out, alpha, ok)
    assert alpha >= 0.0


@pytest.mark.parametrize('name', list(CASES))
def test_header_agrees_with_the_restatement(shim, name):
    """The Philox words bit for bit, the try counts exactly, every other word to 1e-13 relative (the two libms differ in log,
    cos and sqrt by an ulp); at c = 1 the factor is exactly 1."""
    prec, state, K, nf, kT, c, seed, step, _ = CASES[name]
    out, alpha, ok = R.rule(state, K, nf, kT, c, seed, step, _real(prec))
    args = [str(prec)] + ['%.17g' % x for x in state] + ['%.17g' % K, str(nf), '%.17g' % kT, '%.17g' % c, str(seed), str(step)]
    got = subprocess.run([shim] + args, capture_output=True, text=True, check=True).stdout.split()
    assert len(got) == 19
    assert int(got[0]) == int(ok)
    assert got[11:15] == ['%08x' % w for w in R.words(seed, step, 0)]
    assert got[15:19] == ['%08x' % w for w in R.words(seed, step, 1)]
    assert int(got[10]) == R.noise(seed, step, nf)[2]
    have = np.array([float(x) for x in got[1:10]])
    want = np.concatenate([[alpha], out])
    assert have[1 + R.TRIES] == want[1 + R.TRIES] and have[1 + R.FLAGS] == want[1 + R.FLAGS]
    assert have[1 + R.APPLICATIONS] == want[1 + R.APPLICATIONS]
    err = np.abs(have - want)
    assert np.all(err <= 1e-13 * np.abs(want)), (have, want)
    if c == 1.0 and ok:
        assert have[0] == 1.0 and have[1 + R.ALPHA] == 1.0


def test_scalar_and_array_noise_are_one_function():
    steps = np.concatenate([np.arange(200), 2 ** 33 + np.arange(50)])
    for nf in NFS:
        R1, S, tries = R.noise_many(SEED, steps, nf)
        for k, step in enumerate(steps):
            r1, s, t = R.noise(SEED, int(step), nf)
            assert t == tries[k]
            assert abs(r1 - R1[k]) <= 1e-14 * abs(r1) and abs(s - S[k]) <= 1e-14 * abs(s)
    assert R.noise(SEED, 31, 3)[2] >= 2 and all(R.noise(SEED, s, 3)[2] == 1 for s in range(31))


@pytest.mark.parametrize('nf', NFS)
def test_noise_is_chi_square(nf):
    """c = 0 makes K' = (kT/2) (R1^2 + S), which must be chi^2(Nf): seed 12345, steps 0 .. 19999, Kolmogorov's D sqrt(M) below
    1.63, the 1 % critical value of its limiting distribution."""
    from scipy import stats
    M = 20000
    R1, S, tries = R.noise_many(SEED, np.arange(M), nf)
    assert tries.min() >= (1 if nf >= 3 else 0) and tries.max() < R.MAX_TRIES
    D = stats.kstest(R1 * R1 + S, stats.chi2(nf).cdf).statistic
    print('Nf %d: D sqrt(M) = %.2f, largest try count %d' % (nf, D * math.sqrt(M), tries.max()))
    assert D * math.sqrt(M) < 1.63


@pytest.mark.parametrize('nf,c', [(6, 0.9), (1, 0.5), (1943, 0.99)])
def test_chain_is_canonical(nf, c):
    """K_{k+1} = rule(K_k) without forces, 20 000 steps of which the first 2 000 are dropped: x = K / (kT/2) must have the mean
    Nf of chi^2(Nf) within 5 sigma, sigma = sqrt(2 Nf (1 + c) / ((1 - c) n)) (the variance 2 Nf of one sample times the
    integrated autocorrelation time (1 + c) / (1 - c) of a chain whose correlation decays as c^k), and its variance within 15 %."""
    state, K = R.fresh_state(), 0.5 * nf * 0.5 * KT
    xs = []
    for step in range(20000):
        state, _, ok = R.rule(state, K, nf, KT, c, SEED, step)
        assert ok
        K = state[R.K_AFTER]
        xs.append(K / (0.5 * KT))
    x = np.array(xs[2000:])
    sigma = math.sqrt(2.0 * nf * (1.0 + c) / ((1.0 - c) * len(x)))
    print('Nf %d, c %g: mean off by %.2f sigma, variance ratio %.3f' % (nf, c, (x.mean() - nf) / sigma, x.var() / (2.0 * nf)))
    assert abs(x.mean() - nf) < 5.0 * sigma
    assert abs(x.var() / (2.0 * nf) - 1.0) < 0.15
    assert abs(state[R.HEAT] - (K - 0.5 * nf * 0.5 * KT)) <= 1e-9 * nf * KT      # without forces the heat is all of the change
