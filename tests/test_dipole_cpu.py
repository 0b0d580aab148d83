"""The arithmetic of the dipole observable on the host (admp_amd/csrc/dipole_math.h, the text the kernels of dipole_kernels.hip
compile; tests/dipole_shim/main.cpp) against the float64 restatement of tests/dipole_ref.py, and the host helpers of
admp_amd.md: the CSR builder, the dielectric constant, and the gas-phase dipole of the water model as a fixed point.

Double arithmetic is held to 64 eps_f64 sum |terms| per word and per mu_c.  Float arithmetic (frames and minimum images in
float, products and sums in double) is MEASURED: the largest err / (eps_f32 sum |terms|) over the four cases is printed with -s
and held to dipole_ref.SINGLE_RATIO, the figure the GPU test's single-precision bar is four times of.  Measured here: 0.577
(water64 0.237, water64_tric 0.236, general 0.577, general_tric 0.509; recorded as 0.58)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dipole_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = ROOT + '/admp_amd/csrc'
SHIM = ROOT + '/tests/dipole_shim/main.cpp'


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the headers cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('dipole_shim') / 'dipole_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I', CSRC, '-o', exe, SHIM])
    return exe


def run_shim(shim, prec, c, pos, Q, U, masses, start, atoms):
    n, ng = len(pos), len(start) - 1
    lines = ['%d %d %d' % (n, ng, 0 if U is None else 1), ' '.join('%.17g' % x for x in c['box'].reshape(-1))]
    Uz = np.zeros((n, 3)) if U is None else U
    for i in range(n):
        lines.append(' '.join('%.17g' % x for x in (*pos[i], *Q[i], *Uz[i], 1.0 / masses[i]))
                     + ' %d %d %d %d' % (c['axis_type'][i], *c['axis_idx'][i]))
    lines.append(' '.join(str(int(x)) for x in start))
    lines.append(' '.join(str(int(x)) for x in atoms))
    out = subprocess.run([shim, prec], input='\n'.join(lines) + '\n', capture_output=True, text=True, check=True).stdout
    v = np.array(out.split(), dtype=np.float64)
    assert len(v) == 16 + 3 * ng
    return v[:16], v[16:].reshape(ng, 3)


def held(c, prec):
    """the case's arrays as a handle of that precision holds them (1 / m included: the kernel divides 1 by it again)"""
    t = np.float32 if prec == 'f' else np.float64
    r = lambda a: np.asarray(a, dtype=t).astype(np.float64)      # noqa: E731
    return r(c['pos']), r(c['Q_local']), r(c['U']), 1.0 / r(1.0 / c['masses'])


def csr_of(c):
    from admp_amd.md import group_csr
    return group_csr(c['labels'])


@pytest.mark.parametrize('name', R.CASES)
def test_double_arithmetic_against_the_restatement(shim, name):
    c = R.case(name)
    pos, Q, U, m = held(c, 'd')
    start, atoms = csr_of(c)
    for Ux in (U, None):
        words, mu = run_shim(shim, 'd', c, pos, Q, Ux, m, start, atoms)
        x = R.excess(words, mu, R.reference(c, pos, Q, Ux, m), 64 * R.EPS64)
        print('%s%s: err / bar %.3f' % (name, '' if Ux is not None else ' (no U)', x))
        assert x <= 1.0
        if Ux is None:
            assert (words[6:9] == 0).all()


def test_float_arithmetic_is_measured_and_within_the_recorded_ratio(shim):
    worst = 0.0
    for name in R.CASES:
        c = R.case(name)
        pos, Q, U, m = held(c, 'f')
        start, atoms = csr_of(c)
        words, mu = run_shim(shim, 'f', c, pos, Q, U, m, start, atoms)
        x = R.excess(words, mu, R.reference(c, pos, Q, U, m), R.EPS32)
        print('%s: err / (eps_f32 sum |terms|) %.3f' % (name, x))
        worst = max(worst, x)
    print('largest %.3f, recorded %.3f' % (worst, R.SINGLE_RATIO))
    assert worst <= R.SINGLE_RATIO


def test_the_cases_are_what_they_claim():
    for name in ('water64', 'water64_tric'):
        assert R.case(name)['n_straddling'] >= 1
    for name in ('general', 'general_tric'):
        c = R.case(name)
        groups = R.groups_brute(c['labels'])
        sizes = sorted(len(g) for g in groups)
        assert len(groups) == 300 and len(groups) % 256 != 0 and len(groups) > 256
        assert sizes.count(1) == 120 and sizes.count(3) == 179 and sizes[-1] == 70
        assert set(c['axis_type'].tolist()) == {0, 1, 2, 3, 4, 5}
        assert any(np.any(np.diff(g) != 1) for g in groups if len(g) > 1)          # groups are not runs of atoms
        s = c['pos'] @ np.linalg.inv(c['box'])
        assert ((s < 0) | (s >= 1)).any()                                           # atoms outside the cell
        for g in groups:                                                            # narrower than half the cell
            d = R.min_image(c['pos'][g] - c['pos'][g[0]], c['box']) @ np.linalg.inv(c['box'])
            assert (d.max(axis=0) - d.min(axis=0)).max() < 0.5


def test_csr_builder_against_brute_force():
    from admp_amd.md import group_csr
    rng = np.random.default_rng(3)
    lists = [R.case('general')['labels'], R.case('water64')['labels'], np.arange(7)[::-1], np.zeros(5, dtype=np.int64),
             np.array([], dtype=np.int32), rng.integers(-5, 5, size=200), np.array([7, -3, 7, 2 ** 31 - 1, -3, -2 ** 31])]
    for labels in lists:
        start, atoms = group_csr(labels)
        want = R.groups_brute(labels)
        assert start.dtype == np.int32 and atoms.dtype == np.int32
        assert len(start) == len(want) + 1 and start[0] == 0 and start[-1] == len(labels)
        assert [atoms[start[g]:start[g + 1]].tolist() for g in range(len(want))] == want
    with pytest.raises(ValueError):
        group_csr(np.zeros((2, 2), dtype=np.int32))
    with pytest.raises(ValueError):
        group_csr(np.array([0.5, 1.0]))


def test_dielectric_constant_by_hand():
    """M = (+-1, 0, 0): <M.M> = 1, <M> = 0.  V = 1000 A^3, T = 300 K: 1 + 4 pi 1389.35455846 / (3 1000 0.0083144626 300) =
    1 + 17458.5517.../7483.01634 = 3.33312...; a constant offset of M changes nothing; one row has no fluctuation"""
    from admp_amd.md import KB, dielectric_constant
    from admp_amd.pme import DIELECTRIC
    want = 1.0 + 4.0 * np.pi * 1389.35455846 / (3.0 * 1000.0 * 0.0083144626 * 300.0)
    assert abs(want - 3.3331) < 1e-4
    assert (DIELECTRIC, KB) == (1389.35455846, 0.0083144626)
    M = np.array([[1.0, 0, 0], [-1.0, 0, 0]])
    assert abs(dielectric_constant(M, 1000.0, 300.0) - want) < 1e-12
    assert abs(dielectric_constant(M + np.array([0.3, -2.0, 5.0]), 1000.0, 300.0) - want) < 1e-9
    assert dielectric_constant(M[:1], 1000.0, 300.0) == 1.0
    # <M.M> - <M>.<M> over the rows (0,0,0), (0,2,0), (0,0,4): 20/3 - 20/9 = 40/9
    M3 = np.array([[0.0, 0, 0], [0, 2.0, 0], [0, 0, 4.0]])
    assert abs(dielectric_constant(M3, 500.0, 100.0) - (1.0 + 4.0 * np.pi * DIELECTRIC * (40.0 / 9.0) / (3.0 * 500.0 * KB * 100.0))) < 1e-9


def test_gas_phase_water_dipole_is_a_fixed_point():
    """one molecule of systems.water_parameters in its model geometry: q r + the oxygen's dipole rotated by the oracle =
    0.38513861 e A = 1.8499 D, along the bisector; the restatement's form of p_i gives the oracle's rotation"""
    from admp_amd import systems as S
    from admp_amd.md import DEBYE_PER_E_ANGSTROM
    from oracle import admp_oracle as O
    half = 0.5 * S.ANG_HOH
    pos = np.array([[0.0, 0, 0], [S.R_OH * np.sin(half), 0, S.R_OH * np.cos(half)], [-S.R_OH * np.sin(half), 0, S.R_OH * np.cos(half)]])
    pos = pos + np.array([3.0, 4.0, 5.0])
    box = np.eye(3) * 20.0
    at, ai, _ = S.water_topology(1)
    Q = S.water_parameters(1)['Q_local']
    F = O.construct_local_frames(pos, box, at, ai)
    Qg = O.rot_local2global(O._t(Q), F, 2).numpy()
    mu = (Q[:, 0:1] * (pos - pos[0])).sum(axis=0) + Qg[:, [2, 3, 1]].sum(axis=0)
    assert abs(np.linalg.norm(mu) - 0.38513861) < 1e-8
    assert abs(np.linalg.norm(mu) * DEBYE_PER_E_ANGSTROM - 1.8499) < 1e-4
    assert abs(mu[0]) < 1e-12 and abs(mu[1]) < 1e-12 and mu[2] > 0
    c = dict(pos=pos, box=box, Q_local=Q, U=np.zeros((3, 3)), masses=np.array(R.MASS_WATER), axis_type=at, axis_idx=ai,
             labels=np.zeros(3, dtype=np.int32))
    ref = R.reference(c)
    assert np.abs(ref['mu'][0] - mu).max() < 1e-15
    assert ref['words'][12] == 1 and abs(ref['words'][9] - 0.38513861) < 1e-8
