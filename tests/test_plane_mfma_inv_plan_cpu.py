"""The matrix-core share of the inverse plane kernel (admp_amd/csrc/plane_mfma_plan.h: PlaneInvSplit, PlaneMfmaInvYPlan,
PlaneMfmaInvZPlan, the lane maps that k_dft_yz_inv<double, 2, true> calls and one unit's sums in the matrix-core order),
host-compiled.

Lengths N2, N3 in {33, 34, 37, 38, 97}: H = 16 exactly (one whole tile), even lengths with a Nyquist term, H = 18 (masked rows),
H = 48 (three whole tiles; the workload's length); 31 (H = 15) must give no share.

The split: for every N = 6..160 the lines plane_inv_line lists for a workgroup are exactly the vector kernel's s_lines (the
shim carries a copy of that loop), without repeats, and the two workgroups together list every row once.
y phase: walking both workgroups as the kernel does -- waves over their units, lane by lane and accumulator word by word --
every word of every (row, column) of V is written exactly once, each workgroup writes exactly the rows of its s_lines, and
every operand fetched at a padded position or in a dead column is zero (plane_mfma_inv_y_operand_live lets none through).
z phase: every (line, j) of the workgroup's lines is stored exactly once; operands at padded positions and dead lines are zero.
The unit counts at 97 are at most 16 (one round of the 16 waves): 14 and 9 or 12.

Tile sums: the sums P, R of every output in the matrix-core order (plane_mfma_inv_y_unit_host, plane_mfma_inv_z_unit_host)
against dft_pair_partial / real_pair_sums (what dft_pair_core<+1> and irdft_pair_outputs sum) in double on random data.
Bound, derived: a sum of H <= N / 2 products, each factor of modulus <= 1 times an operand, carries a rounding error of at
most H u S in either order (u = 2^-53, S = the sum of the |operands| over the positions); the vector form's twiddles come from
a recurrence re-seeded from the table, which dft_math.h bounds at 64 ulp = 128 u per factor, i.e. 128 u S.  Together
(2 H + 128) u S <= 8 N u S for N >= 22, so the bound is 8 * 2^-53 * N * S.  The outputs of both forms are checked against
numpy's FFT for routing.

Measured: the largest |matrix order - vector order| is 0.015 of the bound (y, N = 33) and 0.020 (z, N = 37)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostshim', 'plane_mfma_inv_shim.cpp')
LIB = os.path.join(HERE, 'hostshim', 'libadmp_planemfmainvshim.so')
CSRC = os.path.join(os.path.dirname(HERE), 'admp_amd', 'csrc')
HDRS = [os.path.join(CSRC, h) for h in ('plane_mfma_plan.h', 'dft_math.h', 'pme_math.h')]
NWAVES, KQ = 16, 2
LENGTHS = (33, 34, 37, 38, 97)
NOSHARE = 31
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in [SRC] + HDRS):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC])
        _lib = ctypes.CDLL(LIB)
        i, p = ctypes.c_int, ctypes.c_void_p
        for name, res, args in (('inv_lines_vector', i, [i] * 4 + [p]), ('inv_lines_plan', i, [i] * 3 + [p] * 2),
                                ('inv_y_plan', None, [i] * 5 + [p]), ('inv_y_cover', None, [i] * 5 + [p] * 2),
                                ('inv_y_lines', i, [i] * 3 + [p] * 6), ('inv_z_plan', None, [i] * 3 + [p]),
                                ('inv_z_cover', None, [i] * 3 + [p] * 2), ('inv_z_lines', i, [i] * 3 + [p] * 6)):
            getattr(_lib, name).restype = res
            getattr(_lib, name).argtypes = args
    return _lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lines_vector(N, z):
    buf = np.zeros(2 * 160 + 2, dtype=np.int64)
    n = lib().inv_lines_vector(N, z, 2, KQ, ptr(buf))
    return [int(v) for v in buf[:n]]


def lines_plan(N, z):
    buf = np.zeros(2 * 160 + 2, dtype=np.int64)
    out = np.zeros(10, dtype=np.int64)
    n = lib().inv_lines_plan(N, z, 2, ptr(buf), ptr(out))
    names = ('TK', 'g0', 'g1', 'kb0', 'kn0', 'kb1', 'kn1', 'own0', 'ownn', 'nlines')
    return [int(v) for v in buf[:n]], dict(zip(names, (int(v) for v in out)))


def yplan(N, nc, z):
    out = np.zeros(8, dtype=np.int64)
    lib().inv_y_plan(N, nc, z, 2, NWAVES, ptr(out))
    return dict(zip(('H', 'KP', 'T0', 'T1', 'MT', 'CT', 'nunits', 'Wm'), (int(v) for v in out)))


def zplan(N, nl):
    out = np.zeros(6, dtype=np.int64)
    lib().inv_z_plan(N, nl, NWAVES, ptr(out))
    return dict(zip(('H', 'KP', 'JT', 'LT', 'nunits', 'Wm'), (int(v) for v in out)))


def test_split_lists_the_vector_kernels_lines():
    for N in range(6, 161):
        seen = []
        for z in (0, 1):
            vec = lines_vector(N, z)
            got, s = lines_plan(N, z)
            assert s['nlines'] == len(vec) == len(set(vec)), (N, z, s, vec)
            assert len(got) == len(set(got)) and set(got) == set(vec), (N, z, s, sorted(got), sorted(vec))
            TK = -(-(N // 2 + 1) // 2)
            assert (s['TK'], s['g0'], s['g1']) == (TK, TK * z // 2, TK * (z + 1) // 2), (N, z, s)
            assert s['own0'] == (1 if z == 0 else 0), (N, z, s)              # kq = 0 belongs to workgroup 0
            if N % 2 == 0 and N >= 8:                                          # N/2 to the one whose second range reaches it
                assert s['ownn'] == (1 if s['g0'] + TK <= N // 2 < s['g1'] + TK else 0), (N, z, s)
            seen += got
        assert sorted(seen) == list(range(N)), N
    assert sorted(len(lines_vector(97, z)) for z in (0, 1)) == [47, 50]        # the workload: 3 and 4 line tiles


def test_y_phase_every_output_once_and_padding_is_zero():
    for N in LENGTHS + (NOSHARE,):
        H = (N - 1) // 2
        for N3 in LENGTHS + (NOSHARE,):
            nc = N3 // 2 + 1                                                    # every column of the plane
            total = np.zeros((N, nc, 2), dtype=np.int64)
            for z in (0, 1):
                p = yplan(N, nc, z)
                _, s = lines_plan(N, z)
                cnt = np.zeros((N, nc, 2), dtype=np.int64)
                pad = np.zeros(4, dtype=np.int64)
                lib().inv_y_cover(N, nc, z, 2, NWAVES, ptr(cnt), ptr(pad))
                if H < 16:
                    assert p['nunits'] == 0 and p['Wm'] == 0 and (cnt == 0).all(), (N, nc, z, p)
                    continue
                assert (p['T0'], p['T1']) == (-(-s['kn0'] // 16), -(-s['kn1'] // 16)) and p['MT'] == p['T0'] + p['T1'], (N, z, p, s)
                assert p['CT'] == -(-nc // 8) and p['nunits'] == p['MT'] * p['CT'] and 0 < p['Wm'] <= NWAVES, (N, nc, z, p)
                rows = sorted(int(r) for r in np.nonzero(cnt.sum(axis=(1, 2)))[0])
                assert rows == sorted(lines_vector(N, z)), (N, nc, z, rows)       # exactly the vector kernel's lines
                assert pad[1] == 0, (N, nc, z, pad)
                assert pad[2] == 2 * p['MT'] * H * nc, (N, nc, z, pad)            # every live operand word once per output tile
                assert pad[3] == p['CT'] * (16 * p['MT'] - s['kn0'] - s['kn1']), (N, nc, z, pad)
                total += cnt
            if H >= 16:
                assert (total == 1).all(), (N, nc, np.argwhere(total != 1)[:4])
    for z in (0, 1):
        p = yplan(97, 49, z)
        assert (p['MT'], p['CT'], p['nunits'], p['Wm']) == (2, 7, 14, 14) and p['nunits'] <= NWAVES, p


def test_z_phase_every_output_once_and_padding_is_zero():
    counts = sorted({len(lines_vector(N2, z)) for N2 in LENGTHS for z in (0, 1)} | {16, 17})      # (and a whole tile, one more)
    assert counts == [15, 16, 17, 18, 19, 47, 50], counts
    for N in LENGTHS + (NOSHARE,):
        H = (N - 1) // 2
        for nl in counts:
            p = zplan(N, nl)
            cnt = np.zeros((nl, N), dtype=np.int64)
            pad = np.zeros(2, dtype=np.int64)
            lib().inv_z_cover(N, nl, NWAVES, ptr(cnt), ptr(pad))
            if H < 16:
                assert p['nunits'] == 0 and p['Wm'] == 0 and (cnt == 0).all(), (N, nl, p)
            else:
                assert p['JT'] == -(-H // 16) and p['LT'] == -(-nl // 16) and p['nunits'] == p['JT'] * p['LT'], (N, nl, p)
                assert 0 < p['Wm'] <= NWAVES and (cnt == 1).all(), (N, nl, p, np.argwhere(cnt != 1)[:4])
                assert pad[0] == p['JT'] * (p['KP'] * 16 * p['LT'] - H * nl), (N, nl, pad)
            assert pad[1] == 0, (N, nl, pad)
    assert zplan(97, 47)['nunits'] == 9 and zplan(97, 50)['nunits'] == 12                # one round of the 16 waves


@pytest.mark.parametrize('N', LENGTHS)
def test_y_tile_sums_in_matrix_core_order(N):
    nc = 9                                                                     # one whole column tile, one of a single column
    rng = np.random.default_rng(300 * N + 1)
    x = rng.uniform(-1.0, 1.0, size=(N, nc, 2))
    Xm, Xv = np.full((N, nc, 2), np.nan), np.full((N, nc, 2), np.nan)
    H = (N - 1) // 2
    Sm, Sv = np.full((N // 2 + 1, nc, 4), np.nan), np.full((N // 2 + 1, nc, 4), np.nan)
    sabs = np.zeros(nc)
    nu = lib().inv_y_lines(N, nc, NWAVES, ptr(x), ptr(Xm), ptr(Xv), ptr(Sm), ptr(Sv), ptr(sabs))
    assert nu == 2 * sum(yplan(N, nc, z)['MT'] for z in (0, 1))
    assert np.isfinite(Xm).all() and np.isfinite(Xv).all()                     # every output written by both forms
    ref = np.fft.ifft(x[..., 0] + 1j * x[..., 1], axis=0) * N
    for X in (Xm, Xv):
        assert np.abs(X[..., 0] + 1j * X[..., 1] - ref).max() <= 1e-12 * np.abs(ref).max()    # (routing)
    assert np.isfinite(Sm[1:H + 1]).all() and np.isfinite(Sv[1:H + 1]).all()
    d = np.abs(Sm[1:H + 1] - Sv[1:H + 1]).max(axis=(0, 2))
    bound = 8 * 2.0 ** -53 * N * sabs
    print('N=%d y: largest |matrix order - dft_pair_core| / (8 * 2^-53 * N * sum|operand|) = %.4f' % (N, (d / bound).max()))
    assert (d <= bound).all(), (N, d / bound)


@pytest.mark.parametrize('N', LENGTHS)
def test_z_tile_sums_in_matrix_core_order(N):
    nl = 19                                                                    # one whole line tile, one with masked rows
    Kh, H = N // 2 + 1, (N - 1) // 2
    rng = np.random.default_rng(500 * N + 3)
    V = rng.uniform(-1.0, 1.0, size=(nl, Kh, 2))
    xm, xv = np.full((nl, N), np.nan), np.full((nl, N), np.nan)
    Sm, Sv = np.full((nl, H + 1, 2), np.nan), np.full((nl, H + 1, 2), np.nan)
    sabs = np.zeros(nl)
    nu = lib().inv_z_lines(N, nl, NWAVES, ptr(V), ptr(xm), ptr(xv), ptr(Sm), ptr(Sv), ptr(sabs))
    assert nu == -(-H // 16) * 2
    assert np.isfinite(xm).all() and np.isfinite(xv).all()
    spec = V[..., 0] + 1j * V[..., 1]
    spec[:, 0] = spec[:, 0].real                                               # (only the real parts of X[0] and X[N/2] count)
    if N % 2 == 0:
        spec[:, N // 2] = spec[:, N // 2].real
    ref = np.fft.irfft(spec, n=N, axis=1) * N
    for X in (xm, xv):
        assert np.abs(X - ref).max() <= 1e-12 * np.abs(ref).max()
    d = np.abs(Sm[:, 1:] - Sv[:, 1:]).max(axis=(1, 2))
    bound = 8 * 2.0 ** -53 * N * sabs
    print('N=%d z: largest |matrix order - irdft_pair_outputs| / (8 * 2^-53 * N * sum|operand|) = %.4f' % (N, (d / bound).max()))
    assert (d <= bound).all(), (N, d / bound)
