"""The matrix-core share of the plane kernels' y lines (admp_amd/csrc/plane_mfma_plan.h: the plan, the lane maps that
k_dft_zy_fwd<double, 2, SPREAD, true> calls, and one unit's sums in the matrix-core order), host-compiled.

Coverage, for every line length N = 6..160 and the column counts the two workgroups of a plane receive (the halves of
Kh = N3 / 2 + 1 for N3 = 6..160: 2..41 columns): walking the workgroup as the kernel does -- waves [0, Wm) over their units,
lane by lane and accumulator word by word, then the vector tasks -- every word of every output X[k], k = 0..N/2, of every
column is produced exactly once, by a matrix unit or by a vector task and never by both; operands at padded positions and
in dead columns are zeros (plane_mfma_operand_live lets none through); H < 16 has no share; N = 97 has three whole output
tiles and no masked row.

Tile arithmetic, N = 33 (H = 16, one exact tile), 34 (even: the Nyquist term), 35 (H = 17, one tile and one masked-down
row), 97 (the workload's length), both directions, 9 columns (one whole column tile, one of a single column): the four sums
of every output (P and R of the real and the imaginary parts) of every unit in the matrix-core order against those of
dft_pair_core (dft_pair_partial) in double.  Bound: 64 ulp (of double, 2^-52) of the largest term of the column's sums, the
one dft_math.h states for the re-seeded recurrence; the matrix form multiplies exact table entries, so its own error lies
below that.  The outputs X[k], X[N-k] of both forms (two sums and x_0 each) are checked against numpy's FFT for routing.

The forward z lines (PlaneMfmaZPlan: 16 outputs against 16 real lines, the share every unit or none) the same way: for every
N = 6..160 and both kz ranges of a plane's two workgroups, against 5, 16, 17 and 97 lines, every (line, output) is produced
exactly once by the units when H >= 16 and by none below (the vector tasks keep the phase); the (P, R) sums of N = 33, 34, 35,
97 against real_pair_sums within the same bound, the outputs against numpy's rfft."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostshim', 'plane_mfma_shim.cpp')
LIB = os.path.join(HERE, 'hostshim', 'libadmp_planemfmashim.so')
CSRC = os.path.join(os.path.dirname(HERE), 'admp_amd', 'csrc')
HDRS = [os.path.join(CSRC, h) for h in ('plane_mfma_plan.h', 'dft_math.h', 'pme_math.h')]
NWAVES, KQ = 16, 2
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in [SRC] + HDRS):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC])
        _lib = ctypes.CDLL(LIB)
        _lib.plane_y_plan.restype = None
        _lib.plane_y_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
        _lib.plane_y_cover.restype = None
        _lib.plane_y_cover.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
        _lib.plane_y_lines.restype = ctypes.c_int
        _lib.plane_y_lines.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 6
        _lib.plane_z_plan.restype = None
        _lib.plane_z_plan.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
        _lib.plane_z_cover.restype = None
        _lib.plane_z_cover.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
        _lib.plane_z_lines.restype = ctypes.c_int
        _lib.plane_z_lines.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 6
    return _lib


def plan(N, ncols):
    out = np.zeros(9, dtype=np.int64)
    lib().plane_y_plan(N, ncols, NWAVES, out.ctypes.data_as(ctypes.c_void_p))
    return dict(zip(('N', 'H', 'KP', 'ncols', 'MT', 'CT', 'nm', 'nunits', 'Wm'), (int(v) for v in out)))


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def column_counts():
    """what the two workgroups of a plane receive: kz0 = Kh z / 2"""
    out = set()
    for N3 in range(6, 161):
        Kh = N3 // 2 + 1
        out.add(Kh // 2)
        out.add(Kh - Kh // 2)
    return sorted(out)


def test_every_output_once_and_padding_is_zero():
    cols = column_counts()
    assert cols[0] == 2 and cols[-1] == 41
    for N in range(6, 161):
        for nc in cols:
            p = plan(N, nc)
            H = (N - 1) // 2
            assert p['H'] == H and p['KP'] % 4 == 0 and H <= p['KP'] < H + 4
            if H < 16:
                assert p['CT'] == 0 and p['nunits'] == 0 and p['Wm'] == 0 and p['nm'] == 0, (N, nc, p)
            else:
                assert p['MT'] == -(-H // 16) and p['nm'] == min(8 * p['CT'], nc) and p['nunits'] == p['MT'] * p['CT'], (N, nc, p)
                assert 0 < p['Wm'] <= NWAVES and (p['nm'] == nc or p['Wm'] < NWAVES), (N, nc, p)     # someone runs the vector tasks
            cnt = np.zeros((N // 2 + 1, nc, 2), dtype=np.int64)
            mat = np.zeros_like(cnt)
            pad = np.zeros(4, dtype=np.int64)
            lib().plane_y_cover(N, nc, NWAVES, KQ, ptr(cnt), ptr(mat), ptr(pad))
            assert (cnt == 1).all(), (N, nc, p, np.argwhere(cnt != 1)[:4])
            assert (mat[:, :p['nm']] == 1).all() and (mat[:, p['nm']:] == 0).all(), (N, nc, p)
            assert pad[1] == 0, (N, nc, pad)
            assert pad[2] == 2 * p['MT'] * H * p['nm'], (N, nc, pad)            # every live operand word is fetched once per output tile
            assert pad[3] == p['CT'] * (16 * p['MT'] - H if p['CT'] else 0), (N, nc, pad)


def test_headline_length_has_whole_tiles():
    for nc in (24, 25):
        p = plan(97, nc)
        assert (p['H'], p['KP'], p['MT'], p['CT'], p['nm'], p['nunits'], p['Wm']) == (48, 48, 3, (nc + 7) // 8, nc, 3 * ((nc + 7) // 8),
                                                                                   3 * ((nc + 7) // 8)), p
        pad = np.zeros(4, dtype=np.int64)
        cnt = np.zeros((49, nc, 2), dtype=np.int64)
        lib().plane_y_cover(97, nc, NWAVES, KQ, ptr(cnt), ptr(np.zeros_like(cnt)), ptr(pad))
        assert pad[3] == 0                     # no masked output row; the only dead operands are the columns beyond nc
        assert pad[0] == 3 * 2 * 48 * (8 * p['CT'] - nc)


@pytest.mark.parametrize('N', [33, 34, 35, 97])
@pytest.mark.parametrize('sign', [-1, 1])
def test_tile_sums_in_matrix_core_order(N, sign):
    nc = 9
    rng = np.random.default_rng(100 * N + sign)
    x = rng.uniform(-1.0, 1.0, size=(N, nc, 2))
    Xm = np.full((N, nc, 2), np.nan)
    Xv = np.full((N, nc, 2), np.nan)
    big = np.zeros(nc)
    H = (N - 1) // 2
    Sm = np.full((N // 2 + 1, nc, 4), np.nan)
    Sv = np.full((N // 2 + 1, nc, 4), np.nan)
    nu = lib().plane_y_lines(N, nc, NWAVES, sign, ptr(x), ptr(Xm), ptr(Xv), ptr(Sm), ptr(Sv), ptr(big))
    assert nu == -(-H // 16) * 2
    assert np.isfinite(Xm).all() and np.isfinite(Xv).all()         # every output written by both forms
    ref = np.fft.fft(x[..., 0] + 1j * x[..., 1], axis=0) if sign < 0 else np.fft.ifft(x[..., 0] + 1j * x[..., 1], axis=0) * N
    for X in (Xm, Xv):
        assert np.abs(X[..., 0] + 1j * X[..., 1] - ref).max() <= 1e-12 * np.abs(ref).max()    # (routing: the right output in the right place)
    assert np.isfinite(Sm[1:H + 1]).all() and np.isfinite(Sv[1:H + 1]).all()
    d = np.abs(Sm[1:H + 1] - Sv[1:H + 1]).max(axis=(0, 2))
    bound = 64 * 2.0 ** -52 * big
    print('N=%d sign=%+d: largest |matrix order - dft_pair_core| / (64 ulp of the largest term) = %.3f' % (N, sign, (d / bound).max()))
    assert (d <= bound).all(), (N, sign, d / bound)


def zplan(N, k0, nout, nl):
    out = np.zeros(10, dtype=np.int64)
    lib().plane_z_plan(N, k0, nout, nl, NWAVES, out.ctypes.data_as(ctypes.c_void_p))
    return dict(zip(('N', 'H', 'KP', 'nlines', 'k0', 'nout', 'MT', 'LT', 'nunits', 'Wm'), (int(v) for v in out)))


def kz_ranges(N):
    Kh = N // 2 + 1
    return [(Kh * z // 2, Kh * (z + 1) // 2 - Kh * z // 2) for z in (0, 1)]


def test_z_lines_every_output_once():
    for N in range(6, 161):
        H = (N - 1) // 2
        for k0, nout in kz_ranges(N):
            for nl in (5, 16, 17, 97):
                p = zplan(N, k0, nout, nl)
                cnt = np.zeros((nl, nout), dtype=np.int64)
                pad = np.zeros(2, dtype=np.int64)
                lib().plane_z_cover(N, k0, nout, nl, NWAVES, ptr(cnt), ptr(pad))
                if H < 16:
                    assert p['nunits'] == 0 and p['Wm'] == 0 and (cnt == 0).all(), (N, k0, nout, nl, p)
                else:
                    assert p['MT'] == -(-nout // 16) and p['LT'] == -(-nl // 16) and 0 < p['Wm'] <= NWAVES, (N, k0, nout, nl, p)
                    assert (cnt == 1).all(), (N, k0, nout, nl, p)
                assert pad[1] == 0, (N, k0, nout, nl, pad)
    p = zplan(97, 0, 25, 97)
    assert (p['MT'], p['LT'], p['nunits'], p['Wm'], p['KP']) == (2, 7, 14, 14, 48), p


@pytest.mark.parametrize('N', [33, 34, 35, 97])
def test_z_tile_sums_in_matrix_core_order(N):
    nl = 19
    rng = np.random.default_rng(7 * N)
    x = rng.uniform(-1.0, 1.0, size=(nl, N))
    ref = np.fft.rfft(x, axis=1)
    worst = 0.0
    for k0, nout in kz_ranges(N):
        Xm, Xv = np.full((nl, nout, 2), np.nan), np.full((nl, nout, 2), np.nan)
        Sm, Sv = np.full((nl, nout, 2), np.nan), np.full((nl, nout, 2), np.nan)
        big = np.zeros(nl)
        nu = lib().plane_z_lines(N, k0, nout, nl, NWAVES, ptr(x), ptr(Xm), ptr(Xv), ptr(Sm), ptr(Sv), ptr(big))
        assert nu == -(-nout // 16) * 2
        for X in (Xm, Xv):
            assert np.isfinite(X).all()
            assert np.abs(X[..., 0] + 1j * X[..., 1] - ref[:, k0:k0 + nout]).max() <= 1e-12 * np.abs(ref).max()
        d = np.abs(Sm - Sv).max(axis=(1, 2))
        bound = 64 * 2.0 ** -52 * big
        worst = max(worst, float((d / bound).max()))
        assert (d <= bound).all(), (N, k0, d / bound)
    print('N=%d z lines: largest |matrix order - real_pair_sums| / (64 ulp of the largest term) = %.3f' % (N, worst))
