"""Block-id layout of the x pass that carries the closing pair kernel (admp_amd/csrc/rider_layout.h rider_block, the
function k_xconv_pair_full calls) and the launch plan of the x pass (admp_amd/csrc/dft_plan.h dft_x_plan, the function
every x-pass launcher calls), host-compiled.

The plan, for every line length 2..160, both word sizes and both forms of the pass, against a restatement of the rule in
Python: columns per tile, tiles per row and LDS bytes agree; a tile's tasks fit the workgroup, the tiles cover the row and
a tile of more than one column stays inside the LDS budget.

For the grid of the headline system (97 y rows, 5 tiles per row, 192 pair workgroups, with and without the workgroups
of the field-increment kernel) and seeded others, in one- and two-dimensional launch shapes: every block id maps to
exactly one (kind, rank); every tile (t, y) and every rider rank appears exactly once; blocks beyond the layout are idle;
all pair ranks precede all field-increment ranks, which precede all tiles, in the linear order the workgroups start in;
a tile keeps the linear position it has in a launch of its own (t + nbx * y), offset by the riders' workgroups."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostshim', 'rider_shim.cpp')
LIB = os.path.join(HERE, 'hostshim', 'libadmp_ridershim.so')
CSRC = os.path.join(os.path.dirname(HERE), 'admp_amd', 'csrc')
HDRS = [os.path.join(CSRC, h) for h in ('rider_layout.h', 'dft_plan.h', 'dft_math.h', 'pme_math.h')]

PAIR, IND, TILE, IDLE = 0, 1, 2, 3
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in [SRC] + HDRS):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC])
        _lib = ctypes.CDLL(LIB)
        _lib.rider_blocks.restype = ctypes.c_uint
        _lib.rider_blocks.argtypes = [ctypes.c_uint] * 4
        _lib.rider_map.restype = None
        _lib.rider_map.argtypes = [ctypes.c_uint] * 6 + [ctypes.c_void_p]
        _lib.x_pass_plan.restype = None
        _lib.x_pass_plan.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    return _lib


def layout(npair, nind, nbx, ny, gdx, gdy):
    out = np.full((gdx * gdy, 4), -1, dtype=np.int64)
    lib().rider_map(npair, nind, nbx, ny, gdx, gdy, out.ctypes.data_as(ctypes.c_void_p))
    return out


def plan(K, w, circ):
    """dft_x_plan of mesh K in words of w bytes: dict of N, Kh, TK, NC, nbx, lds"""
    out = np.zeros(6, dtype=np.int64)
    lib().x_pass_plan(K[0], K[1], K[2], w, 1 if circ else 0, out.ctypes.data_as(ctypes.c_void_p))
    return dict(zip(('N', 'Kh', 'TK', 'NC', 'nbx', 'lds'), (int(v) for v in out)))


# the rule as the x-pass launchers spelled it out before they shared the plan: 256 threads, two output pairs per thread,
# 60 KB of LDS; a complex number is 2 words, a pair sum 4
BLOCK, BUDGET, KQ = 256, 60 * 1024, 2


def rule_tasks(N):
    return (N // 2 + 1 + KQ - 1) // KQ


def rule_cols(N, bytes_per_col, fixed_bytes):
    nc = max(BLOCK // rule_tasks(N), 1)
    while nc > 1 and fixed_bytes + bytes_per_col * nc > BUDGET:
        nc -= 1
    return nc


def rule(N, Kh, w, circ):
    H, cx, pcx = (N - 1) // 2, 2 * w, 4 * w
    if circ:
        ext = N // 2 + N // 2 + (N - 1) // 2 + 1            # circ_ext_len
        col = pcx * H + 2 * cx + w * ext
        NC = rule_cols(N, col, 0)
        lds = col * NC
    else:
        NC = rule_cols(N, pcx * H + cx * (2 + N), cx * N)
        lds = pcx * (H * NC) + cx * (N + 2 * NC + N * NC)
    return NC, (Kh + NC - 1) // NC, lds


def test_plan_matches_the_rule():
    for N in range(2, 161):
        for Kh in (2, 3, 49, 81):
            for w in (4, 8):
                for circ in (False, True):
                    p = plan((N, 7, 2 * Kh - 1), w, circ)
                    NC, nbx, lds = rule(N, Kh, w, circ)
                    assert (p['N'], p['Kh'], p['TK']) == (N, Kh, rule_tasks(N))
                    assert (p['NC'], p['nbx'], p['lds']) == (NC, nbx, lds), (N, Kh, w, circ)
                    assert p['NC'] * p['TK'] <= 256
                    assert p['nbx'] * p['NC'] >= Kh
                    assert p['NC'] == 1 or p['lds'] <= 60 * 1024


def check(npair, nind, nbx, ny, gdx, gdy):
    total = lib().rider_blocks(npair, nind, nbx, ny)
    assert total == npair + nind + nbx * ny
    assert gdx * gdy >= total
    m = layout(npair, nind, nbx, ny, gdx, gdy)
    kind = m[:, 0]
    assert set(np.unique(kind)) <= {PAIR, IND, TILE, IDLE}              # one kind per block id
    lin = np.arange(gdx * gdy)
    for k, n in ((PAIR, npair), (IND, nind)):
        ranks = m[kind == k, 1]
        assert len(ranks) == n and np.array_equal(np.sort(ranks), np.arange(n))      # every rank exactly once
    tiles = m[kind == TILE]
    assert len(tiles) == nbx * ny
    assert (tiles[:, 2] < nbx).all() and (tiles[:, 3] < ny).all()
    assert len({(int(t), int(y)) for t, y in tiles[:, 2:4]}) == nbx * ny                # every (t, y) exactly once
    assert (kind[total:] == IDLE).all() and (kind[:total] != IDLE).all()                # surplus blocks, and only they
    # start order: pair, then field increment, then tiles
    if npair and nind:
        assert lin[kind == PAIR].max() < lin[kind == IND].min()
    if npair and nbx * ny:
        assert lin[kind == PAIR].max() < lin[kind == TILE].min()
    if nind and nbx * ny:
        assert lin[kind == IND].max() < lin[kind == TILE].min()
    # ranks ascend with the block id (rank r on XCD r % 8 when the riders' counts are multiples of 8), tiles keep the
    # linear position of a launch of their own
    assert np.array_equal(m[kind == PAIR, 1], lin[kind == PAIR])
    assert np.array_equal(m[kind == IND, 1], lin[kind == IND] - npair)
    assert np.array_equal(tiles[:, 2] + nbx * tiles[:, 3], lin[kind == TILE] - npair - nind)


@pytest.mark.parametrize('nind', [0, 64, 8])
def test_headline_grid(nind):
    """3072 atoms on the 97^3 mesh: 192 pair workgroups, 5 tiles (the plan's count, f64, either form) for each of 97 y rows"""
    for circ in (True, False):
        p = plan((97, 97, 97), 8, circ)
        assert (p['N'], p['Kh']) == (97, 49)
        nbx = p['nbx']
        assert nbx == 5
        total = 192 + nind + nbx * 97
        check(192, nind, nbx, 97, total, 1)                     # the launch shape of launch_dft_x_pass with the pair rider
        check(192, nind, nbx, 97, total + 13, 1)                # surplus blocks are idle
        check(192, nind, nbx, 97, 97, (total + 96) // 97)       # the same map under a two-dimensional grid
        check(192, nind, nbx, 97, 8, (total + 7) // 8 + 1)


def test_seeded_grids():
    rng = np.random.default_rng(20260)
    for _ in range(200):
        npair = 8 * int(rng.integers(0, 60))
        nind = 8 * int(rng.integers(0, 20))
        nbx, ny = int(rng.integers(1, 12)), int(rng.integers(1, 130))
        total = npair + nind + nbx * ny
        gdx = int(rng.integers(1, total + 20))
        gdy = (total + gdx - 1) // gdx + int(rng.integers(0, 2))
        check(npair, nind, nbx, ny, gdx, gdy)
        check(npair, nind, nbx, ny, total, 1)


def test_kernel_uses_the_layout():
    """the rider kernel takes its block kinds from rider_block and nothing else"""
    src = open(os.path.join(os.path.dirname(HERE), 'admp_amd', 'csrc', 'pair_kernels.hip')).read()
    body = src[src.index('void k_xconv_pair_full('):]
    body = body[:body.index('\n}\n')]
    assert 'rider_block(rg, blockIdx.x, blockIdx.y, gridDim.x)' in body
    assert body.count('blockIdx') == 2
