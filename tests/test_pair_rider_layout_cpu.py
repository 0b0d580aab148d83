"""Block-id layout of the x pass that carries the closing pair kernel (admp_amd/csrc/rider_layout.h rider_block, the
function k_xconv_pair_full calls), host-compiled.

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
HDR = os.path.join(os.path.dirname(HERE), 'admp_amd', 'csrc', 'rider_layout.h')

PAIR, IND, TILE, IDLE = 0, 1, 2, 3
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in (SRC, HDR)):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC])
        _lib = ctypes.CDLL(LIB)
        _lib.rider_blocks.restype = ctypes.c_uint
        _lib.rider_blocks.argtypes = [ctypes.c_uint] * 4
        _lib.rider_map.restype = None
        _lib.rider_map.argtypes = [ctypes.c_uint] * 6 + [ctypes.c_void_p]
    return _lib


def layout(npair, nind, nbx, ny, gdx, gdy):
    out = np.full((gdx * gdy, 4), -1, dtype=np.int64)
    lib().rider_map(npair, nind, nbx, ny, gdx, gdy, out.ctypes.data_as(ctypes.c_void_p))
    return out


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
    """3072 atoms on the 97^3 mesh: 192 pair workgroups, 5 tiles for each of 97 y rows"""
    total = 192 + nind + 5 * 97
    check(192, nind, 5, 97, total, 1)                       # the launch shape of launch_dft_x_conv_full_rider
    check(192, nind, 5, 97, total + 13, 1)                  # surplus blocks are idle
    check(192, nind, 5, 97, 97, (total + 96) // 97)         # the same map under a two-dimensional grid
    check(192, nind, 5, 97, 8, (total + 7) // 8 + 1)


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
