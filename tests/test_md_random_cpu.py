"""The random source of the MD thermostat (admp_amd/csrc/md_math.h) without a GPU: a numpy restatement of the generator
(Philox-4x32-10; counter = (atom, step low, step high, stream), key = (seed low, seed high)) and of the Box-Muller normals,
checked against the generator's published known answers; and the header itself, compiled by the host compiler into a
stand-alone program (tests/md_random_shim/main.cpp), against both.  tests/test_gpu_md_langevin.py imports the restatement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, 'tests', 'md_random_shim', 'main.cpp')
CSRC = os.path.join(ROOT, 'admp_amd', 'csrc')

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xffffffff)
KNOWN = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]
TRIPLES = [(1, 0, 0), (20240, 7, 1), (2 ** 40 + 3, 2 ** 33, 0)]      # (seed, step, stream)


def philox(counter, key):
    """four arrays (or numbers) of 32-bit counter words, two key words -> list of four uint64 arrays holding 32-bit words"""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                              # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0 = p0 >> np.uint64(32), p0 & LOW
        hi1, lo1 = p1 >> np.uint64(32), p1 & LOW
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c


def words(n, seed, step, stream):
    """(n,4) uint32: the words of atoms 0 .. n-1"""
    i = np.arange(n, dtype=np.uint64)
    full = lambda x: np.full(n, x, dtype=np.uint64)      # noqa: E731
    w = philox((i, full(step & 0xffffffff), full(step >> 32), full(stream)), (seed & 0xffffffff, seed >> 32))
    return np.stack(w, axis=1).astype(np.uint32)


def normals(n, seed, step, stream):
    """(n,3) float64: three standard normals per atom"""
    u = (words(n, seed, step, stream).astype(np.float64) + 0.5) * 2.0 ** -32
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    return np.stack([r0 * np.cos(2 * np.pi * u[:, 1]), r0 * np.sin(2 * np.pi * u[:, 1]), r1 * np.cos(2 * np.pi * u[:, 3])], axis=1)


def hexwords(w):
    return ' '.join('%08x' % int(x) for x in w)


def test_restatement_reproduces_the_published_known_answers():
    for counter, key, expect in KNOWN:
        assert hexwords(philox(counter, key)) == expect


def test_restatement_uses_both_halves_of_seed_and_step():
    base = words(8, 2 ** 40 + 3, 2 ** 33, 0)
    assert not np.array_equal(base, words(8, 3, 2 ** 33, 0)) and not np.array_equal(base, words(8, 2 ** 40 + 3, 0, 0))
    assert not np.array_equal(base, words(8, 2 ** 40 + 3, 2 ** 33, 1))
    z = normals(4096, 1, 0, 0)
    assert np.isfinite(z).all() and np.abs(z).max() <= 6.77


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the header cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('md_random_shim') / 'md_random_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, '-o', exe, SHIM])
    return exe


def test_header_reproduces_the_published_known_answers(shim):
    out = subprocess.run([shim], capture_output=True, text=True, check=True).stdout.split('\n')
    assert out[:3] == [k[2] for k in KNOWN]


@pytest.mark.parametrize('seed,step,stream', TRIPLES)
def test_header_matches_the_restatement(shim, seed, step, stream):
    n = 300
    out = subprocess.run([shim, str(seed), str(step), str(stream), str(n)], capture_output=True, text=True, check=True).stdout
    rows = [l.split() for l in out.strip().split('\n')]
    assert len(rows) == n
    w = np.array([[int(x, 16) for x in r[:4]] for r in rows], dtype=np.uint32)
    z = np.array([[float(x) for x in r[4:]] for r in rows])
    assert np.array_equal(w, words(n, seed, step, stream))
    # two libm's on the same doubles: a few ulp of numbers up to 6.77
    assert np.abs(z - normals(n, seed, step, stream)).max() <= 1e-12
