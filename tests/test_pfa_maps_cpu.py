"""Index maps of the two-level (Good-Thomas) direct DFT (admp_amd/csrc/pfa_maps.h: pfa_split_at, pfa_pos, pfa_index_table,
pfa_freq_of_slot, pfa_freq_of_zcolumn), host-compiled, for every length from 2 to 32 * 160.

What the kernels of pfa_kernels.hip rely on, asserted for each length that splits, with plain_max = 0 (ADMP_PFA_MIN=0: split
whatever can be split) and plain_max = 160 (the default):

* N = N1 N2 with gcd(N1, N2) = 1, N1 <= 32, N2 <= 160; the split is the one the header documents (N2 the power of the
  largest prime, whole below plain_max), recomputed here independently; lengths without a usable split return false;
* (n1, n2) -> position is a bijection of 0 .. N-1, and the packed table carries n1 in its upper half;
* the frequency f stored at slot pos(k1, k2) satisfies f = k1 (mod N1), f = k2 (mod N2), and f is a bijection;
* the stored z columns (k1, k2 <= N2/2) and their negatives cover every frequency, and with weight 1/2 on the self-paired
  columns (k2 = 0, and k2 = N2/2 for even N2) the half sum equals half the full sum for any even g -- the energy weights
  of k_pfa_x_conv.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostshim', 'pfa_shim.cpp')
LIB = os.path.join(HERE, 'hostshim', 'libadmp_pfashim.so')
CSRC = os.path.join(os.path.dirname(HERE), 'admp_amd', 'csrc')
N_MAX = 32 * 160

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC])
        _lib = ctypes.CDLL(LIB)
    return _lib


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def split(N, plain_max):
    out = np.zeros(3, dtype=np.int32)
    ok = lib().pfa_shim_split(N, plain_max, _ip(out))
    return (int(out[1]), int(out[2])) if ok else None


def expected_split(N, plain_max):
    """N2 = the power of the largest prime factor, N1 the cofactor; whole up to plain_max; None: not usable."""
    p, m = 1, N
    q = 2
    while q * q <= m:
        while m % q == 0:
            p, m = q, m // q
        q += 1
    if m > 1:
        p = m
    N2 = 1
    m = N
    while m % p == 0:
        N2, m = N2 * p, m // p
    N1 = m
    if N <= plain_max or N1 == 1:
        N1, N2 = 1, N
    return (N1, N2) if (N1 <= 32 and 2 <= N2 <= 160) else None


def tables(N, N1, N2):
    t = np.zeros(N, dtype=np.int32)
    f = np.zeros(N, dtype=np.int32)
    fz = np.zeros(N1 * (N2 // 2 + 1), dtype=np.int32)
    lib().pfa_shim_index_table(N, N1, N2, _ip(t))
    lib().pfa_shim_freq_of_slot(N, N1, N2, _ip(f))
    lib().pfa_shim_freq_of_zcolumn(N, N1, N2, _ip(fz))
    return t, f, fz


@pytest.mark.parametrize('plain_max', [0, 160])
def test_two_level_index_maps_every_length(plain_max):
    rng = np.random.default_rng(160 + plain_max)
    n_split = n_whole = n_refused = 0
    seen_n1 = set()
    for N in range(2, N_MAX + 1):
        got, want = split(N, plain_max), expected_split(N, plain_max)
        assert got == want, (N, got, want)
        if got is None:
            n_refused += 1
            continue
        N1, N2 = got
        assert N1 * N2 == N and math.gcd(N1, N2) == 1 and 1 <= N1 <= 32 and 2 <= N2 <= 160, (N, N1, N2)
        if N1 == 1:
            n_whole += 1
        else:
            n_split += 1
            seen_n1.add(N1)
        t, f, fz = tables(N, N1, N2)
        n1, n2 = np.divmod(np.arange(N), N2)                   # row index n1 * N2 + n2
        pos = t & 0xffff
        assert np.array_equal(t >> 16, n1), N
        assert np.array_equal(pos, (N2 * n1 + N1 * n2) % N), N
        assert np.array_equal(np.sort(pos), np.arange(N)), N   # bijection
        # the frequency stored at slot pos(k1, k2)
        fk = f[pos]
        assert np.array_equal(fk % N1, n1) and np.array_equal(fk % N2, n2), N
        assert np.array_equal(np.sort(f), np.arange(N)), N
        # stored z half: column cz = k2 * N1 + k1, k2 <= N2 / 2
        k2, k1 = np.divmod(np.arange(fz.size), N1)
        assert np.array_equal(fz % N1, k1) and np.array_equal(fz % N2, k2), N
        assert fz.min() >= 0 and fz.max() < N
        cover = np.zeros(N, dtype=np.int64)
        np.add.at(cover, fz, 1)
        selfp = (k2 == 0) | (2 * k2 == N2)
        np.add.at(cover, (N - fz[~selfp]) % N, 1)
        # self-paired columns: their negatives are stored columns too, (-k1, k2) -- counted once each above
        assert np.array_equal(np.sort((N - fz[selfp]) % N), np.sort(fz[selfp])), N
        assert np.all(cover == 1), (N, np.nonzero(cover != 1)[0][:8])
        # energy weights: 1/2 on the self-paired columns
        half = rng.uniform(0.5, 2.0, N // 2 + 1)
        g = half[np.minimum(np.arange(N), N - np.arange(N))]   # even in k
        w = np.where(selfp, 0.5, 1.0)
        lhs, rhs = float(np.sum(w * g[fz])), 0.5 * float(np.sum(g))
        assert abs(lhs - rhs) <= 4 * N * 2.0 ** -53 * rhs, (N, lhs, rhs)
    print('plain_max=%d: %d split, %d whole, %d refused; N1 seen: %s' % (plain_max, n_split, n_whole, n_refused,
                                                                         sorted(seen_n1)))
    assert n_split > 0 and n_refused > 0
    if plain_max == 0:
        assert seen_n1 == set(range(2, 33)), sorted(seen_n1)


def test_pos_function_and_named_lengths():
    # pfa_pos itself (the kernels call it on the device) on a sample
    for N1, N2 in ((5, 61), (8, 157), (32, 3), (7, 17), (1, 97)):
        N = N1 * N2
        for n1 in range(N1):
            for n2 in range(0, N2, 7):
                assert lib().pfa_shim_pos(N, N1, N2, n1, n2) == (N2 * n1 + N1 * n2) % N
    # the lengths the engine is known to meet, and ones it must refuse
    assert split(305, 160) == (5, 61) and split(305, 0) == (5, 61)
    assert split(170, 160) == (10, 17) and split(183, 160) == (3, 61)
    assert split(97, 160) == (1, 97) and split(96, 160) == (1, 96) and split(96, 0) == (32, 3)
    assert split(160, 160) == (1, 160) and split(160, 0) == (32, 5)
    assert split(163, 160) is None and split(163, 0) is None          # a prime above 160
    assert split(2 * 163, 0) is None and split(165, 160) == (15, 11)  # N2 too long; 165 = 15 * 11 is fine
    assert split(33 * 37, 0) is None                                  # cofactor 33 > 32
    assert split(169, 0) is None and split(2 * 169, 160) is None      # 13^2 = 169 > 160
