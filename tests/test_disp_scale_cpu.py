"""No GPU: the fixed-point scale rules of the dispersion brick spreads (admp_amd/csrc/disp_math.h scalar_spread_exponent,
typed_spread_exponent -- the functions k_spread_bricks_scalar and k_spread_bricks_typed call), compiled for the host by
tests/hostshim/disp_scale_shim.cpp and walked over the entry count and the largest coefficient of a brick.  Asserted from the
header's own result:

* f32 tiles: 2^ex 0.17 bmax cnt < 2^30, so no sum of cnt terms leaves a 32-bit word;
* f64 tiles: 2^ex 0.17 bmax cnt < 2^62, and every term 2^ex 0.17 bmax < 2^50 -- the premise of the mantissa trick of
  scalar_fixed (disp_kernels.hip), which is exact for |v| < 2^51;
* the quantum 2^-ex is never coarser than tests/disp_mesh_ref.py's bars take it to be (quantum_f32 / quantum_f64 there), with
  the TRUE maximum of |c| in the bar and the kernel's float maximum x 1.0001f in the rule.

cnt: every value 1 .. 5000 (the chunk sizes 2048 and 3072 and their neighbours among them); bmax: 1e-30 .. 1e30, the exact
powers of two in that range with both float neighbours, and random values in between."""
import ctypes
import os
import subprocess

import numpy as np

from tests import disp_mesh_ref as D

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostshim', 'disp_scale_shim.cpp')
LIB = os.path.join(HERE, 'hostshim', 'libadmp_dispscaleshim.so')
HDRS = [os.path.join(os.path.dirname(HERE), 'admp_amd', 'csrc', h) for h in ('disp_math.h', 'pme_math.h')]
_lib = None


def slib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in [SRC] + HDRS):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC])
        _lib = ctypes.CDLL(LIB)
    return _lib


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def grid():
    rng = np.random.default_rng(11)
    p2 = np.float32(2.0) ** np.arange(-99, 100, dtype=np.float32)
    vals = np.concatenate([p2, np.nextafter(p2, np.float32(0)), np.nextafter(p2, np.float32(np.inf)),
                           (10.0 ** rng.uniform(-30, 30, 150)).astype(np.float32),
                           np.array([1e-30, 1e30, 1.0, 0.17, 1.0 / 0.17], dtype=np.float32)])
    assert vals.min() <= 1e-30 and vals.max() >= 1e30
    cnt = np.arange(1, 5001, dtype=np.int32)
    assert {2047, 2048, 2049, 3071, 3072, 3073} <= set(cnt.tolist())
    c, n = np.meshgrid(vals, cnt, indexing='ij')
    return np.ascontiguousarray(c.reshape(-1)), np.ascontiguousarray(n.reshape(-1))


def scalar_rule(single):
    cmax, cnt = grid()
    ex = np.zeros(len(cmax), dtype=np.int32)
    bmax = np.zeros(len(cmax), dtype=np.float64)
    slib().disp_scale_scalar(int(single), len(cmax), P(cmax), P(cnt), P(ex), P(bmax))
    return cmax.astype(np.float64), cnt.astype(np.float64), ex.astype(np.float64), bmax


def test_f32_words_cannot_overflow_and_quantum_is_within_the_bar():
    cmax, cnt, ex, bmax = scalar_rule(True)
    assert (bmax >= cmax).all()                                      # the rule's maximum is no smaller than the true one
    word = ex + np.log2(0.17 * bmax * cnt)                           # log2 of 2^ex 0.17 bmax cnt
    assert (word < 30).all(), word.max()
    quantum = 2.0 ** -ex
    assert (quantum <= D.quantum_f32(cmax, cnt)).all()
    print('f32: largest log2 word bound %.6f, largest quantum / bar quantum %.6f' % (word.max(), (quantum / D.quantum_f32(cmax, cnt)).max()))


def test_f64_words_and_terms_keep_their_bounds_and_quantum_is_within_the_bar():
    cmax, cnt, ex, bmax = scalar_rule(False)
    word = ex + np.log2(0.17 * bmax * cnt)
    term = ex + np.log2(0.17 * bmax)
    assert (word < 62).all(), word.max()
    assert (term < 50).all(), term.max()
    assert (ex <= 60).all()
    quantum = 2.0 ** -ex
    assert (quantum <= D.quantum_f64(cmax, cnt)).all()
    print('f64: largest log2 word bound %.6f, term bound %.6f, largest quantum / bar quantum %.6f'
          % (word.max(), term.max(), (quantum / D.quantum_f64(cmax, cnt)).max()))


def test_zero_brick_takes_exponent_20():
    cnt = np.array([0, 1, 600, 5000], dtype=np.int32)
    zero = np.zeros(4, dtype=np.float32)
    for single in (0, 1):
        ex = np.zeros(4, dtype=np.int32)
        bmax = np.zeros(4, dtype=np.float64)
        slib().disp_scale_scalar(single, 4, P(zero), P(cnt), P(ex), P(bmax))
        assert (ex == 20).all() and (bmax == 0).all()


def test_typed_rule():
    cnt = np.arange(0, 5001, dtype=np.int32)
    ex = np.zeros(len(cnt), dtype=np.int32)
    slib().disp_scale_typed(1, len(cnt), P(cnt), P(ex))
    n = np.maximum(cnt, 1).astype(np.float64)
    word = ex + np.log2(0.17 * n)
    assert (word < 30).all()
    assert (2.0 ** -ex.astype(np.float64) <= D.quantum_typed('single', n)).all()
    slib().disp_scale_typed(0, len(cnt), P(cnt), P(ex))
    assert (ex == 49).all()                                          # unit sources: every term below 2^49 0.17 < 2^50
    assert (49 + np.log2(0.17 * n) < 62).all()
    assert (2.0 ** -49 <= D.quantum_typed('double', n)).all()
