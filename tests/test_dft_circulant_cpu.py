"""The x pass of the direct-DFT convolution as one real circulant product per line (admp_amd/csrc/dft_math.h:
circ_table_entry, circ_column_even, circ_pair_outputs, circ_pair_energy), host-compiled, against numpy.fft.

Error bounds (u = unit roundoff of the kernel's type T, gamma = (N + 4) u; re and im parts separately, c is real):

* table.  c[d] = G(0) + sum_{k=1..H} (G(k) + G(N-k)) cos(2 pi k d / N) [+ (-1)^d G(N/2)] is summed in double and rounded
  to T once.  A recursive sum of n terms has |err| <= (n - 1) u' sum|terms| (u' = 2^-53); every term carries one more
  rounding from its product, one from the pair sum and <= 2 u' of absolute cosine error, and |cos| <= 1, so with
  n = H + 2 <= N/2 + 2 the sum is within (N/2 + 6) u' sum|G| and the stored value within that plus u |c| <= u sum|G|:
  |dc[d]| <= gamma sum|G|.
* product.  out_i = sum_j c[i-j] x_j is the standard dot product of N terms, |err| <= gamma sum_j |c[i-j]| |x_j| to first
  order (N - 1 additions, one product rounding; the pair sums a_j, b_j, the sums c[i-j] +- c[i+j] and the final (P +- M) / 2
  are the four roundings that "+ 4" stands for).  The table error adds |sum_j dc[i-j] x_j| <= gamma sum|G| sum_j |x_j|.
  Together: |err_i| <= gamma (sum|G| sum_j|x_j| + sum_j |c[i-j]| |x_j|).
* energy.  sum_x Re(conj(in_x) out_x) is summed in double from the T values: |err| <= sum_x |in_x| |err(out_x)| (the bound
  above) + (N + 4) 2^-53 sum_x |in_x| |out_x|.

numpy.fft's own error (O(log N) 2^-53 in norm) is far below these and is not added.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostshim', 'circ_shim.cpp')
LIB = os.path.join(HERE, 'hostshim', 'libadmp_circshim.so')
CSRC = os.path.join(os.path.dirname(HERE), 'admp_amd', 'csrc')

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC])
        _lib = ctypes.CDLL(LIB)
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def even_G(rng, N):
    """positive, even in k, spread over ten decades like the Ewald factor between k = 1 and the mesh edge"""
    half = 10.0 ** rng.uniform(-8.0, 2.0, N // 2 + 1)
    G = np.empty(N)
    for k in range(N):
        G[k] = half[min(k, N - k)]
    return G


def table(f32, G):
    N = len(G)
    c = np.zeros(N // 2 + 1)
    ok = lib().circ_table(int(f32), N, _p(np.ascontiguousarray(G)), _p(c))
    return c, bool(ok)


def apply(f32, c, x):
    N = len(x)
    xi = np.ascontiguousarray(np.stack([x.real, x.imag], axis=1))
    out = np.zeros((N, 2))
    e = ctypes.c_double(0.0)
    lib().circ_apply(int(f32), N, _p(np.ascontiguousarray(c)), _p(xi), _p(out), ctypes.byref(e))
    return out[:, 0] + 1j * out[:, 1], e.value


@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('N', [97, 31, 64, 34, 100])
def test_circulant_line_vs_numpy_fft(N, f32):
    rng = np.random.default_rng(1000 * N + int(f32))
    rt = np.float32 if f32 else np.float64
    u = 2.0 ** -24 if f32 else 2.0 ** -53
    gamma = (N + 4) * u
    for trial in range(4):
        G = even_G(rng, N).astype(rt).astype(np.float64)           # what the kernels see: values of type T
        x = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * 10.0 ** rng.uniform(-2, 2, N)
        x = x.real.astype(rt).astype(np.float64) + 1j * x.imag.astype(rt).astype(np.float64)
        c, ok = table(f32, G)
        assert ok
        S = np.fft.fft(x)
        ref = np.fft.ifft(G * S) * N
        e_ref = float(np.sum(G * np.abs(S) ** 2))
        c_ref = (np.fft.ifft(G) * N).real                             # first column of the circulant
        sumG = float(np.sum(np.abs(G)))
        # table
        dc = np.abs(c - c_ref[:N // 2 + 1])
        print('N=%d f32=%d table err/bound %.3g' % (N, f32, dc.max() / (gamma * sumG)))
        assert np.all(dc <= gamma * sumG)
        # product
        out, e = apply(f32, c, x)
        idx = (np.arange(N)[:, None] - np.arange(N)[None, :]) % N
        C = np.abs(c_ref)[idx]
        e_bound = 0.0
        for part in ('real', 'imag'):
            xa = np.abs(getattr(x, part))
            bound = gamma * (sumG * xa.sum() + C @ xa)
            err = np.abs(getattr(out, part) - getattr(ref, part))
            print('N=%d f32=%d %s err/bound %.3g' % (N, f32, part, (err / bound).max()))
            assert np.all(err <= bound)
            e_bound += float(np.sum(xa * bound)) + (N + 4) * 2.0 ** -53 * float(np.sum(xa * np.abs(getattr(ref, part))))
        print('N=%d f32=%d energy err/bound %.3g' % (N, f32, abs(e - e_ref) / e_bound))
        assert abs(e - e_ref) <= e_bound


@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('N', [97, 64])
def test_uneven_column_is_reported(N, f32):
    rng = np.random.default_rng(7 + N)
    rt = np.float32 if f32 else np.float64
    u = 2.0 ** -24 if f32 else 2.0 ** -53
    G = even_G(rng, N).astype(rt).astype(np.float64)
    assert table(f32, G)[1]
    # one ulp on the smallest entry of one side: far inside the bound (8 u max|G|), still valid
    k = 1 + int(np.argmin(G[1:(N - 1) // 2 + 1]))
    G1 = G.copy()
    G1[k] = float(np.nextafter(rt(G1[k]), rt(np.inf)))
    assert table(f32, G1)[1]
    # 32 u max|G| on one side: not even
    G2 = G.copy()
    G2[N - k] += 32.0 * u * G.max()
    assert float(rt(G2[N - k])) - G[k] > 8.0 * u * G.max()
    assert not table(f32, G2)[1]
