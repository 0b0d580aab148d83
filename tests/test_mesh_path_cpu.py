"""The path choice of the mesh convolution (admp_amd/csrc/mesh_path.h `mesh_path`) without a GPU: the header compiled by the
host compiler into a stand-alone program (tests/mesh_path_shim/main.cpp) against a Python restatement of the rule, written as
the flags of the engine's `ensure_mesh`, `setup_dft` and `setup_pfa` and the order in which `convolve` tested them before the
choice became a function.  The walk takes ALL 12^3 mesh triples of the twelve lengths below times the five booleans, the four
modes of ADMP_DFT and one rank or three: 442 368 rows, a few seconds.  The same program runs under the address and
undefined-behaviour sanitizers on every 17th row.  tests/test_gpu_mesh_conv_census.py pins the paths on the GPU."""
import itertools
import shutil
import subprocess

import pytest

from tests.test_md_random_cpu import CSRC, ROOT

SHIM = ROOT + '/tests/mesh_path_shim/main.cpp'
FIELDS = ('K0', 'K1', 'K2', 'snranks', 'dft_mode', 'pfa_on', 'fused_x_on', 'fftx_ok', 'splits', 'zy_fits')
LENGTHS = (6, 32, 45, 96, 97, 128, 160, 161, 183, 305, 508, 1024)
SINGLE = {'Rocfft3D', 'FusedX', 'DirectPlanes', 'DirectLines', 'TwoLevel'}
SLAB = {'SlabRocfftX', 'SlabFusedX'}


def largest_prime_factor(n):
    p, best = 2, 1
    while p * p <= n:
        while n % p == 0:
            best, n = p, n // p
        p += 1
    return max(best, n) if n > 1 else best


def fftx_usable(n):
    """fftx_kernels.hip: a power of two from 32 to 1024"""
    return 32 <= n <= 1024 and n & (n - 1) == 0


def restated(K0, K1, K2, snranks, dft_mode, pfa_on, fused_x_on, fftx_ok, splits, zy_fits):
    K = (K0, K1, K2)
    # ensure_mesh: the twiddles of the fused x pass are uploaded (use_fx) on one rank and on a slab rank alike
    use_fx = bool(fused_x_on and fftx_ok)
    use_dft = use_pfa = False
    # setup_dft, with setup_pfa where it called it
    if snranks == 1 and dft_mode != 0:
        small = all(2 <= k <= 160 for k in K)
        hard = any(largest_prime_factor(k) > 13 for k in K)
        pfa_taken = bool(pfa_on and splits)
        if dft_mode == 2 and pfa_taken:
            use_pfa = True
        elif not small and hard and pfa_taken:
            use_pfa = True
        elif not small or not (hard or dft_mode == 1 or dft_mode == 2):
            pass
        else:
            use_dft = True
    # convolve: slab ranks first, then the flags in this order
    if snranks > 1:
        return 'SlabFusedX' if use_fx else 'SlabRocfftX'
    if use_pfa:
        return 'TwoLevel'
    if use_dft:
        return 'DirectPlanes' if zy_fits else 'DirectLines'
    return 'FusedX' if use_fx else 'Rocfft3D'


def rows():
    b = (0, 1)
    return [K + r for K in itertools.product(LENGTHS, repeat=3) for r in itertools.product((1, 3), (-1, 0, 1, 2), b, b, b, b, b)]


def build(tmp_path_factory, name, flags):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the header cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, '-o', exe, SHIM] + flags)
    return exe


def run_rows(exe, rs):
    text = ''.join(' '.join(map(str, r)) + '\n' for r in rs)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert len(got) == len(rs)
    return got


def check_rows(exe, rs):
    got = run_rows(exe, rs)
    bad = [(dict(zip(FIELDS, r)), g, restated(*r)) for r, g in zip(rs, got) if g != restated(*r)]
    assert not bad, bad[:5]
    return got


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    return build(tmp_path_factory, 'mesh_path_shim', ['-O2'])


def test_every_input_against_the_restatement(shim):
    rs = rows()
    assert len(rs) == 12 ** 3 * 2 * 4 * 32 == 442368
    got = check_rows(shim, rs)
    assert set(got) == SINGLE | SLAB
    # a slab input never takes a single-rank path, and the reverse
    for r, g in zip(rs, got):
        assert (g in SLAB) == (r[3] > 1), (r, g)


def path_of(shim, K, snranks=1, dft_mode=-1, pfa_on=1, fused_x_on=1, splits=0, zy_fits=1):
    r = tuple(K) + (snranks, dft_mode, pfa_on, fused_x_on, int(fftx_usable(K[0])), splits, zy_fits)
    got = run_rows(shim, [r])[0]
    assert got == restated(*r)
    return got


def test_the_documented_meshes(shim):
    """the meshes DESIGN.md names, with the facts the kernel files give for them"""
    assert path_of(shim, (97, 97, 97), zy_fits=1) == 'DirectPlanes'
    assert path_of(shim, (97, 97, 97), zy_fits=0) == 'DirectLines'
    # 305 = 5 * 61, 170 = 10 * 17, 183 = 3 * 61: every dimension splits
    assert path_of(shim, (305, 170, 183), splits=1, zy_fits=0) == 'TwoLevel'
    assert path_of(shim, (256, 256, 256), zy_fits=0) == 'FusedX'
    assert path_of(shim, (128, 128, 128)) == 'FusedX'
    assert path_of(shim, (96, 100, 45)) == 'Rocfft3D'
    assert path_of(shim, (36, 33, 22), snranks=2) == 'SlabRocfftX'
    assert path_of(shim, (32, 7, 20), snranks=5) == 'SlabFusedX'


def test_the_switches(shim):
    b = (0, 1)
    rs = [K + (n, 0) + r for K in itertools.product((32, 97, 161, 305), repeat=3) for n in (1, 3)
          for r in itertools.product(b, b, b, b, b)]
    assert not {'DirectPlanes', 'DirectLines', 'TwoLevel'} & set(run_rows(shim, rs)), 'ADMP_DFT=0 took a direct form'
    rs = [K + (n, m, p, 0) + r for K in itertools.product((32, 97, 128, 305), repeat=3) for n in (1, 3) for m in (-1, 0, 1, 2)
          for p in b for r in itertools.product(b, b, b)]
    assert not {'FusedX', 'SlabFusedX'} & set(run_rows(shim, rs)), 'ADMP_FUSED_X=0 took the fused x pass'


def test_under_the_sanitizers(tmp_path_factory):
    check_rows(build(tmp_path_factory, 'mesh_path_shim_san', ['-O1', '-g', '-fsanitize=address,undefined',
                                                              '-fno-sanitize-recover=all']), rows()[::17])
