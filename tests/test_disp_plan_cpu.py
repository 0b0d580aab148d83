"""The path choice of a dispersion PME call (admp_amd/csrc/disp_plan.h `disp_path`) without a GPU: the header compiled by the
host compiler into a stand-alone program (tests/disp_shim/main.cpp) against a Python restatement of the conditions, written as
the nested ifs of the engine's `disp` before the choice became a function, over the WHOLE input space (6144 rows); and the same
program built with the address and undefined-behaviour sanitizers.  tests/test_gpu_disp_paths.py pins the paths on the GPU."""
import itertools
import shutil
import subprocess

import pytest

from tests.test_md_random_cpu import CSRC, ROOT

SHIM = ROOT + '/tests/disp_shim/main.cpp'
FIELDS = ('snranks', 'use_dft', 'use_pfa', 'use_fx', 'bricks', 'single_precision', 'nch', 'disp_nt', 'have_types', 'types_on',
          'batch_on')


def restated(snranks, use_dft, use_pfa, use_fx, bricks, single_precision, nch, disp_nt, have_types, types_on, batch_on):
    fused = not (use_dft or use_pfa) and (snranks > 1 or bricks)
    if fused:
        typed = types_on and batch_on and snranks == 1 and use_fx and single_precision and disp_nt >= 1 and disp_nt <= nch \
            and have_types
        if typed:
            return 'BricksTyped'
        if batch_on and snranks == 1 and use_fx and nch >= 2:
            return 'BricksBatched'
        return 'BricksPerPower'
    if types_on and disp_nt >= 1 and disp_nt < nch and have_types and use_dft and not use_pfa and snranks == 1 and not bricks:
        return 'DftTyped'
    if (use_dft or use_pfa) and nch > 1:
        return 'DftBatched'
    return 'PerPower'


def rows():
    b = (0, 1)
    return list(itertools.product((1, 2), b, b, b, b, b, (1, 2, 3), (0, 1, 2, 3), b, b, b))


def build(tmp_path_factory, name, flags):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the header cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, '-o', exe, SHIM] + flags)
    return exe


def check_every_row(exe):
    rs = rows()
    assert len(rs) == 6144
    text = ''.join(' '.join(map(str, r)) + '\n' for r in rs)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert len(got) == len(rs)
    bad = [(dict(zip(FIELDS, r)), g, restated(*r)) for r, g in zip(rs, got) if g != restated(*r)]
    assert not bad, bad[:5]
    return got


def test_every_input_against_the_restatement(tmp_path_factory):
    got = check_every_row(build(tmp_path_factory, 'disp_shim', ['-O2']))
    assert set(got) == {'BricksTyped', 'BricksBatched', 'BricksPerPower', 'DftTyped', 'DftBatched', 'PerPower'}


def test_the_asymmetry_of_the_type_counts():
    """as many types as powers: the brick form still takes the types, the direct-DFT form keeps the powers"""
    common = dict(snranks=1, use_pfa=0, single_precision=1, have_types=1, types_on=1, batch_on=1)
    for n in (2, 3):
        assert restated(use_dft=0, use_fx=1, bricks=1, nch=n, disp_nt=n, **common) == 'BricksTyped'
        assert restated(use_dft=1, use_fx=0, bricks=0, nch=n, disp_nt=n, **common) == 'DftBatched'
        assert restated(use_dft=1, use_fx=0, bricks=0, nch=n, disp_nt=n - 1, **common) == 'DftTyped'


def test_under_the_sanitizers(tmp_path_factory):
    check_every_row(build(tmp_path_factory, 'disp_shim_san', ['-O1', '-g', '-fsanitize=address,undefined',
                                                             '-fno-sanitize-recover=all']))
