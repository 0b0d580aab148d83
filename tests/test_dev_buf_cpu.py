"""The owning device buffer (admp_amd/csrc/dev_buf.h) without a GPU: the real header, compiled by the host compiler against a
counting stand-in for the HIP runtime (tests/devbuf_shim/hip/hip_runtime.h) into a stand-alone program (tests/devbuf_shim/main.cpp)
that states each property of the buffer; built and run plainly, and once more under the address and undefined-behaviour
sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, 'tests', 'devbuf_shim')
CSRC = os.path.join(ROOT, 'admp_amd', 'csrc')
PROPERTIES = ['starts empty', 'need allocates', 'a smaller or equal request keeps the allocation', 'a larger request grows',
              'as<U> is the pointer', 'a failed hipMalloc throws and leaves {nullptr, 0}', 'release twice is harmless',
              'a released buffer can be used again', 'scope exit frees', 'an exception between need and the end of scope frees',
              'a struct holds two allocations', 'a struct of two buffers frees both',
              'nothing live at exit, every free was of a live allocation']


@pytest.mark.parametrize('flags', [(), ('-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g')],
                         ids=['plain', 'sanitized'])
def test_dev_buf(tmp_path, flags):
    """every property line reads ok, none is missing, and the program (the copy check is a static_assert in it) exits clean"""
    if shutil.which('g++') is None:
        pytest.skip('no host compiler')
    exe = str(tmp_path / 'devbuf_shim')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', '-Wextra', '-Werror', *flags, '-I', SHIM, '-I', CSRC, '-o', exe,
                           os.path.join(SHIM, 'main.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.stdout.splitlines() == ['ok ' + p for p in PROPERTIES]
    assert r.returncode == 0 and r.stderr == ''
