"""The lattice translation of the bonded box gradient (admp_amd/csrc/md_kernels.hip k_md_bonded_box: image_shift and min_image of
csrc/pme_math.h) without a GPU: the header compiled by the host compiler into a stand-alone program (tests/md_shift_shim/main.cpp),
with a bond across each face and across a corner of a triclinic cell.  For a bond of two atoms wrapped into the cell the raw
vector is the true one plus n . box with integer n; image_shift must return exactly that translation (shift = d_min - d_raw is
its negative), min_image the true vector, and a bond inside the cell must report no crossing and a translation of exactly zero
-- what makes the box gradient of an unwrapped configuration vanish identically."""
import itertools
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_md_random_cpu import CSRC, ROOT

SHIM = ROOT + '/tests/md_shift_shim/main.cpp'
BOX = np.array([[12.4, 0.0, 0.0], [0.9, 12.1, 0.0], [-0.6, 0.7, 12.7]])
BOND = np.array([0.61, -0.52, 0.53])                      # |d| = 0.96 A, no component zero
FACES = [n for n in itertools.product((-1, 0, 1), repeat=3) if sum(map(abs, n)) == 1]
CORNERS = [(1, 1, 1), (-1, 1, -1), (1, -1, 0)]            # two corners and an edge


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the header cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('md_shift_shim') / 'md_shift_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I', CSRC, '-o', exe, SHIM])
    return exe


def run(shim, prec, box, d):
    out = subprocess.run([shim, prec] + ['%.17g' % x for x in list(box.ravel()) + list(d)], capture_output=True, text=True,
                         check=True).stdout.split()
    return int(out[0]), np.array([float(x) for x in out[1:4]]), np.array([float(x) for x in out[4:7]])


@pytest.mark.parametrize('prec,eps', [('d', 2.0 ** -52), ('f', 2.0 ** -23)])
@pytest.mark.parametrize('n', FACES + CORNERS)
def test_shift_across_faces_and_corners(shim, prec, eps, n):
    """the second atom wrapped through the face(s) n: raw = true + n . box; a few roundings of numbers up to the box length"""
    lattice = np.asarray(n, dtype=np.float64) @ BOX
    crosses, sh, dmin = run(shim, prec, BOX, BOND + lattice)
    tol = 8 * eps * np.abs(BOX).max()
    assert crosses == 1
    assert np.abs(sh - lattice).max() <= (0.0 if prec == 'd' else tol)      # n . box with integer n: exact in double
    assert np.abs(dmin - BOND).max() <= tol
    assert np.abs((dmin - (BOND + lattice)) + sh).max() <= tol              # shift = d_min - d_raw = -sh


@pytest.mark.parametrize('prec', ['d', 'f'])
def test_no_shift_inside_the_cell(shim, prec):
    crosses, sh, dmin = run(shim, prec, BOX, BOND)
    assert crosses == 0 and not sh.any()
    assert np.abs(dmin - BOND).max() <= 8 * (2.0 ** -52 if prec == 'd' else 2.0 ** -23) * np.abs(BOX).max()
