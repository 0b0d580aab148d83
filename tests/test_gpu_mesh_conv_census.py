"""Which kernels one admp_mesh_convolve launches on every path of the mesh convolution (admp_amd/csrc/mesh_conv.hip), by
label and count, against a table written here from the code: the orchestration of the k-space leg, pinned so that moving its
host code shows.  One child process per set of switches (they are read once per process), the profiler on, two calls per
type on the smallest mesh of each path that tests/test_gpu_mesh_convolve.py uses: the G table (and, on the direct forms, the
circulant table) is built by the first call only.  info[0] must be the word of the path the CPU rule
(tests/test_mesh_path_cpu.py `restated`, the facts of the kernel files given here) names for that input."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORD = {'Rocfft3D': 0, 'FusedX': 1, 'DirectLines': 2, 'DirectPlanes': 3, 'TwoLevel': 4}      # ADMP_MESH_PATH_*
CALLS = 2
LINES = ('dft_z_r2c', 'dft_y_fwd', 'dft_x_kspace', 'dft_y_inv', 'dft_z_c2r')
# per call / on the first call only
CENSUS = {
    'Rocfft3D': (('rocfft_r2c', 'kspace', 'rocfft_c2r'), ('gtab',)),
    'FusedX': (('rocfft_r2c_yz', 'fftx_kspace', 'rocfft_c2r_yz'), ('gtab',)),
    'DirectPlanes': (('dft_zy_fwd', 'dft_x_kspace', 'dft_yz_inv'), ('gtab', 'xcirc_table')),
    'DirectLines': (LINES, ('gtab', 'xcirc_table')),
    'TwoLevel': (LINES, ('gtab',)),
}
SMALL_DIRECT = (2, 3, 160)       # smooth: direct only when ADMP_DFT=1 asks; its planes fit the LDS in both types
# name, switches, [(K, facts of the kernel files: splits (pfa_split of every axis), zy_fits (dft_zy_fits))]
CHILDREN = [
    ('direct_planes', {'ADMP_DFT': '1'}, [(SMALL_DIRECT, dict(splits=1, zy_fits=1))]),
    ('direct_lines', {'ADMP_DFT': '1', 'ADMP_DFT_PLANES': '0'}, [(SMALL_DIRECT, dict(splits=1, zy_fits=0))]),
    # 254 = 2 * 127, 35 = 5 * 7, 7: with ADMP_PFA_MIN=0 every axis goes through pfa_split's factorisation
    ('two_level', {'ADMP_DFT': '2', 'ADMP_PFA_MIN': '0'}, [((254, 35, 7), dict(splits=1, zy_fits=0))]),
    ('default', {}, [((32, 33, 36), dict(splits=1, zy_fits=1)), (SMALL_DIRECT, dict(splits=1, zy_fits=1))]),
]
SWITCHES = ('ADMP_DFT', 'ADMP_DFT_PLANES', 'ADMP_DFT_XCIRC', 'ADMP_PFA', 'ADMP_PFA_MIN', 'ADMP_FUSED_X')


def expected_path(K, switches, facts):
    from tests.test_mesh_path_cpu import fftx_usable, restated
    return restated(K[0], K[1], K[2], 1, int(switches.get('ADMP_DFT', -1)), 1, 1, int(fftx_usable(K[0])), facts['splits'],
                    facts['zy_fits'])


def child_main(meshes_json):
    import ctypes

    import numpy as np
    import torch                             # before the library, as everywhere else: one HIP runtime per process, torch's
    torch.cuda.init()
    from admp_amd import _lib
    L = _lib.load()
    out = []
    for K in json.loads(meshes_json):
        for prec in (4, 8):
            h = ctypes.c_void_p()
            assert L.admp_create(ctypes.byref(h), 0, prec) == 0
            _lib.check(h, L.admp_set_ewald(h, 0.7, K[0], K[1], K[2], 2, 0), 'admp_set_ewald')
            _lib.check(h, L.admp_profile_enable(h, 1), 'admp_profile_enable')
            box = _lib.darr(np.diag([0.32 * k for k in K]))
            rng = np.random.default_rng(sum(K))
            info = (ctypes.c_int * _lib.MESH_INFO_WORDS)()
            for _ in range(CALLS):
                x = rng.standard_normal(K).astype(np.float32 if prec == 4 else np.float64)
                E = ctypes.c_double(0.0)
                _lib.check(h, L.admp_mesh_convolve(h, box, 1, x.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(E), info),
                           'admp_mesh_convolve')
                assert np.isfinite(x).all() and np.isfinite(E.value)
            seen = {}
            for k in range(L.admp_profile_count(h)):
                label, ms, count = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int64()
                _lib.check(h, L.admp_profile_entry(h, k, ctypes.byref(label), ctypes.byref(ms), ctypes.byref(count)),
                           'admp_profile_entry')
                seen[label.value.decode()] = int(count.value)
            out.append(dict(K=list(K), prec=prec, info0=int(info[0]), seen=seen))
            assert L.admp_destroy(h) == 0
    print('CENSUS ' + json.dumps(out))


@pytest.mark.gpu
@pytest.mark.parametrize('name,switches,meshes', CHILDREN, ids=[c[0] for c in CHILDREN])
def test_launch_census_of_one_convolution(name, switches, meshes):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'child', json.dumps([K for K, _ in meshes])], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('CENSUS ')]
    assert len(line) == 1, r.stdout[-2000:]
    got = json.loads(line[0][7:])
    assert [(tuple(g['K']), g['prec']) for g in got] == [(K, p) for K, _ in meshes for p in (4, 8)]
    for g in got:
        facts = dict(meshes)[tuple(g['K'])]
        path = expected_path(tuple(g['K']), switches, facts)
        print(name, g['K'], g['prec'], path, g['info0'], g['seen'])
        per_call, once = CENSUS[path]
        want = {lab: CALLS for lab in per_call}
        want.update({lab: 1 for lab in once})
        assert g['seen'] == want, (name, g['K'], g['prec'], path)
        assert g['info0'] == WORD[path], (name, g['K'], g['prec'], path)


def test_the_children_cover_every_single_rank_path():
    paths = {expected_path(K, sw, f) for _, sw, meshes in CHILDREN for K, f in meshes}
    assert paths == set(WORD)


if __name__ == '__main__' and len(sys.argv) == 3 and sys.argv[1] == 'child':
    child_main(sys.argv[2])
