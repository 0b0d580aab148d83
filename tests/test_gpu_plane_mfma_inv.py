"""The matrix-core share of the inverse plane kernel's y and z lines (k_dft_yz_inv<double, 2, true>, plane_mfma_plan.h,
ADMP_DFT_PLANE_MFMA_INV) against its vector form (ADMP_DFT_PLANE_MFMA_INV=0): one build, one process -- the switch is read per
launch, so the process sets it before every call.  The forward kernel keeps its share in both modes (ADMP_DFT_PLANE_MFMA is
left at its default), so only the inverse form differs.

Part 1, admp_mesh_convolve on white-noise meshes (each with a prime factor >= 17, so that the plane kernels run; asserted):
    (17, 37, 34)   y lines H = 18: masked rows, uneven groups      z lines H = 16, even: Nyquist term
    (19, 97, 38)   y lines H = 48: the workload's tiles            z lines H = 18, even, masked rows
    (23, 38, 97)   y lines H = 18, even: the N/2 row               z lines H = 48
    (29, 31, 17)   y lines H = 15, z lines H = 8: no share
    (17, 37, 19)   y lines H = 18: a share; z lines H = 9: none -- the vector z tasks read the matrix units' V
    (17, 19, 37)   y lines H = 9: none; z lines H = 18: a share -- the matrix units read the vector tasks' V
at the production and at a flat kappa, with the share on and off: both against the float64 FFT reference of
tests/test_gpu_mesh_convolve.py with its bounds for the direct path (check_case: word, energy and per-bin bound D), and the
on-against-off difference under the same word, per-bin and energy bounds.  admp_plane_mfma_stats4 must show the inverse
launch with a share on every mesh but the fourth, in the vector form everywhere with the switch off, and the same forward
launches in both modes.

Part 2, whole evaluations: 125 waters (375 atoms), polarizable, double precision, mesh (35, 37, 34) on the direct path (19
y groups split 5 + 5 / 4 + 4 pairs and the N/2 row of z), one sequence at the default SCF threshold and one at 1e-2 (the
increments of the SCF then run through the inverse kernel's accum path), as tests/test_gpu_plane_mfma.py runs them for the
forward share: two handles see the same inputs call by call.  Cycle counts, flags and SCF forms are equal; energy parts,
gradient and dipoles agree within TOL64 of tests/test_gpu_pair_rider.py, 1e3 * 2^-53 = 1.1e-13 of the largest entry.

Measured on an MI355X: largest bin err / D 1.2e-3 with the share and 1.3e-3 without it, word / B_word 1.2e-4 both, on - off at
most 3.3e-4 of D, 3.3e-5 of B_word and 8.4e-6 of B_E; whole evaluations: largest |on - off| / max|off| 2.4e-16 (energy parts),
2.2e-15 (gradient), 2.1e-15 (dipoles); inverse launches 8 + 16 with the share in A, as many without in B."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import test_gpu_mesh_convolve as M          # noqa: E402  (the reference and its bounds)
from tests.test_gpu_pair_rider import TOL64            # noqa: E402

# (K, the inverse launch carries a share)
MESHES = [((17, 37, 34), True), ((19, 97, 38), True), ((23, 38, 97), True), ((29, 31, 17), False), ((17, 37, 19), True),
          ((17, 19, 37), True)]
SWITCH = 'ADMP_DFT_PLANE_MFMA_INV'


def mesh_cases():
    out = []
    for K, share in MESHES:
        for kind in ('prod', 'flat'):
            kap = M.KAPPA_PROD if kind == 'prod' else M.kappa_flat(K, False, 1)
            out.append(dict(id='%dx%dx%d_%s' % (K + (kind,)), K=list(K), tric=False, prec=8, ref_order=0, which=1, kappa=kap, kind=kind,
                            input=dict(kind='noise', seed=2000 + sum(K)), share=share))
    return out


def child_mesh(cases_path, outdir):
    import torch                             # before the library, as everywhere else
    torch.cuda.init()
    from admp_amd import _lib
    L = _lib.load()
    cases = json.load(open(cases_path))
    results = {}
    for c in cases:
        K = tuple(c['K'])
        x = M.make_input(c)
        box = _lib.darr(M.make_box(K, False))
        for mode in ('1', '0'):
            os.environ[SWITCH] = mode
            h = ctypes.c_void_p()
            assert L.admp_create(ctypes.byref(h), 0, 8) == 0
            _lib.check(h, L.admp_set_ewald(h, float(c['kappa']), K[0], K[1], K[2], 2, 0), 'admp_set_ewald')
            E = ctypes.c_double(0.0)
            info = (ctypes.c_int * _lib.MESH_INFO_WORDS)()
            out = x.copy()
            _lib.check(h, L.admp_mesh_convolve(h, box, 1, out.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(E), info),
                       'admp_mesh_convolve')
            st = (ctypes.c_int64 * 4)()
            _lib.check(h, L.admp_plane_mfma_stats4(h, st, 0), 'admp_plane_mfma_stats4')
            np.save(os.path.join(outdir, '%s_%s.npy' % (c['id'], mode)), out)
            results['%s_%s' % (c['id'], mode)] = dict(E=E.value, info=list(info), stats=[int(v) for v in st])
            L.admp_destroy(h)
    json.dump(results, open(os.path.join(outdir, 'results.json'), 'w'))
    print('PLANE-MFMA-INV-MESH-OK')


@pytest.mark.gpu
def test_mesh_convolve_inverse_share_on_and_off(tmp_path):
    cases = mesh_cases()
    (tmp_path / 'cases.json').write_text(json.dumps(cases))
    env = {k: v for k, v in os.environ.items() if not k.startswith('ADMP_') or k == 'ADMP_HIP_LIB'}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'mesh', str(tmp_path / 'cases.json'), str(tmp_path)],
                       capture_output=True, text=True, env=dict(env, ADMP_DFT='1'), timeout=300, cwd=ROOT)
    assert r.returncode == 0 and 'PLANE-MFMA-INV-MESH-OK' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    res = json.load(open(tmp_path / 'results.json'))
    worst = dict(word=0.0, bin=0.0, E=0.0)
    for c in cases:
        K = tuple(c['K'])
        on, off = res[c['id'] + '_1'], res[c['id'] + '_0']
        for side in (on, off):
            assert M.PATHS[side['info'][0]] == 'direct_planes', (c['id'], side['info'])
        # one forward and one inverse plane launch per convolution: (forward share, forward vector, inverse share, inverse vector)
        assert on['stats'][2:] == ([1, 0] if c['share'] else [0, 1]), (c['id'], on['stats'])
        assert off['stats'][2:] == [0, 1], (c['id'], off['stats'])
        assert on['stats'][:2] == off['stats'][:2] and sum(on['stats'][:2]) == 1, (c['id'], on['stats'], off['stats'])
        G = M.half_spectrum_table(M.g_table(M.make_box(K, False), K, c['kappa'], 1, 0))
        ref = M.Reference(M.make_input(c), G, 8)
        outs = {}
        for mode, side in (('1', on), ('0', off)):
            outs[mode] = np.load(tmp_path / ('%s_%s.npy' % (c['id'], mode)))
            fig = M.check_case(c, ref, outs[mode], side['E'])
            print('%-18s share %s  %s' % (c['id'], mode, ' '.join('%s=%.3g' % kv for kv in fig.items())))
        dword = float(np.abs(outs['1'] - outs['0']).max() / ref.B_word)
        dbin = float((np.abs(M._fftn(outs['1'] - outs['0'])) / ref.D).max())
        dE = abs(on['E'] - off['E']) / ref.B_E
        print('%-18s on - off: word/B_word=%.3g bin/D=%.3g E/B_E=%.3g' % (c['id'], dword, dbin, dE))
        assert dword <= 1.0 and dbin <= 1.0 and dE <= 1.0, (c['id'], dword, dbin, dE)
        worst = dict(word=max(worst['word'], dword), bin=max(worst['bin'], dbin), E=max(worst['E'], dE))
        if c['share']:
            assert not np.array_equal(outs['1'], outs['0']), c['id']          # (two forms did run)
    print('largest on - off:', {k: '%.3g' % v for k, v in worst.items()})


CODE = """
import os, sys, numpy as np
sys.path.insert(0, %r)
import torch
from tests.test_gpu_parity import water_system
from admp_amd import settings
from admp_amd.pme import ADMPPmeForce
out = {}

def host(x):
    return np.asarray(torch.as_tensor(x).cpu(), dtype=np.float64)

def call(f, mode, pos, box, pairs, par, U):
    os.environ['ADMP_DFT_PLANE_MFMA_INV'] = mode
    rest = (par['Q_local'], par['pol'], par['tholes'], par['mScales'], par['pScales'], par['dScales'])
    E, G = f.get_forces(pos, box, pairs, *rest, U_init=U)
    return dict(parts=np.asarray(f.energy_parts, dtype=np.float64), G=host(G), U=host(f.U_ind),
                n=np.asarray([int(f.n_cycle), int(bool(f.lconverg))]))

def sequence(key, make, frames, box, pairs, par):
    # handle A runs the inverse share, handle B the vector form; both start every call from A's dipoles
    fA, fB = make(), make()
    U = None
    for k, pos in enumerate(frames):
        a = call(fA, '1', pos, box, pairs, par, U)
        b = call(fB, '0', pos, box, pairs, par, U)
        U = fA.U_ind
        U = U.clone() if hasattr(U, 'clone') else np.array(U)
        for name in a:
            out['%%s|%%d|%%s|A' %% (key, k, name)] = a[name]
            out['%%s|%%d|%%s|B' %% (key, k, name)] = b[name]
    sA, sB = fA.scf_stats(), fB.scf_stats()
    keys = ('plain', 'speculative', 'speculative_failed', 'chained', 'chained_too_short', 'chained_too_long', 'jacobi_steps')
    out[key + '|scf|A'] = np.asarray([sA[q] for q in keys])
    out[key + '|scf|B'] = np.asarray([sB[q] for q in keys])
    pk = ('matrix_share', 'vector', 'inverse_share', 'inverse_vector')
    pA, pB = fA.plane_mfma_stats(), fB.plane_mfma_stats()
    out[key + '|planes|A'] = np.asarray([pA[q] for q in pk])
    out[key + '|planes|B'] = np.asarray([pB[q] for q in pk])

pos, box, at, ai, cov, par, pairs = water_system(125, 5, True)
box = np.asarray(box, dtype=np.float64)
rng = np.random.default_rng(5)
kick = rng.standard_normal(pos.shape)
frames = lambda n: [pos + 0.001 * (k // 3) * kick for k in range(n)]      # every geometry three times, as the rider test moves it

def make():
    settings.PRECISION = 'double'
    settings.REFERENCE_KPOINT_ORDER = False
    f = ADMPPmeForce(box, at, ai, cov, 4.0, 1e-4, 2, lpol=True)
    f.K1, f.K2, f.K3 = (35, 37, 34)
    f.refresh_calculators()
    return f

for key, thresh, n in (('plain', None, 6), ('tight', 1e-2, 6)):
    old = settings.POL_CONV
    if thresh is not None:
        settings.POL_CONV = thresh
    try:
        sequence(key, make, frames(n), box, pairs, par)
    finally:
        settings.POL_CONV = old
np.savez(sys.argv[1], **out)
print('PLANE-MFMA-INV-RUN-OK')
""" % ROOT


@pytest.mark.gpu
def test_whole_evaluation_inverse_share_on_and_off(tmp_path):
    path = str(tmp_path / 'planes.npz')
    env = dict(os.environ, ADMP_DFT='1')
    env.pop(SWITCH, None)
    env.pop('ADMP_DFT_PLANE_MFMA', None)
    r = subprocess.run([sys.executable, '-c', CODE, path], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and 'PLANE-MFMA-INV-RUN-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    res = dict(np.load(path))
    for key in ('plain', 'tight'):
        scfA, scfB = res[key + '|scf|A'], res[key + '|scf|B']
        pA, pB = res[key + '|planes|A'], res[key + '|planes|B']
        print(key, 'scf (plain, speculative, failed, chained, too short, too long, Jacobi steps):', scfA,
              'plane launches (forward share, all others, inverse share, inverse vector):', pA, pB)
        assert np.array_equal(scfA, scfB), (key, scfA, scfB)            # the same decisions, the same number of steps
        assert pA[2] > 0 and pA[3] == 0, (key, pA)                       # every inverse launch of A with the share
        assert pB[2] == 0 and pB[3] == pA[2], (key, pB)                  # ... and of B without, as many of them
        assert pA[0] > 0 and pA[0] == pB[0] and pA[1] == pB[1] == pA[2], (key, pA, pB)      # the forward share in both; [1] = the inverse launches
    worst = {}
    for name, b in res.items():
        if not name.endswith('|B') or name.count('|') != 3:
            continue
        key, k, what, _ = name.split('|')
        a = res[name[:-1] + 'A']
        if what == 'n':
            assert np.array_equal(a, b), (name, a, b)                   # cycle count and convergence flag
            continue
        assert np.isfinite(a).all() and np.isfinite(b).all(), name
        scale = np.abs(b).max()
        err = np.abs(a - b).max()
        worst[what] = max(worst.get(what, 0.0), err / scale)
        print('%-6s call %2s %-5s max|on - off| / max|off| = %.2e' % (key, k, what, err / scale))
        assert err <= TOL64 * scale, (name, err, scale)
    print('largest |share on - off| / max|off|:', {k: '%.2e' % v for k, v in sorted(worst.items())})


if __name__ == '__main__' and len(sys.argv) == 4 and sys.argv[1] == 'mesh':
    child_mesh(sys.argv[2], sys.argv[3])
