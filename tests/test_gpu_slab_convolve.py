"""The k-space leg of the SLAB ranks, bin by bin: MeshConv::slab_convolve with either x pass (admp_slab_mesh_convolve) against
numpy.fft in float64 -- the reference, the inputs and every bound of tests/test_gpu_mesh_convolve.py, unchanged (the passes run
in the same order z, y, x, x, y, z; what is new is where the words live while they run).

Why: the slab tests of tests/test_gpu_parity.py compare whole evaluations at the production kappa with tolerances of 1e-8 to
5e-4, the setting in which the single-rank bin-by-bin test found a table that was off by the whole signal in bins 1e-50 below
the leading ones.  A slab rank has more places of that kind: its G table starts at row Y0 (the Nyquist row K2/2 belongs to a
middle rank), k_transpose_pack works out owner, y0 and ny of every row in groups of 16 rows with spectrum rows of pitch
`khp`, k_fftx_conv / launch_kspace hold ny < K2 rows, and the ghost planes are added before and fetched after the transform.

Ranks: N threads of one child process on one GPU, one handle per rank on ThreadComm + CommBinding (admp_amd/parallel.py),
one child per switch setting: `default` (the fused x kernel on the transposed layout where K1 is a power of two, rocFFT 1-D x
lines + launch_kspace elsewhere) and `lines` (ADMP_FUSED_X=0: the power-of-two meshes through the rocFFT x lines, same data).

Input: the global mesh x of that module (unit-modulus noise, plane waves).  On the first 5 planes of every rank x is split in
the handle's type T as b = 0.25 x, a = x - b; b is handed to the previous rank as its 5 ghost planes, a stays in the own
planes.  The device adds them with one IEEE addition per word (k_mesh_add), so the reference input is fl_T(a + b), computed by
numpy in T: exact, no tolerance.  A ghost plane dropped, added twice or added to another plane changes the input by a quarter
of the signal.

Checks per case: the own planes of all ranks, assembled, and the sum of the ranks' energy words go through check_case of that
module (word bound B_word, energy bound B_E, f64 per bin under D with D / signal < 1e-3 at flat kappa, f32 per bin under the
model, waves in relative 2-norm under their bound, itself below 0.5); the ghost planes every rank received equal bit for bit
the first 5 own planes its successor returned; the info words equal slab_bounds() of parallel.py, the row pitch and K3/2+1;
the x pass is the expected one.  f32 per bin: C of the module's rule is measured in the same run, per kind of kappa, as the
largest err / model of the single-rank rocFFT 3-D path (one more child, ADMP_DFT=0 ADMP_FUSED_X=0, admp_mesh_convolve, the
noise inputs of every mesh of this file); every slab case, either x pass, is held to HAND_FACTOR C, and
HAND_FACTOR C model / signal < 0.1 is asserted at flat kappa.

Meshes (K1 x K2 x K3, ranks), the smallest at which each piece can go wrong (update_slab needs 6 planes and one row per rank):
  32x7x20  N=5   shortest length of the fused x kernel; widths 6 6 7 6 7; odd K2, 1 or 2 rows per rank; nh = 11 under pitch 16
  64x18x30 N=3   nh = 16 = pitch; K2 crosses the 16-row group of k_transpose_pack (second group: 2 rows); the Nyquist row
                 y = 9 on rank 1; Nyquist planes on x and z too
  36x33x22 N=2,6 rocFFT x lines; N=6: widths of exactly 6, rows 5 6 5 6 5 6; two full row groups plus one row.  N=2 orthorhombic
                 also runs tables 6, 8, 10 and the reference's literal k-point order on table 1 (gfactor_at with a row offset)
  45x8x12  N=7   widths 6 and 7; one row per rank but the last; the Nyquist row y = 4 on rank 3
every one in f32 and f64, orthorhombic and triclinic, noise at the production and the flat kappa, waves at the flat kappa; the
first case of every child on a device pointer.

Every case prints its ratios, the file its C, every test its worst ratios and its wall time (run with -s).  Measured on an
MI355X: C = 7.22 at the production kappa, 1.86 at flat kappa (rocFFT 3-D, 14 + 14 f32 cases on the four meshes; smaller
than the 33.2 / 2.6 of tests/test_gpu_mesh_convolve.py because the meshes are).  Largest ratios over all cases:
    x pass                        f32 bin err / (C model)   f64 bin err / D   word err / B_word   E err / B_E   wave rel2 (bound)
    fused x kernel, f32 | f64     0.92 of the 8 allowed     9.7e-4            2.5e-4 | 1.2e-4     1.8e-4 | 4.8e-4   2.2e-7 (0.016) | 2.2e-15 (5.5e-11)
    rocFFT x lines, f32 | f64     0.93 of the 8 allowed     0.065             2.5e-4 | 5.8e-4     6.7e-5 | 8.8e-4   1.7e-6 (0.016) | 3.2e-15 (5.5e-11)
At flat kappa D / signal <= 4.5e-10 (f64) and 8 C model / signal <= 2.2e-4 (f32) in every bin.  A test takes 6.1 to 7.0 s, of
which 1.6 s are the child's import of torch and about 2.5 s the transform plans of its two types; the calibration 9.8 s, once.
Nothing was found: no kernel changed.  Detection: with y0 of the wrong peer for the last row of a
group in k_transpose_pack, and with k_gtab's mirror index formed without the row offset, all seven tests fail.
"""
import ctypes
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_gpu_mesh_convolve import (Reference, g_table, half_spectrum_table, make_box, noise, wave, wave_bins,      # noqa: E402
                                          kappa_flat, KAPPA_PROD, check_case, g_ratio, HAND_FACTOR, PATHS, RT)

GHOST = 5                                  # Engine::kGhost
MESHES = [((32, 7, 20), 5), ((64, 18, 30), 3), ((36, 33, 22), 2), ((36, 33, 22), 6), ((45, 8, 12), 7)]
CHILDREN = {'default': {}, 'lines': {'ADMP_FUSED_X': '0'}}
CALIBRATION = {'ADMP_DFT': '0', 'ADMP_FUSED_X': '0'}
PARAMS = [(K, N, 'default') for K, N in MESHES] + [(K, N, 'lines') for K, N in MESHES if K[0] & (K[0] - 1) == 0]
TABLES_ON = ((36, 33, 22), 2)              # tables 6, 8, 10 and the literal k-point order, orthorhombic


def slab_bounds(K, size):
    from admp_amd.parallel import slab_bounds as sb
    return sb(K, size)


def cases_of(K, N, precs=(4, 8)):
    out = []
    for prec in precs:
        for tric in (False, True):
            tag = '%dx%dx%d_n%d_%s_f%d' % (K + (N, 'tric' if tric else 'ortho', 8 * prec))
            base = dict(K=list(K), N=N, tric=tric, prec=prec, ref_order=0, dev=0)
            tables = (1, 6, 8, 10) if ((K, N) == TABLES_ON and not tric) else (1,)
            for which in tables:
                for kind in ('prod', 'flat'):
                    kap = KAPPA_PROD if kind == 'prod' else kappa_flat(K, tric, which)
                    out.append(dict(base, id='%s_w%d_%s_noise' % (tag, which, kind), which=which, kappa=kap, kind=kind,
                                    input=dict(kind='noise', seed=1000 + sum(K))))
            kap = kappa_flat(K, tric, 1)
            for m in wave_bins(K, 7):
                out.append(dict(base, id='%s_w1_flat_wave_%d_%d_%d' % ((tag,) + m), which=1, kappa=kap, kind='flat',
                                input=dict(kind='wave', m=list(m))))
            if (K, N) == TABLES_ON and not tric:
                for kind in ('prod', 'flat'):
                    kap = KAPPA_PROD if kind == 'prod' else kappa_flat(K, tric, 1)
                    out.append(dict(base, id='%s_w1_%s_noise_reforder' % (tag, kind), which=1, kappa=kap, kind=kind, ref_order=1,
                                    input=dict(kind='noise', seed=1000 + sum(K))))
    out[0]['dev'] = 1                        # one case per child on a device pointer
    return out


def global_input(c):
    K = tuple(c['K'])
    if c['input']['kind'] == 'noise':
        return noise(K, c['input']['seed'], c['prec'])
    return wave(K, tuple(c['input']['m']), c['prec'])


def split_input(c):
    """(reference input fl_T(a + b) on the global mesh, [local mesh of rank s: own planes, then 5 ghost planes])"""
    K, N = tuple(c['K']), c['N']
    T = RT[c['prec']]
    x = global_input(c)
    assert x.dtype == T
    xs = slab_bounds(K[0], N)
    xref = x.copy()
    own = [x[lo:hi].copy() for lo, hi in xs]
    ghost = []
    for s in range(N):
        lo = xs[(s + 1) % N][0]              # the first planes of the next rank (rank N-1 overhangs into rank 0: periodic)
        b = (T(0.25) * x[lo:lo + GHOST]).astype(T)
        a = (x[lo:lo + GHOST] - b).astype(T)
        own[(s + 1) % N][:GHOST] = a
        ghost.append(b)
        xref[lo:lo + GHOST] = (a + b).astype(T)
    return xref, [np.ascontiguousarray(np.concatenate([own[s], ghost[s]], axis=0)) for s in range(N)]


def pitch_of(K, prec):
    per_line = 128 // (2 * prec)
    nh = K[2] // 2 + 1
    return (nh + per_line - 1) // per_line * per_line


# ---- children ------------------------------------------------------------------------------------------------------------------
def child_slab(cases_path, outdir):
    """every case on its N rank threads; a rank that fails releases the others (barrier.abort), the joins have a timeout"""
    import torch                             # before the library, as everywhere else: one HIP runtime per process, torch's
    torch.cuda.init()
    from admp_amd import _lib
    from admp_amd.parallel import CommBinding, ThreadComm
    L = _lib.load()
    cases = json.load(open(cases_path))
    N = cases[0]['N']
    assert all(c['N'] == N for c in cases)
    device = torch.device('cuda', 0)
    world = ThreadComm.World(N)
    inputs = [split_input(c)[1] for c in cases]
    results = [dict() for _ in range(N)]
    errors = []

    def work(rank):
        try:
            torch.cuda.set_device(0)
            binding = CommBinding(ThreadComm(world, rank), device)
            handles = {}
            for c, loc in zip(cases, inputs):
                K, prec = tuple(c['K']), c['prec']
                if prec not in handles:
                    h = ctypes.c_void_p()
                    rc = L.admp_create(ctypes.byref(h), 0, prec)
                    assert rc == 0, 'admp_create %d' % rc
                    # ThreadComm orders its exchanges by synchronising torch's current stream: the handle works on it
                    _lib.check(h, L.admp_use_default_stream(h), 'admp_use_default_stream')
                    _lib.check(h, L.admp_slab_configure(h, rank, N), 'admp_slab_configure')
                    _lib.check(h, L.admp_set_comm(h, ctypes.byref(binding.struct)), 'admp_set_comm')
                    handles[prec] = h
                h = handles[prec]
                _lib.check(h, L.admp_set_ewald(h, float(c['kappa']), K[0], K[1], K[2], 2, 0), 'admp_set_ewald')
                _lib.check(h, L.admp_set_option(h, _lib.OPT_REFERENCE_KPOINTS, int(c['ref_order'])), 'admp_set_option')
                box = _lib.darr(make_box(K, c['tric']))
                E = ctypes.c_double(0.0)
                info = (ctypes.c_int * _lib.MESH_INFO_WORDS)()
                binding.error = None
                if c['dev']:
                    t = torch.from_numpy(loc[rank]).to(device)
                    torch.cuda.synchronize()
                    rc = L.admp_slab_mesh_convolve(h, box, c['which'], ctypes.c_void_p(t.data_ptr()), 1, ctypes.byref(E), info)
                    out = t.cpu().numpy() if rc == 0 else None
                else:
                    out = loc[rank].copy()
                    rc = L.admp_slab_mesh_convolve(h, box, c['which'], out.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(E), info)
                if rc != 0 and binding.error is not None:
                    raise binding.error
                _lib.check(h, rc, 'admp_slab_mesh_convolve')
                np.save(os.path.join(outdir, '%s.r%d.npy' % (c['id'], rank)), out)
                results[rank][c['id']] = dict(E=E.value, info=list(info))
            for h in handles.values():
                L.admp_destroy(h)
        except BaseException as e:      # noqa: BLE001
            errors.append((rank, repr(e)))
            try:
                world.barrier.abort()
            except Exception:      # noqa: BLE001
                pass

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(N)]
    for t in threads:
        t.start()
    deadline = time.time() + 240
    for t in threads:
        t.join(timeout=max(1.0, deadline - time.time()))
    alive = [r for r, t in enumerate(threads) if t.is_alive()]
    if errors or alive:
        print('SLAB-CHILD-FAILED errors=%r alive=%r' % (errors, alive))
        sys.stdout.flush()
        os._exit(3)
    json.dump(results, open(os.path.join(outdir, 'results.json'), 'w'))
    print('SLAB-CHILD-OK %d cases on %d ranks' % (len(cases), N))


def child_single(cases_path, outdir):
    """the calibration: the same reference inputs through admp_mesh_convolve on one rank (rocFFT 3-D by the child's switches)"""
    import torch
    torch.cuda.init()
    from admp_amd import _lib
    L = _lib.load()
    cases = json.load(open(cases_path))
    handles, results = {}, {}
    for c in cases:
        K, prec = tuple(c['K']), c['prec']
        if (K, prec) not in handles:
            h = ctypes.c_void_p()
            rc = L.admp_create(ctypes.byref(h), 0, prec)
            assert rc == 0, 'admp_create %d' % rc
            handles[(K, prec)] = h
        h = handles[(K, prec)]
        _lib.check(h, L.admp_set_ewald(h, float(c['kappa']), K[0], K[1], K[2], 2, 0), 'admp_set_ewald')
        _lib.check(h, L.admp_set_option(h, _lib.OPT_REFERENCE_KPOINTS, int(c['ref_order'])), 'admp_set_option')
        out = split_input(c)[0].copy()
        E = ctypes.c_double(0.0)
        info = (ctypes.c_int * _lib.MESH_INFO_WORDS)()
        _lib.check(h, L.admp_mesh_convolve(h, _lib.darr(make_box(K, c['tric'])), c['which'], out.ctypes.data_as(ctypes.c_void_p), 0,
                                           ctypes.byref(E), info), 'admp_mesh_convolve')
        np.save(os.path.join(outdir, c['id'] + '.npy'), out)
        results[c['id']] = dict(E=E.value, info=list(info))
    json.dump(results, open(os.path.join(outdir, 'results.json'), 'w'))
    print('SLAB-CHILD-OK %d cases on 1 rank' % len(cases))


def run_child(mode, cases, d, switches, timeout):
    clean = {k: v for k, v in os.environ.items() if not k.startswith('ADMP_') or k == 'ADMP_HIP_LIB'}
    d.mkdir()
    (d / 'cases.json').write_text(json.dumps(cases))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, str(d / 'cases.json'), str(d)], capture_output=True,
                       text=True, env=dict(clean, **switches), timeout=timeout, cwd=ROOT)
    assert r.returncode == 0 and 'SLAB-CHILD-OK' in r.stdout, (mode, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.load(open(d / 'results.json'))


# ---- reference, shared by the tests of a run -----------------------------------------------------------------------------------
_REFS = {}


def reference_of(c):
    """one Reference per (mesh, ranks, box, kappa, table, order, type, input); never modified"""
    key = (tuple(c['K']), c['N'], c['tric'], c['kappa'], c['which'], c['ref_order'], c['prec'], json.dumps(c['input'], sort_keys=True))
    if key not in _REFS:
        K = tuple(c['K'])
        G = half_spectrum_table(g_table(make_box(K, c['tric']), K, c['kappa'], c['which'], c['ref_order']))
        if c['kind'] == 'flat':
            assert g_ratio(G) < 1e5, (c['id'], g_ratio(G))
        _REFS[key] = Reference(split_input(c)[0], G, c['prec'], per_bin=c['input']['kind'] == 'noise')
    return _REFS[key]


@pytest.fixture(scope='module')
def calibration(tmp_path_factory):
    """C of the f32 per-bin model, per kind of kappa: the largest err / model of the single-rank rocFFT 3-D path over the noise
    inputs of every mesh of this file"""
    t0 = time.time()
    cases = [c for K, N in MESHES for c in cases_of(K, N, precs=(4,)) if c['input']['kind'] == 'noise']
    for c in cases:
        c['dev'] = 0
    d = tmp_path_factory.mktemp('slab_convolve') / 'calibration'
    res = run_child('single', cases, d, CALIBRATION, 300)
    ratios = {'prod': [], 'flat': []}
    for c in cases:
        assert PATHS[res[c['id']]['info'][0]] == 'rocfft', (c['id'], res[c['id']]['info'])
        fig = check_case(c, reference_of(c), np.load(d / (c['id'] + '.npy')), res[c['id']]['E'])
        ratios[c['kind']].append(fig['bin/model'])
    C = {k: max(v) for k, v in ratios.items()}
    print('\nf32 model constant C: %.4g at the production kappa, %.4g at flat kappa (rocFFT 3-D path, %d + %d cases, %.1f s)'
          % (C['prod'], C['flat'], len(ratios['prod']), len(ratios['flat']), time.time() - t0))
    return C


@pytest.mark.gpu
@pytest.mark.parametrize('K,N,child', PARAMS, ids=['%dx%dx%d-n%d-%s' % (K + (N, ch)) for K, N, ch in PARAMS])
def test_slab_convolve_bin_by_bin(tmp_path, calibration, K, N, child):
    t0 = time.time()
    cases = cases_of(K, N)
    d = tmp_path / 'run'
    res = run_child('slab', cases, d, CHILDREN[child], 300)
    t_gpu = time.time() - t0
    xs, ys = slab_bounds(K[0], N), slab_bounds(K[1], N)
    assert min(hi - lo for lo, hi in xs) >= 6 and min(hi - lo for lo, hi in ys) >= 1
    want_path = 'fused_x' if (child == 'default' and K[0] & (K[0] - 1) == 0 and K[0] >= 32) else 'rocfft'
    worst = {}
    for c in cases:
        loc = [np.load(d / ('%s.r%d.npy' % (c['id'], s))) for s in range(N)]
        E = 0.0
        for s in range(N):
            info = res[s][c['id']]['info']
            assert PATHS[info[0]] == want_path, (c['id'], s, info)
            assert tuple(info[2:6]) == xs[s] + ys[s], (c['id'], s, info, xs[s], ys[s])
            assert info[6] == pitch_of(K, c['prec']) and info[7] == K[2] // 2 + 1, (c['id'], s, info)
            assert info[1] == 0 and not any(info[8:]), (c['id'], s, info)
            nx = xs[s][1] - xs[s][0]
            assert loc[s].shape == (nx + GHOST, K[1], K[2]) and loc[s].dtype == RT[c['prec']], (c['id'], s, loc[s].shape)
            E += res[s][c['id']]['E']
        for s in range(N):                   # what the closing shift delivered: the successor's first planes, bit for bit
            nx = xs[s][1] - xs[s][0]
            assert np.array_equal(loc[s][nx:].view(np.uint8), loc[(s + 1) % N][:GHOST].view(np.uint8)), (c['id'], 'ghost planes of rank', s)
        out = np.concatenate([loc[s][:xs[s][1] - xs[s][0]] for s in range(N)], axis=0)
        assert out.shape == K
        fig = check_case(c, reference_of(c), out, E)
        print('%-8s %-52s %s' % (child, c['id'], ' '.join('%s=%.3g' % (k, v) for k, v in fig.items() if k != 'worst_bin')))
        if 'bin/model' in fig:
            C = calibration[c['kind']]
            fig['bin/(C model)'] = fig['bin/model'] / C
            assert fig['bin/model'] <= HAND_FACTOR * C, (child, c['id'], fig, C)
            if 'model/signal' in fig:
                fig['8 C model/signal'] = HAND_FACTOR * C * fig['model/signal']
                assert fig['8 C model/signal'] < 0.1, (child, c['id'], fig, C)
        for k, v in fig.items():
            if k != 'worst_bin':
                kk = '%s f%d %s' % (want_path, 8 * c['prec'], k)
                worst[kk] = max(worst.get(kk, 0.0), v)
    for k in sorted(worst):
        print('worst  %-44s %.3g' % (k, worst[k]))
    print('wall time %dx%dx%d N=%d %s: %.1f s (%d cases, %.1f s in the child)' % (K + (N, child, time.time() - t0, len(cases), t_gpu)))


@pytest.mark.gpu
def test_slab_entries_refuse_a_single_rank_handle():
    import torch                             # before the library, as everywhere else
    torch.cuda.init()
    from admp_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.admp_create(ctypes.byref(h), 0, 8) == 0
    x = np.zeros((8, 8, 8))
    box = _lib.darr(make_box((8, 8, 8), False))
    E = ctypes.c_double(0.0)
    info = (ctypes.c_int * _lib.MESH_INFO_WORDS)()
    p = x.ctypes.data_as(ctypes.c_void_p)
    assert L.admp_slab_mesh_convolve(h, box, 1, p, 0, ctypes.byref(E), info) != 0          # no admp_set_ewald yet
    _lib.check(h, L.admp_set_ewald(h, 0.5, 8, 8, 8, 2, 0), 'admp_set_ewald')
    assert L.admp_slab_mesh_convolve(h, box, 1, p, 0, ctypes.byref(E), info) != 0
    assert b'slab-decomposed handle only' in L.admp_last_error(h)
    _lib.check(h, L.admp_slab_configure(h, 0, 2), 'admp_slab_configure')
    assert L.admp_slab_mesh_convolve(h, box, 1, p, 0, ctypes.byref(E), info) != 0          # decomposed, but no communicator
    assert b'communicator' in L.admp_last_error(h)
    L.admp_destroy(h)


if __name__ == '__main__' and len(sys.argv) == 4 and sys.argv[1] in ('slab', 'single'):
    (child_slab if sys.argv[1] == 'slab' else child_single)(sys.argv[2], sys.argv[3])
