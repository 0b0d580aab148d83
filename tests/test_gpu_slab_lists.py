"""The decomposition of the slab ranks, word by word: owner and bits of every atom, the home / rows / act lists, the per-peer
import and export lists and the migrant lists of SlabDecomp::decompose (k_slab_owner, k_slab_marks, k_slab_bins, k_compact_*,
k_slab_concat; read back by admp_slab_lists) against the plain float64 restatement of the rule in tests/slab_ref.py.

Why: this is integer work whose outputs nothing looked at -- only admp_slab_home exposes the home list and the import count.
Since round 4 a steady-state rank prepares the site rows of its home atoms and its imports only, so an import that is missing
reads a stale row: an error of the size of one step's motion, below every end-to-end tolerance.

Every case of tests/slab_ref.py (its features are proved in tests/test_slab_ref_cpu.py) runs as SlabPme evaluations on
ThreadComm ranks, N threads of one child process on one GPU, in both types, in two children: the one-pass bins (default) and
the per-column compaction (ADMP_SLAB_BINS=0).  Compared, exactly, on every rank: owner; bits (kSlabHome, kSlabPolar and the
export mask on home words, 1 << owner on the words of the atoms the rank reads, 0 elsewhere); home, act, imports and exports
per peer, migrants per peer, element by element with their counts; rows as a permutation of home; n_home / n_import of
admp_slab_home.  Across the ranks, on the device's own outputs: the imports of r from t are the exports of t to r.  The two
children return the same words (a digest of every array of a group is compared when both have run).

Cases: water boxes of 192, 1026 and 4098 atoms (the 64-lane chunk and the 1024-atom span of the compaction, crossed by two
atoms) with wrapped positions, 48 planes along x, N = 2, 3, 5, 8 (at N = 8 a slab is 6 planes); ZBisect / ThreeFold / Zonly
frames with an axis atom two lattice planes away; pol = 0 on a third of the sites; a handle that is not polarizable; an
orthorhombic 16 A cell with 32 planes where u = 2 x is exact in both types and atoms sit on planes and slab faces; two
evaluations with all atoms moved by 1.5 planes in between (polarizable handle, outputs='home': migrants, and the steady-state
path that prepares home + import rows only); a table built by admp_set_pairs_from_positions on the slab rank (filtered rows,
`built` flags) against the full-list reference.

Not reached: the second 1024-block chunk of k_compact_scan needs more than a million atoms.  The halo pack / unpack kernels
stay under the end-to-end tests.  The only figure of this file is zero differences; every test prints its wall time (-s).
Measured on an MI355X: 0 differences in 764 460 words per child setting, 0 atoms excluded; a test takes 5.7 to 9.3 s, of which
about 5.5 s are the child's start, its transform plans and a handle's first evaluation.  Detection:
k_slab_marks without its inverse-frame loop fails the general-frame cases alone, k_slab_bins ranking by the higher lanes of a
bin fails every `bins` test and no `columns` test; the existing slab tests pass under both.

A new topology forgets the previous owners (test_a_new_topology_forgets_the_previous_owners): 192 atoms on 2 ranks, double
precision, an evaluation at pos, one 5.5 planes further (tracked, 8 migrants each way), admp_set_topology again with the same
arrays, an evaluation at pos -- not tracked, no migrants, every list that of pos.  5.7 s on the MI355X.  Against the library of
the commit before SlabDecomp::forget the third evaluation came back tracked with 8 + 8 migrants (observed).
"""
import ctypes
import hashlib
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
from tests import slab_ref as R      # noqa: E402

CHILDREN = {'bins': {}, 'columns': {'ADMP_SLAB_BINS': '0'}}
PRECS = ('double', 'single')
ARRAYS = ('owner', 'bits', 'home', 'rows', 'act', 'imp', 'exp', 'mig_in', 'mig_out', 'counts')


def read_lists(f, na, N):
    """admp_slab_lists of a calculator's handle -> dict of trimmed arrays"""
    i32 = lambda n: np.full(n, -7, dtype=np.int32)      # noqa: E731
    a = dict(owner=i32(na), bits=i32(na), home=i32(na), rows=i32(na), act=i32(na), imp=i32(na), exp=i32(na * N), mig_in=i32(na),
             mig_out=i32(na), counts=np.full(8 + 4 * N, -7, dtype=np.int64))
    p = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_int))      # noqa: E731
    from admp_amd import _lib
    _lib.check(f._h, f._L.admp_slab_lists(f._h, na, N, p(a['owner']), p(a['bits']), p(a['home']), p(a['rows']), p(a['act']),
                                          p(a['imp']), p(a['exp']), p(a['mig_in']), p(a['mig_out']),
                                          a['counts'].ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), 'admp_slab_lists')
    c = a['counts']
    for k, n in (('home', c[0]), ('rows', c[0]), ('act', c[1]), ('imp', c[2]), ('exp', c[3]), ('mig_in', c[5]), ('mig_out', c[6])):
        assert (a[k][int(n):] == -7).all(), ('admp_slab_lists wrote past the count of', k)
        a[k] = a[k][:int(n)].copy()
    return a


def child_main(spec_path, outdir):
    """every (case, type) on its N rank threads; a rank that fails releases the others, the joins have a timeout"""
    import torch                             # before the library, as everywhere else
    torch.cuda.init()
    from admp_amd import settings
    from admp_amd.parallel import SlabPme, ThreadComm
    settings.REFERENCE_KPOINT_ORDER = False      # (unequal mesh dimensions: the consistent k-point order, no warning)
    settings.MAX_N_POL = 2                       # the lists are made before the SCF starts: two cycles (one dipole exchange) will do
    spec = json.load(open(spec_path))
    for name in spec['cases']:
        c = R.case(name)
        N, na, par = c['N'], c['na'], c['par']
        for prec in spec['precs']:
            settings.PRECISION = prec
            world = ThreadComm.World(N)
            errors = []

            def work(rank):
                try:
                    torch.cuda.set_device(0)
                    f = SlabPme(ThreadComm(world, rank), c['box'], c['at'], c['ai'], c['cov'], c['rc'], 1e-4, 2, lpol=c['lpol'],
                                outputs='home')
                    f.K1 = c['K0']
                    f.refresh_calculators()
                    for e, pos in enumerate([c['pos']] + ([c['pos2']] if c['shift_planes'] is not None else [])):
                        pairs = c['pairs']
                        if c['from_positions']:
                            f.update_neighbors(pos, c['box'], c['rc'])
                            pairs = None
                        if c['lpol']:
                            f.get_forces(pos, c['box'], pairs, par['Q_local'], par['pol'], par['tholes'], par['mScales'],
                                         par['pScales'], par['dScales'])
                        else:
                            f.get_forces(pos, c['box'], pairs, par['Q_local'], par['mScales'])
                        a = read_lists(f, na, N)
                        a['slab_home'] = np.array([f.n_home, f.n_import], dtype=np.int64)
                        a['home_atoms'] = f.home_atoms.cpu().numpy().astype(np.int64)
                        a['mesh'] = np.array([f.K1, f.K2, f.K3], dtype=np.int64)
                        np.savez(os.path.join(outdir, '%s.%s.r%d.e%d.npz' % (name, prec, rank, e)), **a)
                except BaseException as ex:      # noqa: BLE001
                    errors.append((name, prec, rank, repr(ex)))
                    try:
                        world.barrier.abort()
                    except Exception:      # noqa: BLE001
                        pass

            threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(N)]
            for t in threads:
                t.start()
            deadline = time.time() + 120
            for t in threads:
                t.join(timeout=max(1.0, deadline - time.time()))
            alive = [r for r, t in enumerate(threads) if t.is_alive()]
            if errors or alive:
                print('LISTS-CHILD-FAILED errors=%r alive=%r' % (errors, alive))
                sys.stdout.flush()
                os._exit(3)
    print('LISTS-CHILD-OK %d cases' % len(spec['cases']))


def segments(flat, counts):
    out, o = [], 0
    for n in counts:
        out.append([int(v) for v in flat[o:o + int(n)]])
        o += int(n)
    assert o == len(flat)
    return out


def check_rank(tag, a, want, owner, N, r, lpol, tracked, mig):
    """one rank's arrays against the reference, exactly; returns (imports per peer, exports per peer) as the device has them"""
    na = len(owner)
    assert np.array_equal(a['owner'].astype(np.int64), owner), (tag, 'owner', np.nonzero(a['owner'] != owner)[0][:10])
    bad = np.nonzero(a['bits'].astype(np.int64) != want['bits'])[0]
    assert bad.size == 0, (tag, 'bits', [(int(i), hex(int(a['bits'][i])), hex(int(want['bits'][i]))) for i in bad[:10]])
    assert [int(v) for v in a['home']] == want['home'], (tag, 'home')
    assert sorted(int(v) for v in a['rows']) == want['home'] and len(set(a['rows'].tolist())) == len(a['rows']), (tag, 'rows')
    assert [int(v) for v in a['act']] == want['act'], (tag, 'act')
    cn = a['counts']
    imp_cnt, exp_cnt = cn[8:8 + N], cn[8 + N:8 + 2 * N]
    min_cnt, mout_cnt = cn[8 + 2 * N:8 + 3 * N], cn[8 + 3 * N:8 + 4 * N]
    imp, exp = segments(a['imp'], imp_cnt), segments(a['exp'], exp_cnt)
    assert imp == want['imports'], (tag, 'imports', [(t, len(imp[t]), len(want['imports'][t])) for t in range(N)])
    assert exp == want['exports'], (tag, 'exports', [(t, len(exp[t]), len(want['exports'][t])) for t in range(N)])
    assert (int(cn[0]), int(cn[1]), int(cn[2]), int(cn[3])) == (len(want['home']), len(want['act']), sum(map(len, imp)),
                                                                  sum(map(len, exp))), (tag, 'counts', cn[:8])
    assert int(cn[7]) == 0 and int(cn[4]) == (1 if tracked else 0), (tag, 'tracked', cn[:8])
    mig_in, mig_out = segments(a['mig_in'], min_cnt), segments(a['mig_out'], mout_cnt)
    if tracked:
        assert (mig_in, mig_out) == (mig[0], mig[1]), (tag, 'migrants')
        assert (int(cn[5]), int(cn[6])) == (sum(map(len, mig[0])), sum(map(len, mig[1]))), (tag, cn[:8])
    else:
        assert int(cn[5]) == 0 and int(cn[6]) == 0 and not any(mig_in) and not any(mig_out), (tag, 'migrants of an untracked call')
    assert tuple(a['slab_home']) == (len(want['home']), sum(map(len, want['imports']))), (tag, 'admp_slab_home', a['slab_home'])
    assert [int(v) for v in a['home_atoms']] == want['home'], (tag, 'admp_slab_home list')
    assert len(a['bits']) == na
    return imp, exp


_DIGESTS = {}
# (group, types): the two larger water boxes run their types in tests of their own -- four rank counts of up to 8 threads
# each take 3 to 4 s per type next to the 3.5 s a child needs to start and to build its transform plans
RUNS = [(g, PRECS) for g in R.GROUPS if g not in ('w342', 'w1366')] + [(g, (p,)) for g in ('w342', 'w1366') for p in PRECS]


@pytest.mark.gpu
@pytest.mark.parametrize('child', list(CHILDREN))
@pytest.mark.parametrize('group,precs', RUNS, ids=['%s-%s' % (g, '+'.join(p)) for g, p in RUNS])
def test_slab_lists_word_by_word(tmp_path, group, precs, child):
    t0 = time.time()
    names = R.GROUPS[group]
    clean = {k: v for k, v in os.environ.items() if not k.startswith('ADMP_') or k == 'ADMP_HIP_LIB'}
    (tmp_path / 'spec.json').write_text(json.dumps(dict(cases=names, precs=list(precs))))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'child', str(tmp_path / 'spec.json'), str(tmp_path)],
                       capture_output=True, text=True, env=dict(clean, **CHILDREN[child]), timeout=600, cwd=ROOT)
    assert r.returncode == 0 and 'LISTS-CHILD-OK' in r.stdout, (group, child, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    t_gpu = time.time() - t0
    digest = hashlib.sha256()
    words = 0
    for name in names:
        c, ref = R.case(name), R.reference(name)
        N = c['N']
        evals = [(ref['owner'], ref['ranks'])] + ([(ref['owner2'], ref['ranks2'])] if 'owner2' in ref else [])
        for prec in precs:
            for e, (owner, ranks) in enumerate(evals):
                tracked = e > 0 and c['lpol']
                got = []
                for rk in range(N):
                    a = dict(np.load(tmp_path / ('%s.%s.r%d.e%d.npz' % (name, prec, rk, e))))
                    assert tuple(a['mesh'][:1]) == (c['K0'],) and a['mesh'][1] >= N, (name, a['mesh'])
                    tag = '%s %s rank %d evaluation %d (%s)' % (name, prec, rk, e, child)
                    got.append(check_rank(tag, a, ranks[rk], owner, N, rk, c['lpol'], tracked, ref['mig'][rk] if tracked else None))
                    for k in ARRAYS:
                        digest.update(np.ascontiguousarray(a[k]).tobytes())
                        words += a[k].size
                for rk in range(N):          # on the device's own outputs: what r imports from t is what t exports to r
                    for t in range(N):
                        assert got[rk][0][t] == got[t][1][rk], (name, prec, e, rk, t)
    key = (group, tuple(precs))
    _DIGESTS.setdefault(key, {})[child] = digest.hexdigest()
    assert len(set(_DIGESTS[key].values())) == 1, ('the two compactions differ', key, _DIGESTS[key])
    print('wall time %s %s %s: %.1f s (%.1f s in the child), %d cases, %d words compared, 0 differences'
          % (group, '+'.join(precs), child, time.time() - t0, t_gpu, len(names), words))


@pytest.mark.gpu
def test_slab_lists_refuses_handles_without_a_decomposition():
    import torch                             # before the library, as everywhere else
    torch.cuda.init()
    from admp_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.admp_create(ctypes.byref(h), 0, 8) == 0
    na, N = 6, 2
    i32 = [np.zeros(na * N, dtype=np.int32) for _ in range(9)]
    cnt = np.zeros(8 + 4 * N, dtype=np.int64)
    args = [x.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) for x in i32] + [cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))]
    assert L.admp_slab_lists(h, na, N, *args) != 0
    assert b'slab-decomposed handle only' in L.admp_last_error(h)
    _lib.check(h, L.admp_slab_configure(h, 0, N), 'admp_slab_configure')
    assert L.admp_slab_lists(h, na, N, *args) != 0
    assert b'no decomposed evaluation' in L.admp_last_error(h)
    L.admp_destroy(h)


def retopology_case():
    """the smallest polarizable water box of slab_ref (192 atoms, 2 ranks) with a second configuration 5.5 planes along x: 8 atoms
    change hands in each direction"""
    if 'retopology_n2' not in R._BUILT:
        R._BUILT['retopology_n2'] = R.water_case('retopology_n2', 64, 59, 2, shift_planes=5.5)
    return R._BUILT['retopology_n2']


def child_retopology(outdir):
    """pos, pos2, then admp_set_topology again with the same arrays, then pos: the lists after each evaluation"""
    import torch                             # before the library, as everywhere else
    torch.cuda.init()
    from admp_amd import _lib, settings
    from admp_amd._device import covalent_to_csr
    from admp_amd.parallel import SlabPme, ThreadComm
    settings.REFERENCE_KPOINT_ORDER = False
    settings.MAX_N_POL = 2
    settings.PRECISION = 'double'
    c = retopology_case()
    N, na, par = c['N'], c['na'], c['par']
    world = ThreadComm.World(N)
    errors = []

    def work(rank):
        try:
            torch.cuda.set_device(0)
            f = SlabPme(ThreadComm(world, rank), c['box'], c['at'], c['ai'], c['cov'], c['rc'], 1e-4, 2, lpol=True, outputs='home')
            f.K1 = c['K0']
            f.refresh_calculators()
            for e, pos in enumerate((c['pos'], c['pos2'], c['pos'])):
                if e == 2:
                    at = np.ascontiguousarray(c['at'], dtype=np.int32)
                    ai = np.ascontiguousarray(c['ai'], dtype=np.int32)
                    csr = covalent_to_csr(c['cov'], na)
                    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
                    _lib.check(f._h, f._L.admp_set_topology(f._h, na, p(at), p(ai), p(csr[0]), p(csr[1]), p(csr[2])),
                               'admp_set_topology')
                    f._pairs_key = None              # the handle dropped its table with the topology
                f.get_forces(pos, c['box'], c['pairs'], par['Q_local'], par['pol'], par['tholes'], par['mScales'], par['pScales'],
                             par['dScales'])
                a = read_lists(f, na, N)
                a['slab_home'] = np.array([f.n_home, f.n_import], dtype=np.int64)
                a['home_atoms'] = f.home_atoms.cpu().numpy().astype(np.int64)
                np.savez(os.path.join(outdir, 'retopology.r%d.e%d.npz' % (rank, e)), **a)
        except BaseException as ex:      # noqa: BLE001
            errors.append((rank, repr(ex)))
            try:
                world.barrier.abort()
            except Exception:      # noqa: BLE001
                pass

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(N)]
    for t in threads:
        t.start()
    deadline = time.time() + 120
    for t in threads:
        t.join(timeout=max(1.0, deadline - time.time()))
    alive = [r for r, t in enumerate(threads) if t.is_alive()]
    if errors or alive:
        print('LISTS-CHILD-FAILED errors=%r alive=%r' % (errors, alive))
        sys.stdout.flush()
        os._exit(3)
    print('LISTS-CHILD-OK retopology')


@pytest.mark.gpu
def test_a_new_topology_forgets_the_previous_owners(tmp_path):
    """admp_set_topology between two evaluations of the same atom count: the next decomposition is a first one -- not tracked,
    no migrants -- and its lists are those of its positions.  (Before SlabDecomp::forget the owners of the system that is gone
    stayed on record: counts[4] came back 1 and the dipoles of the "migrants" were shipped between the ranks.)"""
    t0 = time.time()
    clean = {k: v for k, v in os.environ.items() if not k.startswith('ADMP_') or k == 'ADMP_HIP_LIB'}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'retopology', str(tmp_path)], capture_output=True, text=True,
                       env=clean, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and 'LISTS-CHILD-OK' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    c = retopology_case()
    N, par = c['N'], c['par']
    assert (c['na'], N, c['lpol']) == (192, 2, True)
    table, axes = R.pair_table(c['pairs'], c['na']), R.axis_atoms(c['at'], c['ai'])
    own, own2 = R.owners(c['pos'], c['box'], c['K0'], N), R.owners(c['pos2'], c['box'], c['K0'], N)
    ranks, ranks2 = (R.decomposition(o, table, axes, par['pol'], True, N) for o in (own, own2))
    mig = [R.migrants(own, own2, rk, N) for rk in range(N)]
    assert all(sum(map(len, m[0])) == 8 and sum(map(len, m[1])) == 8 for m in mig)      # atoms change hands in both directions
    for e, (owner, want, tracked) in enumerate(((own, ranks, False), (own2, ranks2, True), (own, ranks, False))):
        for rk in range(N):
            a = dict(np.load(tmp_path / ('retopology.r%d.e%d.npz' % (rk, e))))
            print('evaluation %d rank %d counts[:8] = %s' % (e, rk, a['counts'][:8].tolist()))
            assert int(a['counts'][4]) == (1 if tracked else 0), ('evaluation', e, 'rank', rk, 'tracked', a['counts'][:8])
            check_rank('retopology rank %d evaluation %d' % (rk, e), a, want[rk], owner, N, rk, True, tracked,
                       mig[rk] if tracked else None)
    print('wall time retopology: %.1f s' % (time.time() - t0))


if __name__ == '__main__' and len(sys.argv) == 4 and sys.argv[1] == 'child':
    child_main(sys.argv[2], sys.argv[3])
if __name__ == '__main__' and len(sys.argv) == 3 and sys.argv[1] == 'retopology':
    child_retopology(sys.argv[2])
