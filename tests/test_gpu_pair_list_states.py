"""The states a handle's neighbour table goes through -- set from a list, built from positions, pruned, recompiled for new
site classes, lent and borrowed, dropped by a new topology, and the pending count of admp_neighbor_count -- walked one
transition at a time.  A cutoff of RC is set on every handle, so a skin list, any pruned list above RC and the exact list
must give the same numbers: after every transition the energies, gradient, dipoles and cycle count are compared at 1e-10
with a fresh handle that was given the exact list, and admp_num_pairs with the count of the list in force.

The hydrogens carry a charge only, so that the first evaluation of a handle compiles site classes into its table (and, on a
pruned table, goes back to the table as built to do so)."""
import ctypes

import numpy as np
import pytest
import torch

from admp_amd import _lib, settings
from admp_amd import systems as S
from admp_amd._device import covalent_to_csr
from tests.test_gpu_pme_cutoff import RC, SKIN, lists, pme, run, same, water

pytestmark = pytest.mark.gpu

N_A, N_B = 216, 125                # the system, and one of another atom count for admp_set_topology
R1, R2 = RC + 0.4, RC + 0.7        # pruning radii between the cutoff and the skin list's
NO_PAIRS = 'topology, ewald parameters and pairs must be set first'


def system(n_mol, seed):
    pos, box, at, ai, cov, par = water(n_mol, seed)
    par = dict(par)
    Q = np.array(par['Q_local'], dtype=np.float64)
    Q[np.arange(len(Q)) % 3 != 0, 1:] = 0.0       # charge-only hydrogens
    par['Q_local'] = Q
    skin, exact = lists(pos, box)
    return dict(pos=pos, box=box, at=at, ai=ai, cov=cov, par=par, skin=skin, exact=exact, na=3 * n_mol)


def below(s, r):
    """Number of pairs below r, none of them within 1e-5 A of it (the device and the host then count the same pairs)."""
    L = np.diag(np.asarray(s['box'], dtype=np.float64))
    wide = S.build_pairs(s['pos'], s['box'], r + 0.1)
    d = s['pos'][wide[:, 0]] - s['pos'][wide[:, 1]]
    d -= L * np.floor(d / L + 0.5)
    dist = np.sqrt((d * d).sum(1))
    assert np.abs(dist - r).min() > 1e-5
    return int((dist < r).sum())


@pytest.fixture(scope='module')
def world():
    old = settings.PRECISION
    settings.PRECISION = 'double'
    A, B = system(N_A, 36), system(N_B, 41)
    box = A['box']                                # every handle takes its Ewald parameters from this box
    w = dict(A=A, B=B, box=box)
    for s in (A, B):
        s['want'] = run(pme(box, s['at'], s['ai'], s['cov']), s['pos'], s['box'], s['exact'], s['par'], True)
        s['n_skin'] = below(s, RC + SKIN)
        assert s['n_skin'] == len(s['skin'])
    A['wider'] = S.build_pairs(A['pos'], A['box'], RC + SKIN + 0.3)
    assert below(A, RC + SKIN + 0.3) == len(A['wider'])
    A['n1'], A['n2'] = below(A, R1), below(A, R2)
    assert len(A['exact']) < A['n1'] < A['n2'] < A['n_skin'] < len(A['wider'])
    # (d): one hydrogen gets a dipole -- the table compiled for the parameters above is stale for these
    stale = dict(A['par'])
    Q = A['par']['Q_local'].copy()
    Q[4, 1:4] = (0.02, -0.01, 0.03)
    stale['Q_local'] = Q
    A['stale'] = stale
    A['want_stale'] = run(pme(box, A['at'], A['ai'], A['cov']), A['pos'], A['box'], A['exact'], stale, True)
    assert np.abs(A['want_stale']['G'] - A['want']['G']).max() > 1e-6      # (another system, not the same numbers twice)
    yield w
    settings.PRECISION = old


def handle(w, s):
    return pme(w['box'], s['at'], s['ai'], s['cov'], cutoff=RC)


def check(f, s, pairs, n_before, n_after, what, par=None, want=None):
    """One evaluation: admp_num_pairs before it (None: not asserted) and after it, the numbers against the exact list's."""
    if n_before is not None:
        assert f.n_pairs == n_before, (what, f.n_pairs, n_before)
    got = run(f, s['pos'], s['box'], pairs, par or s['par'], True)
    want = want or s['want']
    same(got, want, True, 1e-10, 1e-10, what)
    assert got['n'] == want['n'], (what, got['n'], want['n'])
    assert f.n_pairs == n_after, (what, f.n_pairs, n_after)


def retopo(f, s):
    """admp_set_topology of system s on a live handle (the Python class sets a topology only when it is created)."""
    ptr, col, val = covalent_to_csr(s['cov'], s['na'])
    at = np.ascontiguousarray(s['at'], dtype=np.int32)
    ai = np.ascontiguousarray(s['ai'], dtype=np.int32)
    p = [a.ctypes.data_as(ctypes.c_void_p) for a in (at, ai, ptr, col, val)]
    _lib.check(f._h, f._L.admp_set_topology(f._h, s['na'], *p), 'admp_set_topology')
    f.n_atoms = s['na']
    f._pairs_key = f._pairs_keep = f._lender = f._pol_key = None
    assert f.n_pairs == 0


def refused(f, s, text, code=_lib.E_ARG):
    with pytest.raises(_lib.AdmpHipError) as e:
        run(f, s['pos'], s['box'], None, s['par'], True)
    assert text in str(e.value) and '(code %d)' % code in str(e.value), str(e.value)


def pruned_handle(w, A):
    """A handle whose table was built from positions, compiled for the classes, and pruned to R1."""
    f = handle(w, A)
    f.update_neighbors(A['pos'], A['box'], rc=RC + SKIN)
    check(f, A, None, A['n_skin'], A['n_skin'], 'built from positions')
    f.prune_neighbors(A['pos'], A['box'], R1)
    check(f, A, None, A['n1'], A['n1'], 'pruned')
    return f


def test_a_set_pairs_and_the_first_class_compile(world):
    A = world['A']
    f = handle(world, A)
    assert f.n_pairs == 0
    check(f, A, A['skin'], None, A['n_skin'], 'first evaluation (compiles the classes)')
    check(f, A, A['skin'], A['n_skin'], A['n_skin'], 'second evaluation')


def test_b_prune_and_prune_again(world):
    A = world['A']
    f = handle(world, A)
    f.update_neighbors(A['pos'], A['box'], rc=RC + SKIN)
    f.prune_neighbors(A['pos'], A['box'], R1)
    # the first evaluation of a handle compiles the classes into the table as built: it ends the pruning
    check(f, A, None, A['n1'], A['n_skin'], 'pruned before the first evaluation')
    f.prune_neighbors(A['pos'], A['box'], R1)
    check(f, A, None, A['n1'], A['n1'], 'pruned at R1')
    f.prune_neighbors(A['pos'], A['box'], R2)
    check(f, A, None, A['n2'], A['n2'], 'pruned at R2')
    f.prune_neighbors(A['pos'], A['box'], R1)
    check(f, A, None, A['n1'], A['n1'], 'pruned at R1 again')
    f.prune_neighbors(A['pos'], A['box'], 0.0)
    check(f, A, None, A['n_skin'], A['n_skin'], 'rc <= 0: the table as built')


def test_c_a_new_list_on_a_pruned_table(world):
    A = world['A']
    f = pruned_handle(world, A)
    check(f, A, A['wider'], A['n1'], len(A['wider']), 'new list while pruned')
    f.prune_neighbors(A['pos'], A['box'], R2)
    check(f, A, None, A['n2'], A['n2'], 'pruned again')
    f.update_neighbors(A['pos'], A['box'], rc=RC + SKIN)
    check(f, A, None, A['n_skin'], A['n_skin'], 'rebuilt from positions while pruned')


def test_d_stale_classes_on_a_pruned_table(world):
    A = world['A']
    f = pruned_handle(world, A)
    # the sites disagree with the classes: this evaluation ignores them, the next one recompiles the table as built
    check(f, A, None, A['n1'], A['n1'], 'stale classes', A['stale'], A['want_stale'])
    check(f, A, None, A['n1'], A['n_skin'], 'recompiled table', A['stale'], A['want_stale'])
    check(f, A, None, A['n_skin'], A['n_skin'], 'recompiled table, again', A['stale'], A['want_stale'])
    f.prune_neighbors(A['pos'], A['box'], R2)
    check(f, A, None, A['n2'], A['n2'], 'recompiled table, pruned', A['stale'], A['want_stale'])


def test_e_a_borrower_follows_its_lender(world):
    A, B = world['A'], world['B']
    lender, b = handle(world, A), handle(world, A)
    lender.set_pairs(A['skin'])
    b.share_neighbors(lender)
    check(b, A, None, A['n_skin'], A['n_skin'], 'borrowed, before the lender evaluated')
    check(lender, A, None, A['n_skin'], A['n_skin'], 'lender (compiles the classes)')
    check(b, A, None, A['n_skin'], A['n_skin'], 'borrowed, classes compiled')
    lender.set_pairs(A['wider'])
    check(b, A, None, None, len(A['wider']), 'the lender got a new list')
    lender.prune_neighbors(A['pos'], A['box'], R1)
    check(b, A, None, None, A['n1'], 'the lender pruned')
    check(lender, A, None, A['n1'], A['n1'], 'lender, pruned')
    check(b, A, A['skin'], None, A['n_skin'], 'a list of its own ends the loan')
    check(lender, A, None, A['n1'], A['n1'], 'lender after the loan')
    b.share_neighbors(lender)
    check(b, A, None, A['n1'], A['n1'], 'borrowed again')
    retopo(lender, B)
    refused(b, A, NO_PAIRS)
    assert b.n_pairs == 0
    _lib.check(lender._h, lender._L.admp_destroy(lender._h), 'admp_destroy')
    lender._h = ctypes.c_void_p()
    refused(b, A, 'the handle the neighbour table was borrowed from has been destroyed')
    refused(b, A, NO_PAIRS)                       # (the loan is over: an ordinary handle without a list)
    check(b, A, A['skin'], 0, A['n_skin'], 'a list of its own after the lender is gone')


def test_f_another_topology_while_pruned_and_while_borrowing(world):
    A, B = world['A'], world['B']
    f = pruned_handle(world, A)
    retopo(f, B)
    check(f, B, B['skin'], 0, B['n_skin'], 'another topology while pruned')
    lender = handle(world, B)
    lender.set_pairs(B['skin'])
    f.share_neighbors(lender)
    check(f, B, None, B['n_skin'], B['n_skin'], 'borrowed')
    retopo(f, A)
    check(f, A, A['skin'], 0, A['n_skin'], 'another topology while borrowing')
    check(lender, B, None, B['n_skin'], B['n_skin'], 'the lender keeps its table')
    # (the first look at the class flags is spent: a later table of this handle gets its classes at the second evaluation)
    check(f, A, None, A['n_skin'], A['n_skin'], 'classes compiled')
    f.prune_neighbors(A['pos'], A['box'], R1)
    check(f, A, None, A['n1'], A['n1'], 'pruned after all that')


def test_g_neighbor_count_and_fill(world):
    A, B = world['A'], world['B']
    f = handle(world, A)
    L, h = f._L, f._h
    pos = torch.as_tensor(A['pos'], dtype=torch.float64).cuda()
    box = _lib.darr(np.asarray(A['box'], dtype=np.float64).reshape(-1))

    def count():
        n = ctypes.c_int64(0)
        with f._on_stream():
            _lib.check(h, L.admp_neighbor_count(h, A['na'], ctypes.c_void_p(pos.data_ptr()), box, RC, ctypes.byref(n)),
                       'admp_neighbor_count')
        return int(n.value)

    def fill(n):
        out = torch.full((n, 2), -1, dtype=torch.int32, device='cuda')
        rc = L.admp_neighbor_fill(h, ctypes.c_void_p(out.data_ptr()))
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()

    def listed(p):
        p = np.sort(p, axis=1)
        return p[np.lexsort((p[:, 1], p[:, 0]))]

    n = count()
    assert n == len(A['exact'])
    rc, got = fill(n)
    assert rc == 0 and np.array_equal(listed(got), A['exact'])
    rc, got = fill(n)
    assert rc == _lib.E_ARG and b'admp_neighbor_count must precede admp_neighbor_fill' in L.admp_last_error(h)
    assert (got == -1).all() and f.n_pairs == 0
    # the pending count belongs to the positions it was taken at, not to the handle's topology
    assert count() == n
    retopo(f, B)
    rc, got = fill(n)
    assert rc == 0 and np.array_equal(listed(got), A['exact'])
    check(f, B, B['skin'], 0, B['n_skin'], 'evaluates after the search')
