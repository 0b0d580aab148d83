"""The neighbour kernels (admp_amd/csrc/cell_kernels.hip, nbr_kernels.hip) at the edges of every path, against the float64
brute-force reference of tests/neighbour_ref.py (inputs and reference are proved sound without a GPU in
tests/test_neighbour_ref_cpu.py).

(a) pair-list builder   NeighborList.allocate (k_cell_bin / k_cell_sort / k_cell_pairs): the launch shapes, 2 / 3 / mixed cell
                        counts, a box edge that is a multiple of rc, atoms on cell faces and the fold, far outside the cell,
                        skewed cells, one full cell among empty ones, the 1024-per-axis clamp, the 64 M-cell halving, refusals.
                        double: the reference's set.  single: differences only within band of rc; the margin is printed.
(b) fused table builder update_neighbors then pairs=None (k_brute_rows up to 4096 atoms, k_cell_rows above), observed through
                        the hand-written Tang-Toennies kernel: n_pairs, energy, gradient, and dE/dmScales -- the covalent
                        class packed into every entry -- against oracle.admp_oracle on the reference pairs.
(c) list compiler       set_pairs (k_nbr_count / k_nbr_fill / k_nbr_rank_sort): the three paths of the rank sort in one table,
                        the 64 / 65 switch, the ways a list can arrive (wave_runs), duplicates, the second grid-stride round.
Tolerances: double 1e-11 relative; single 2e-5 (energy) and 2e-4 (gradient, dE/dmScales) plus the summed |pair term| of the
reference pairs within band of rc (from the reference, never from the output)."""
import ctypes

import numpy as np
import pytest

from admp_amd import settings
from tests import neighbour_ref as R

pytestmark = pytest.mark.gpu

PRECS = ('double', 'single')


@pytest.fixture()
def precision():
    old = settings.PRECISION
    yield
    settings.PRECISION = old


# ---- (a) pair-list builder ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,prec', [(n, p) for n in R.PAIRLIST_CASES for p in PRECS
                                       if not (p == 'single' and n in R.DOUBLE_ONLY)])
def test_pair_list_matches_brute_force(precision, name, prec):
    from admp_amd.neighbor import NeighborList
    settings.PRECISION = prec
    c = R.pairlist_case(name)
    assert prec in c['precs']
    nbl = NeighborList(c['box'], c['rc'])
    got = nbl.allocate(np.array(c['pos']))
    assert got.dtype.is_floating_point is False and tuple(got.shape[1:]) == (2,)
    got = got.cpu().numpy()
    margin = R.check_pair_list(got, c['pos'], c['box'], c['rc'], c['ref_pairs'], prec)
    print('MARGIN %s %s pairs %d |r-rc|/band %.4f' % (name, prec, len(got), margin))
    if len(c['ref_pairs']) == 0:
        assert got.shape == (0, 2)
    if c['exact']:
        s = R.as_set(got)
        assert tuple(sorted(c['absent'])) not in s and tuple(sorted(c['present'])) in s
    again = nbl.update(np.array(c['pos'])).cpu().numpy()         # same handle, scratch reused: the same list, row for row
    assert np.array_equal(again, got)


def test_pair_list_refusals(precision):
    """rc above half a height, rc <= 0, no atoms, a singular box: error returns (checked before anything is launched), and
    the handle still serves a valid call afterwards"""
    from admp_amd import _lib
    from admp_amd.neighbor import NeighborList
    settings.PRECISION = 'double'
    c = R.pairlist_case('na65')
    pos = np.array(c['pos'])
    nbl = NeighborList(c['box'], c['rc'])
    for box, rc, p, msg in ((c['box'], 10.0 * (1 + 1e-9), pos, 'half the box height'),
                            (np.array([[14.0, 0, 0], [2.5, 13.0, 0], [-1.5, 2.0, 15.0]]), 6.5, pos, 'half the box height'),
                            (c['box'], 0.0, pos, 'bad argument'), (c['box'], -1.0, pos, 'bad argument'),
                            (c['box'], 5.0, np.zeros((0, 3)), 'bad argument'),
                            (np.array([[20.0, 0, 0], [0, 20.0, 0], [20.0, 20.0, 0]]), 5.0, pos, 'singular box')):
        nbl.rc = rc
        with pytest.raises(_lib.AdmpHipError, match=msg):
            nbl.allocate(p, box=box)
    nbl.rc = c['rc']
    got = nbl.allocate(pos, box=c['box']).cpu().numpy()
    R.check_pair_list(got, c['pos'], c['box'], c['rc'], c['ref_pairs'], 'double')
    # a fill without a count, and a NULL output after a non-zero count, are refused; NULL after a zero count is the contract
    L, h = nbl._L, nbl._h
    assert L.admp_neighbor_fill(h, None) != 0
    import torch
    dev = torch.as_tensor(pos, device='cuda')
    n = ctypes.c_int64(-1)
    assert L.admp_neighbor_count(h, len(pos), dev.data_ptr(), _lib.darr(c['box'].reshape(-1)), c['rc'], ctypes.byref(n)) == 0
    assert n.value == len(c['ref_pairs']) and L.admp_neighbor_fill(h, None) != 0
    one = torch.as_tensor(pos[:1].copy(), device='cuda')
    assert L.admp_neighbor_count(h, 1, one.data_ptr(), _lib.darr(c['box'].reshape(-1)), c['rc'], ctypes.byref(n)) == 0
    assert n.value == 0 and L.admp_neighbor_fill(h, None) == 0
    assert L.admp_neighbor_fill(h, None) != 0                      # the pending count was spent


def test_a_refused_build_leaves_the_list_as_it_was(precision):
    """A list build or a count that is refused for its arguments changes nothing: the inner list stays in force, a loan goes
    on, the pending count still belongs to its own box."""
    import torch
    from admp_amd import _lib
    from tests.test_gpu_pair_list_states import R1, below, handle, system
    from tests.test_gpu_pme_cutoff import RC, SKIN
    settings.PRECISION = 'double'
    A = system(216, 36)
    w = dict(box=A['box'])
    n_skin, n1 = below(A, RC + SKIN), below(A, R1)
    too_far = 0.5 * A['box'][0, 0] * 1.01
    f, b = handle(w, A), handle(w, A)
    f.update_neighbors(A['pos'], A['box'], rc=RC + SKIN)
    f.prune_neighbors(A['pos'], A['box'], R1)
    b.share_neighbors(f)
    assert f.n_pairs == n1 < n_skin and b.n_pairs == n1
    for g in (f, b):
        with pytest.raises(_lib.AdmpHipError, match='half the box height'):
            g.update_neighbors(A['pos'], A['box'], rc=too_far)
        assert g._L.admp_set_pairs(g._h, -1, None, 1) == _lib.E_ARG and b'negative pair count' in g._L.admp_last_error(g._h)
        assert g.n_pairs == n1
    f.prune_neighbors(A['pos'], A['box'], 0.0)
    assert f._L.admp_synchronize(b._h) == 0 and b.n_pairs == n_skin      # (any call of the borrower: it still follows f)
    # a refused count leaves the pending one alone
    L, h = f._L, f._h
    pos = torch.as_tensor(A['pos'], device='cuda')
    box = _lib.darr(np.asarray(A['box'], dtype=np.float64).reshape(-1))
    n, m = ctypes.c_int64(0), ctypes.c_int64(0)
    assert L.admp_neighbor_count(h, A['na'], pos.data_ptr(), box, RC, ctypes.byref(n)) == 0 and n.value == len(A['exact'])
    assert L.admp_neighbor_count(h, A['na'], pos.data_ptr(), box, too_far, ctypes.byref(m)) == _lib.E_ARG
    out = torch.full((n.value, 2), -1, dtype=torch.int32, device='cuda')
    assert L.admp_neighbor_fill(h, out.data_ptr()) == 0
    torch.cuda.synchronize()
    got = np.sort(out.cpu().numpy(), axis=1)
    assert np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], A['exact'])


# ---- (b), (c): the Tang-Toennies observable ------------------------------------------------------------------------------------
def tt_calculator(s):
    from admp_amd.pairwise import generate_pairwise_interaction, TT_damping_qq_c6_kernel
    return generate_pairwise_interaction(TT_damping_qq_c6_kernel, s['cov'], static_args={})


def tt_observe(pot, s, pairs, want_dm=True):
    pos, box = np.array(s['pos']), np.array(s['box'])
    E, G = pot.value_and_grad(pos, box, pairs, R.MSCALES, *s['params'])
    dm = pot.get_mscale_gradient(pos, box, None, R.MSCALES, *s['params']) if want_dm else None
    return dict(E=float(E), grad=np.asarray(G, dtype=np.float64), dm=dm, n_pairs=pot.n_pairs)


def check_from_positions(pot, name, prec, rc=None):
    s = R.table_system(name)
    pairs, r, ref, slack, n_band = R.table_reference(name, rc)
    pot.update_neighbors(np.array(s['pos']), np.array(s['box']), rc=s['rc'] if rc is None else rc)
    got = tt_observe(pot, s, None)
    print('TT %s %s rc %s pairs %d/%d E %.12e ref %.12e band pairs %d' % (name, prec, rc, got['n_pairs'], len(pairs), got['E'],
                                                                      ref['E'], n_band))
    R.check_tt(got, ref, prec, slack if prec == 'single' else (0, 0, 0), n_pairs_ref=len(pairs), n_band=n_band)
    return got


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name', ['gas1', 'gas15', 'gas16', 'gas17', 'gas1023', 'gas1024', 'gas1025', 'gas4096',    # brute rows
                                  'gas4097', 'gas4200', 'gas4097_tri', 'gas4200_tri'])                              # cell rows
def test_table_from_positions(precision, name, prec):
    settings.PRECISION = prec
    got = check_from_positions(tt_calculator(R.table_system(name)), name, prec)
    if name == 'gas1':
        assert got['n_pairs'] == 0 and got['E'] == 0.0 and not got['grad'].any()


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name', ['stars40', 'stars470'])
def test_more_than_six_covalent_partners(precision, name, prec):
    """eight partners on every atom: the rows' register window (kEx = 6) overflows into its loop in k_brute_rows (360 atoms)
    and k_cell_rows (4230); the same systems through an explicit list (lookup_nbonds in k_nbr_fill)"""
    settings.PRECISION = prec
    s = R.table_system(name)
    pot = tt_calculator(s)
    a = check_from_positions(pot, name, prec)
    pairs, r, ref, slack, n_band = R.table_reference(name)
    assert ref['dm'][0] != 0 and ref['dm'][1] != 0               # both bonded classes carry weight in the reference
    b = tt_observe(tt_calculator(s), s, pairs.astype(np.int32))
    R.check_tt(b, ref, prec, (0, 0, 0), n_pairs_ref=len(pairs))  # (an explicit list: nothing is classified by distance)
    if prec == 'double':
        assert abs(a['E'] - b['E']) <= 1e-11 * abs(ref['E'])
        assert np.linalg.norm(a['grad'] - b['grad']) <= 1e-11 * np.linalg.norm(ref['grad'])


@pytest.mark.parametrize('prec', PRECS)
def test_table_buffer_growth_on_the_cell_path(precision, prec):
    """one calculator, rc 3.0 -> 5.5 -> 4.0: a short list, one that outgrows the buffer (the optimistic fill is repeated
    after the growth), a shorter one into the grown buffer"""
    settings.PRECISION = prec
    pot = tt_calculator(R.table_system('gas4200'))
    for rc in (3.0, 5.5, 4.0):
        check_from_positions(pot, 'gas4200', prec, rc)


@pytest.mark.parametrize('prec', PRECS)
def test_no_pair_at_all_from_positions(precision, prec):
    settings.PRECISION = prec
    pot = tt_calculator(R.table_system('dilute'))
    got = check_from_positions(pot, 'dilute', prec)
    assert got['n_pairs'] == 0 and got['E'] == 0.0 and not got['grad'].any() and not np.asarray(got['dm']).any()
    got = check_from_positions(pot, 'dilute', prec, 25.0)            # the same calculator then builds a real table
    assert got['n_pairs'] > 100


@pytest.mark.parametrize('prec', PRECS)
def test_retopologised_handle(precision, prec):
    """The C ABI lets one handle take a second topology.  5000 atoms (cell rows: 4 partial counts per atom), then 2000
    (brute rows: 16 per atom, more words than the first system needed): each build against the reference."""
    import torch
    from admp_amd import _lib
    from admp_amd._device import covalent_to_csr
    L = _lib.load()
    nbytes = 8 if prec == 'double' else 4
    dt = torch.float64 if prec == 'double' else torch.float32
    h = ctypes.c_void_p()
    assert L.admp_create(ctypes.byref(h), torch.cuda.current_device(), nbytes) == 0
    try:
        _lib.check(h, L.admp_use_default_stream(h), 'admp_use_default_stream')
        for name in ('gas5000', 'gas2000'):
            s = R.table_system(name)
            pairs, r, ref, slack, n_band = R.table_reference(name)
            na = len(s['pos'])
            ptr, col, val = covalent_to_csr(s['cov'], na)
            vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)     # noqa: E731
            _lib.check(h, L.admp_set_topology(h, na, None, None, vp(ptr), vp(col), vp(val)), 'admp_set_topology')
            pos = torch.as_tensor(np.array(s['pos']), dtype=dt, device='cuda')
            par = torch.as_tensor(np.stack(s['params'], axis=1), dtype=dt, device='cuda').contiguous()
            grad = torch.empty((na, 3), dtype=dt, device='cuda')
            box = _lib.darr(s['box'].reshape(-1))
            _lib.check(h, L.admp_set_pairs_from_positions(h, pos.data_ptr(), box, s['rc']), 'admp_set_pairs_from_positions')
            E = (ctypes.c_double * 1)()
            _lib.check(h, L.admp_tt_energy_grad(h, pos.data_ptr(), box, par.data_ptr(), 5, _lib.darr(R.MSCALES), E,
                                                grad.data_ptr(), 1), 'admp_tt_energy_grad')
            dm = (ctypes.c_double * 5)()
            _lib.check(h, L.admp_mscale_grad(h, 2, pos.data_ptr(), box, par.data_ptr(), 0, 5, dm, 1), 'admp_mscale_grad')
            got = dict(E=float(E[0]), grad=grad.cpu().numpy().astype(np.float64), dm=np.array(dm[:]),
                       n_pairs=int(L.admp_num_pairs(h)))
            R.check_tt(got, ref, prec, slack if prec == 'single' else (0, 0, 0), n_pairs_ref=len(pairs), n_band=n_band)
    finally:
        L.admp_destroy(h)


def test_covalent_class_eight_is_refused():
    """three bits of a table entry hold the class: 8 is refused by the Python check and by admp_set_topology; no launch"""
    from admp_amd import _lib
    import torch
    s = R.table_system('gas16')
    cov = s['cov'].toarray()
    cov[0, 1] = cov[1, 0] = 7
    tt_calculator(dict(s, cov=cov))                                  # 7 is the largest class
    cov[0, 1] = cov[1, 0] = 8
    with pytest.raises(ValueError, match=r'0\.\.7'):
        tt_calculator(dict(s, cov=cov))
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.admp_create(ctypes.byref(h), torch.cuda.current_device(), 8) == 0
    try:
        ptr, col = np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)             # noqa: E731
        assert L.admp_set_topology(h, 2, None, None, vp(ptr), vp(col), vp(np.array([7, 7], dtype=np.int32))) == 0
        assert L.admp_set_topology(h, 2, None, None, vp(ptr), vp(col), vp(np.array([8, 8], dtype=np.int32))) != 0
        assert b'0..7' in L.admp_last_error(h)
    finally:
        L.admp_destroy(h)


# ---- (c) explicit-list compiler --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name', ['sort_paths', 'switch65'])
def test_rank_sort_paths(precision, name, prec):
    """sort_paths: rows of 342+ entries (32 of them outgrow the 8192-entry LDS segment: entries read from global memory),
    rows of at most 64 (registers) and rows of 99 (general path, LDS) in one table.  switch65: rows of exactly 64 and 65
    entries.  The table from positions of the same system agrees to 1e-11 in double (another summation order)."""
    settings.PRECISION = prec
    s = R.table_system(name)
    pairs, r, ref, slack, n_band = R.table_reference(name)
    got = tt_observe(tt_calculator(s), s, pairs.astype(np.int32))
    R.check_tt(got, ref, prec, (0, 0, 0), n_pairs_ref=len(pairs))
    fused = check_from_positions(tt_calculator(s), name, prec)
    if prec == 'double':
        assert abs(fused['E'] - got['E']) <= 1e-11 * abs(ref['E'])
        assert np.linalg.norm(fused['grad'] - got['grad']) <= 1e-11 * np.linalg.norm(ref['grad'])
        assert np.abs(fused['dm'] - got['dm']).max() <= 1e-11 * np.abs(ref['dm']).max()


def test_list_arrival_orders(precision):
    """wave_runs: one list fed sorted by i, fully shuffled, sorted with invalid rows spliced inside the runs, and with runs
    of one i exactly 64, 65 and 130 rows long starting at lanes 0, 1 and 63 of a wavefront: one result, one n_pairs"""
    settings.PRECISION = 'double'
    s = R.table_system('sort_paths')
    pairs, r, ref, slack, n_band = R.table_reference('sort_paths')
    na = len(s['pos'])
    rng = np.random.default_rng(5)
    P = pairs.astype(np.int32)
    bad = np.array([[5, 5], [9, 3], [-1, 4], [-7, -2], [3, na], [na, na + 1], [0, 2 ** 31 - 1]], dtype=np.int32)
    where = np.sort(rng.integers(1, len(P), 400))
    spliced = np.insert(P, where, bad[rng.integers(0, len(bad), 400)], axis=0)
    # atom i of the block (atoms 0..342, every pair of them listed) leads 342 - i rows, plus none outside the block
    first = np.searchsorted(P[:, 0], np.arange(na + 1))
    runs = {}
    for i, want in ((278, 64), (277, 65), (212, 130)):
        runs[i] = P[first[i]:first[i + 1]]
        assert len(runs[i]) == want
    rest = P[~np.isin(P[:, 0], list(runs))]
    pad = lambda n: np.full((n, 2), na, dtype=np.int32)              # noqa: E731
    # rows 0..63 run 278 (lane 0), 1 pad, run 277 from row 65 (lane 1), pads to row 191, run 212 from row 191 (lane 63)
    placed = np.concatenate([runs[278], pad(1), runs[277], pad(191 - 130), runs[212], rest])
    assert (placed[0:64, 0] == 278).all() and (placed[65:130, 0] == 277).all() and (placed[191:321, 0] == 212).all()
    assert 65 % 64 == 1 and 191 % 64 == 63
    forms = dict(sorted=P, shuffled=P[rng.permutation(len(P))], spliced=spliced, placed=placed)
    out = {}
    for k, lst in forms.items():
        out[k] = tt_observe(tt_calculator(s), s, np.ascontiguousarray(lst))
        R.check_tt(out[k], ref, 'double', (0, 0, 0), n_pairs_ref=len(pairs))
    for k in ('shuffled', 'spliced', 'placed'):
        # rows are sorted by partner after the fill, so the summation order does not depend on the arrival order
        # (row by row: the gradient is bit-equal; the energy is a sum of workgroup sums added in the order they finish)
        assert np.array_equal(out[k]['grad'], out['sorted']['grad']), k
        assert abs(out[k]['E'] - out['sorted']['E']) <= 1e-13 * abs(ref['E']), k


def test_duplicate_rows_count_twice(precision):
    """the reference sums over the rows it is given: a pair listed twice counts twice, and n_pairs counts the rows"""
    settings.PRECISION = 'double'
    s = R.table_system('gas1024')
    pairs = s['ref_pairs']
    rng = np.random.default_rng(9)
    dup = pairs[rng.choice(len(pairs), 100, replace=False)]
    lst = np.concatenate([pairs, dup])
    lst = lst[rng.permutation(len(lst))]
    ref = R.tt_reference(s, lst)
    once = R.tt_reference(s, pairs, want_mscale=False)
    assert abs(ref['E'] - once['E']) > 1e-6 * abs(once['E'])         # the doubled rows are visible in the reference
    got = tt_observe(tt_calculator(s), s, lst.astype(np.int32))
    R.check_tt(got, ref, 'double', (0, 0, 0), n_pairs_ref=len(pairs) + 100)


def test_second_grid_stride_round(precision):
    """8192 workgroups of 256 rows cover 2 097 152 rows per round: 300 rows more, valid rows at both ends of the list"""
    settings.PRECISION = 'double'
    s = R.table_system('gas1024')
    na = len(s['pos'])
    rng = np.random.default_rng(10)
    valid = s['ref_pairs'][np.sort(rng.choice(len(s['ref_pairs']), 3000, replace=False))].astype(np.int32)
    n_rows = 8192 * 256 + 300
    lst = np.full((n_rows, 2), na, dtype=np.int32)
    lst[:1500] = valid[:1500]
    lst[-1500:] = valid[1500:]                                         # the last 300 rows belong to the second round
    ref = R.tt_reference(s, valid)
    got = tt_observe(tt_calculator(s), s, lst)
    R.check_tt(got, ref, 'double', (0, 0, 0), n_pairs_ref=3000)
