"""tests/slab_ref.py on the CPU: the reference of the slab decomposition is consistent with itself, and every case has what it
is there for.

* imports(r <- t), worked out from the reader's side, equal exports(t -> r), worked out from the owner's side through the
  symmetry of the table and the inverse frame map, as lists, for all r, t; the home lists partition the atoms.
* The table's rule: rows 0 <= i < j < Na of the list, both directions (reversed rows, self pairs and padding dropped).
* Features: export masks with several bits, imports from a non-adjacent rank, an empty per-peer list, a frame across a slab
  face, migrants in both directions -- per case, as listed in FEATURES.
* No atom lies within 1e-3 of a mesh plane in u units.  That is a condition, not a measurement: u is rounded to the handle's
  type on the device, in f32 with an error of order K0 2^-24 = 3e-6, so ownership is the same in both types and in the
  float64 reference.  The number of atoms excluded for it is zero in every case (asserted).  The exact case stands the other
  way round: its atoms lie ON planes, with u = 2 x computed exactly in both types (asserted).  The case that builds its table
  from positions has no pair within 1e-5 A of the cutoff either.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import slab_ref as R      # noqa: E402

MULTIBIT, NONADJACENT, EMPTY, FRAME_ACROSS, FRAME_NONADJACENT, MIGRANTS, NOT_POLAR = range(7)
FEATURES = {name: {FRAME_ACROSS} for name in R.CASES}
for name in ('w64_n8', 'w342_n8', 'w64_n5', 'general_n8', 'migrants_n8'):
    FEATURES[name] |= {MULTIBIT, NONADJACENT}
for name in ('w1366_n8', 'w1366_n5', 'w342_n5'):
    FEATURES[name] |= {MULTIBIT, EMPTY}
for name in ('general_n5', 'general_n8'):
    FEATURES[name] |= {FRAME_NONADJACENT}
for name in ('migrants_n3', 'migrants_n8'):
    FEATURES[name] |= {MIGRANTS}
FEATURES['nopol_n3'] |= {NOT_POLAR}


def adjacent(r, t, N):
    return (r - t) % N in (1, N - 1)


@pytest.mark.parametrize('name', list(R.CASES))
def test_reference_is_consistent_and_the_case_has_its_features(name):
    c, ref = R.case(name), R.reference(name)
    N, na = c['N'], c['na']
    configs = [(ref['owner'], ref['ranks'], c['pos'])]
    if 'owner2' in ref:
        configs.append((ref['owner2'], ref['ranks2'], c['pos2']))
    axes = R.axis_atoms(c['at'], c['ai'])
    for owner, ranks, pos in configs:
        # the condition on the positions
        d = R.plane_distance(pos, c['box'], c['K0'])
        if c['exact']:
            u = R.u_of(pos, c['box'], c['K0'])
            assert np.array_equal(u, 2.0 * pos[:, 0]) and np.array_equal(2.0 * u, np.round(2.0 * u))
            assert np.array_equal(pos.astype(np.float32).astype(np.float64), pos)
            assert (d == 0).sum() >= na // 3
            edges = R.slab_edges(c['K0'], N)
            base = np.mod(u[d == 0].astype(np.int64) - 3, c['K0'])
            assert np.isin(base, edges[:-1]).sum() >= 2            # atoms exactly on slab faces
        else:
            assert int((d < R.MARGIN).sum()) == 0, (name, 'atoms within the margin of a plane', int((d < R.MARGIN).sum()))
        # partition
        homes = np.concatenate([np.array(r['home'], dtype=np.int64) for r in ranks])
        assert np.array_equal(np.sort(homes), np.arange(na))
        for r in range(N):
            assert np.array_equal(np.array(ranks[r]['home']), np.nonzero(owner == r)[0])
            assert ranks[r]['imports'][r] == [] and ranks[r]['exports'][r] == []
            for t in range(N):
                assert ranks[r]['imports'][t] == ranks[t]['exports'][r], (name, r, t)
                assert ranks[r]['imports'][t] == sorted(ranks[r]['imports'][t])
            # bits: what the lists say, nothing else
            b = ranks[r]['bits']
            assert np.array_equal(np.nonzero(b & R.K_HOME)[0], np.array(ranks[r]['home']))
            assert np.array_equal(np.nonzero(b & R.K_POLAR)[0], np.array(ranks[r]['act'], dtype=np.int64))
            for t in range(N):
                if t != r:
                    assert np.array_equal(np.nonzero(((b & R.K_HOME) == 0) & (((b >> t) & 1) == 1))[0],
                                          np.array(ranks[r]['imports'][t], dtype=np.int64))
    owner, ranks = ref['owner'], ref['ranks']
    f = FEATURES[name]
    peers = (1 << 28) - 1
    if MULTIBIT in f:
        assert any(bin(int(w) & peers).count('1') >= 2 for r in ranks for w in r['bits'][r['home']]), name
    if NONADJACENT in f:
        assert any(ranks[r]['imports'][t] for r in range(N) for t in range(N) if t != r and not adjacent(r, t, N)), name
    if EMPTY in f:
        assert any(not ranks[r]['imports'][t] for r in range(N) for t in range(N) if t != r), name
    if FRAME_ACROSS in f:
        assert any(owner[a] != owner[i] for i in range(na) for a in axes[i]), name
    if FRAME_NONADJACENT in f:
        assert any(owner[a] != owner[i] and not adjacent(owner[a], owner[i], N) for i in range(na) for a in axes[i]), name
        assert {int(t) for t in c['at']} == {R.ZBISECT, R.THREEFOLD, R.ZONLY}
        assert all(len(axes[i]) == R.N_AXIS_ATOMS[int(c['at'][i])] for i in range(na))
    if MIGRANTS in f:
        n_in = [sum(len(m) for m in ref['mig'][r][0]) for r in range(N)]
        n_out = [sum(len(m) for m in ref['mig'][r][1]) for r in range(N)]
        assert all(a + b > 0 for a, b in zip(n_in, n_out)), (name, n_in, n_out)
        assert sum(1 for a, b in zip(n_in, n_out) if a > 0 and b > 0) >= (N + 1) // 2, (name, n_in, n_out)
        assert sum(len(m) for r in range(N) for m in ref['mig'][r][0]) == int((ref['owner'] != ref['owner2']).sum())
    if NOT_POLAR in f:
        assert not c['lpol'] and all(not r['act'] for r in ranks) and not any((r['bits'] & R.K_POLAR).any() for r in ranks)
    else:
        assert all(r['act'] for r in ranks) and any(len(r['act']) < len(r['home']) for r in ranks)      # pol = 0 on a third
    if c['from_positions']:
        from tests.pair_ref import distances
        assert np.abs(distances(c['pos'], c['box'], np.stack(np.triu_indices(na, 1), axis=1)) - c['rc']).min() > 1e-5


def test_sizes_cross_the_chunk_and_the_span():
    assert [R.case('w%d_n2' % n)['na'] for n in (64, 342, 1366)] == [192, 1026, 4098]      # 3 * 64, 1024 + 2, 4 * 1024 + 2
    for name in ('w64_n8', 'w342_n8', 'w1366_n8'):
        e = R.slab_edges(48, 8)
        assert all(b - a == 6 for a, b in zip(e[:-1], e[1:]))
    c = R.case('w64_n8')
    assert 6 * c['box'][0, 0] / 48 < c['rc']                                                # thinner than the cutoff


def test_the_table_drops_rows_by_the_reference_rule():
    """rows with i >= j, negative or too large indices are dropped (admp/pme.py: pairs[pairs[:, 0] < pairs[:, 1]]); a row of the
    table holds both directions of the rest"""
    pairs = np.array([[0, 1], [1, 0], [2, 2], [1, 3], [3, 1], [-1, 2], [2, 5], [4, 4], [0, 3], [0, 3]])
    t = R.pair_table(pairs, 5)
    assert t == [[1, 3], [0, 3], [], [0, 1], []]
    axes = R.axis_atoms([R.ZONLY, R.ZTHENX, R.ZBISECT, R.NOAXIS, R.THREEFOLD, R.BISECTOR],
                        [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2], [0, -1, 4]])
    assert axes == [[1], [0, 2], [0, 1, 3], [], [0, 1, 2], [0]]
    assert R.inverse_frames(axes) == [[1, 2, 4, 5], [0, 2, 4], [1, 4], [2], [], []]


def test_owner_rule_on_exact_planes():
    box = np.eye(3) * 16.0
    pos = np.array([[0.0, 1, 1], [1.5, 1, 1], [1.75, 1, 1], [-0.5, 1, 1], [16.0, 1, 1], [15.75, 1, 1]])
    # u = 0, 3, 3.5, -1, 32, 31.5 -> base = -3, 0, 1, -4, 29, 29 mod 32; slabs of 6, 6, 7, 6, 7 planes
    assert list(R.owners(pos, box, 32, 5)) == [4, 0, 0, 4, 4, 4]
    assert R.slab_edges(32, 5) == [0, 6, 12, 19, 25, 32]
    # u = 9 (on the plane: base 6, the first plane of slab 1), 8.5 (ceil 9: base 6), 8 (base 5, the last plane of slab 0)
    assert list(R.owners(np.array([[4.5, 0, 0], [4.25, 0, 0], [4.0, 0, 0]]), box, 32, 5)) == [1, 1, 0]
