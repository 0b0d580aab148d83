"""The distance constraints without a GPU: the host plan (admp_amd/csrc/con_plan.h) against a Python restatement (union-find
plus the packing rule), array for array, and the per-tile loops of the three kernels run serially by a stand-alone host program
(tests/con_shim/main.cpp) with the arithmetic the kernels compile (md_con_math.h) against a float64 numpy restatement of the
scheme.  tests/test_gpu_md_constraints.py imports the restatements, the system builder and the bar rule.

The restatement repeats the sweep exactly: a cluster's constraints in the caller's order, a converged constraint left alone,
sweeps until one whole sweep changes nothing or max_sweeps is reached.  It handles all clusters at once (the k-th constraint of
every cluster that is still sweeping in one numpy operation); clusters share no atom, so that is the same arithmetic.

Bar rule: that of tests/test_mts_plan_cpu.py (`bars`: 16 x the float32 restatement's deviation from the float64 one, x 2^-29 in
double) plus the stop-rule allowance: two correct runs may stop one sweep apart, which moves r by at most tol d and v by at
most tol d / dt per constraint touching the atom, so 4 tol d_max is added to the position bar and 4 tol d_max / dt to the
velocity bar.  A wrong step is off by 1e-3 and more."""
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_md_random_cpu import CSRC, ROOT, normals
from tests.test_mts_plan_cpu import ACC, BOX, KB, bars, water_system

SHIM = ROOT + '/tests/con_shim/main.cpp'
CROSSINGS = [((0, 0),), ((1, 0),), ((2, 0),), ((0, 1),), ((1, 1),), ((2, 1),), ((0, 0), (1, 0), (2, 0))]


# ---- restatement of the plan ---------------------------------------------------------------------------------------------
def clusters_of(n_atoms, pairs):
    """{smallest atom: ascending atoms} of the connected components of the constraint list"""
    parent = list(range(n_atoms))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i, j in pairs:
        a, b = find(int(i)), find(int(j))
        parent[max(a, b)] = min(a, b)
    comps = {}
    for i in range(n_atoms):
        comps.setdefault(find(i), []).append(i)
    return comps


def plan_restated(n_atoms, pairs, tile_atoms):
    """dict of the plan's arrays, or the (size, smallest atom) of the first cluster that does not fit"""
    comps = clusters_of(n_atoms, pairs)
    tiles = []
    for root in sorted(comps):
        c = comps[root]
        if len(c) > tile_atoms:
            return len(c), root
        if not tiles or sum(map(len, tiles[-1])) + len(c) > tile_atoms:
            tiles.append([])
        tiles[-1].append(c)
    clusters = [c for t in tiles for c in t]
    atom_id = [a for c in clusters for a in c]
    clu_of, local = {}, {}
    k = 0
    for t in tiles:
        s = 0
        for c in t:
            for a in c:
                clu_of[a], local[a] = k, s
                s += 1
            k += 1
    per_clu = [[q for q, p in enumerate(pairs) if clu_of[int(p[0])] == c] for c in range(len(clusters))]
    order = [q for x in per_clu for q in x]
    return dict(n_tiles=len(tiles), n_clusters=len(clusters), max_cluster=max(map(len, clusters)),
                tile_atom0=np.concatenate([[0], np.cumsum([sum(map(len, t)) for t in tiles])]), atom_id=np.array(atom_id),
                tile_clu0=np.concatenate([[0], np.cumsum([len(t) for t in tiles])]),
                clu_atom0=np.concatenate([[0], np.cumsum([len(c) for c in clusters])]),
                clu_con0=np.concatenate([[0], np.cumsum([len(x) for x in per_clu])]), con_order=np.array(order, dtype=int),
                con_slot=np.array([local[int(a)] for q in order for a in pairs[q]], dtype=int))


# ---- restatement of the scheme (dtype of the arrays throughout; float64 is the reference) -------------------------------
class Con:
    """the constraint list as the restatement wants it: pairs (nc, 2), d2 (nc) float64, sweep (n clusters with constraints,
    most constraints of a cluster): the caller's index of the k-th constraint of each cluster, -1 where there is none"""

    def __init__(self, n_atoms, pairs, lengths):
        self.n_atoms = n_atoms
        self.pairs = np.asarray(pairs, dtype=int).reshape(-1, 2)
        self.lengths = np.asarray(lengths, dtype=np.float64).reshape(-1)
        self.d2 = self.lengths * self.lengths
        comps = clusters_of(n_atoms, self.pairs)
        self.comps = [np.array(comps[r]) for r in sorted(comps)]
        root = {a: r for r, c in comps.items() for a in c}
        per = {}
        for q, p in enumerate(self.pairs):
            per.setdefault(root[int(p[0])], []).append(q)
        width = max([len(x) for x in per.values()] + [1])
        self.sweep = np.array([x + [-1] * (width - len(x)) for _, x in sorted(per.items())], dtype=int).reshape(-1, width)


def min_image(d, box):
    ty = d.dtype
    h, hinv = box.astype(ty), np.linalg.inv(box).astype(ty)
    s = d @ hinv
    return (s - np.floor(s + ty.type(0.5))) @ h


def vectors(con, r, box):
    return min_image(r[con.pairs[:, 1]] - r[con.pairs[:, 0]], box) if len(con.pairs) else np.zeros((0, 3), dtype=r.dtype)


def _sweeps(con, max_sweeps, one):
    """the loop of md_con_solve_*: `one(q)` treats the constraints q (one per cluster) and returns (converged, bad)"""
    ncl = len(con.sweep)
    done, bad, sweeps = np.zeros(ncl, dtype=bool), np.zeros(ncl, dtype=bool), np.zeros(ncl, dtype=int)
    for _ in range(max_sweeps):
        run = ~done & ~bad
        if not run.any():
            break
        ok = run.copy()
        for k in range(con.sweep.shape[1]):
            sel = np.nonzero(run & ~bad & (con.sweep[:, k] >= 0))[0]
            if len(sel) == 0:
                continue
            conv, isbad = one(con.sweep[sel, k])
            ok[sel[~conv]] = False
            bad[sel[isbad]] = True
        sweeps[run] += 1
        done[run] = ok[run]
    return int((~done).sum()), int(sweeps.max()) if ncl else 0


def solve_shake(con, x, im, s, b, tol, max_sweeps):
    """x (n, 3) is changed in place; returns (failed clusters, most sweeps of a cluster)"""
    ty = x.dtype.type
    d2, tol2 = con.d2.astype(x.dtype), ty(2.0 * tol)

    def one(q):
        i, j = con.pairs[q, 0], con.pairs[q, 1]
        p = b[q] + (x[j] - x[i])
        diff = d2[q] - (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])
        conv = np.abs(diff) <= tol2 * d2[q]
        sp = s[q, 0] * p[:, 0] + s[q, 1] * p[:, 1] + s[q, 2] * p[:, 2]
        isbad = ~conv & ~(sp > 0)
        u = ~conv & ~isbad
        g = diff[u] / (ty(2) * (im[i[u]] + im[j[u]]) * sp[u])
        x[i[u]] -= (g * im[i[u]])[:, None] * s[q[u]]
        x[j[u]] += (g * im[j[u]])[:, None] * s[q[u]]
        return conv, isbad
    return _sweeps(con, max_sweeps, one)


def solve_rattle(con, v, im, s, tol, dt, max_sweeps):
    ty = v.dtype.type
    d2, tol_dt = con.d2.astype(v.dtype), ty(tol / dt)

    def one(q):
        i, j = con.pairs[q, 0], con.pairs[q, 1]
        w = v[j] - v[i]
        dot = s[q, 0] * w[:, 0] + s[q, 1] * w[:, 1] + s[q, 2] * w[:, 2]
        conv = np.abs(dot) <= tol_dt * d2[q]
        u = ~conv
        k = dot[u] / ((s[q[u], 0] * s[q[u], 0] + s[q[u], 1] * s[q[u], 1] + s[q[u], 2] * s[q[u], 2]) * (im[i[u]] + im[j[u]]))
        v[i[u]] += (k * im[i[u]])[:, None] * s[q[u]]
        v[j[u]] -= (k * im[j[u]])[:, None] * s[q[u]]
        return conv, np.zeros(len(q), dtype=bool)
    return _sweeps(con, max_sweeps, one)


def step_restated(con, r, v, g, im, box, dt, T, gamma, seed, step, tol, max_sweeps):
    """first half of a step: (r, v, failed clusters, most sweeps)"""
    ty = r.dtype.type
    hda, hd = ty(0.5 * dt * ACC), ty(0.5 * dt)
    c1 = float(np.exp(-gamma * dt))
    v = v - hda * g * im[:, None]
    delta = hd * v
    if c1 < 1.0:
        sig = np.sqrt(ty((1.0 - c1 * c1) * KB * T * ACC) * im)[:, None]
        v = ty(c1) * v + sig * normals(len(im), seed, step % 2 ** 64, 0).astype(r.dtype)
    delta = delta + hd * v
    du = delta.copy()
    s = vectors(con, r, box)
    failed, most = solve_shake(con, delta, im, s, s, tol, max_sweeps)
    return r + delta, v + (delta - du) / ty(dt), failed, most


def kick_restated(con, r, v, g, im, box, dt, tol, max_sweeps):
    """second half of a step (g None: a pure projection): (v, failed clusters, most sweeps, sum m v^2 / 2 in float64)"""
    ty = r.dtype.type
    v = v.copy() if g is None else v - ty(0.5 * dt * ACC) * g * im[:, None]
    failed, most = solve_rattle(con, v, im, vectors(con, r, box), tol, dt, max_sweeps)
    return v, failed, most, float((0.5 * v.astype(np.float64) ** 2 / im.astype(np.float64)[:, None]).sum())


def project_restated(con, r, ref, im, box, tol, max_sweeps):
    delta = np.zeros_like(r)
    failed, most = solve_shake(con, delta, im, vectors(con, ref, box), vectors(con, r, box), tol, max_sweeps)
    return r + delta, failed, most


def con_bars(single, ref, is_double, tol, d_max, per_dt=None):
    """the bar rule of this module for one quantity: (bar, deviation of the float32 restatement from the float64 one)"""
    bar, dev = bars(single, ref, is_double)
    return bar + 4.0 * tol * d_max / (1.0 if per_dt is None else per_dt), dev


def constraint_errors(con, r, box):
    """| |s_ij| - d | / d per constraint, in float64"""
    s = vectors(con, np.asarray(r, dtype=np.float64), box)
    return np.abs(np.sqrt((s * s).sum(1)) - con.lengths) / con.lengths


# ---- the test system -------------------------------------------------------------------------------------------------------
def rigid_system(n_mol, n_free, seed, crossings=CROSSINGS, extras=True, shuffle=True):
    """water_system (tests/test_mts_plan_cpu.py) with the waters made rigid -- O-H, O-H and H-H at the lengths they have --, plus
    (extras) two 5-atom stars (a centre with four arms, 4 constraints) and a 6-atom chain (5 constraints), every atom wrapped
    into the cell and the whole atom order shuffled once more.  The velocities are projected onto the constraints with the
    float64 restatement.  Returns r, v, masses, Con, wrapped (of the waters, as water_system)."""
    r, v, mass, bonds, _, angles, _, wrapped = water_system(n_mol, n_free, seed, crossings, shuffle=shuffle)
    rng = np.random.default_rng(seed + 1000)
    pairs = [tuple(b) for b in bonds] + [(a[0], a[2]) for a in angles]
    pairs = [pairs[k] for m in range(n_mol) for k in (m, n_mol + m, 2 * n_mol + m)]      # a water's three side by side
    if extras:
        tet = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
        for frac, arm in (((0.21, 0.33, 0.47), 1.09), ((0.71, 0.58, 0.14), 1.33)):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            n0 = len(r)
            r = np.concatenate([r, np.array(frac) @ BOX + np.concatenate([np.zeros((1, 3)), arm * tet @ q.T])])
            mass = np.concatenate([mass, [12.011, 1.008, 1.008, 18.998, 35.45]])
            pairs += [(n0, n0 + k) for k in (3, 1, 4, 2)]                                # (not in the order of the atoms)
        n0 = len(r)
        zig = np.array([[1.25 * k, 0.45 * (k % 2), 0.1 * k] for k in range(6)])
        r = np.concatenate([r, np.array((0.45, 0.81, 0.66)) @ BOX + zig])
        mass = np.concatenate([mass, [12.011, 14.007, 12.011, 15.999, 12.011, 1.008]])
        pairs += [(n0 + k, n0 + k + 1) for k in (2, 0, 4, 1, 3)]
        n = len(r)
        vx = rng.normal(size=(n - len(v), 3)) * np.sqrt(ACC * KB * 300.0 / mass[len(v):])[:, None]
        v = np.concatenate([v, vx])
        inv = np.linalg.inv(BOX)
        s = r @ inv
        r = (s - np.floor(s)) @ BOX
        new = rng.permutation(n) if shuffle else np.arange(n)
        rs, vs, ms = np.empty_like(r), np.empty_like(v), np.empty_like(mass)
        rs[new], vs[new], ms[new] = r, v, mass
        r, v, mass = rs, vs, ms
        pairs = [(int(new[i]), int(new[j])) for i, j in pairs]
    pairs = np.array(pairs, dtype=int).reshape(-1, 2)
    d = min_image(r[pairs[:, 1]] - r[pairs[:, 0]], BOX)
    con = Con(len(r), pairs, np.sqrt((d * d).sum(1)))
    v = kick_restated(con, r, v, None, 1.0 / mass, BOX, 1.0, 1e-14, 500)[0]
    return r, v, mass, con, wrapped


# ---- the host program -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the headers cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('con_shim') / 'con_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I', CSRC, '-o', exe, SHIM])
    return exe


def lists_text(n_atoms, tile_atoms, pairs, lengths):
    rows = ['%d %d %d' % (n_atoms, tile_atoms, len(pairs))]
    rows += ['%d %d %.17g' % (p[0], p[1], d) for p, d in zip(pairs, lengths)]
    return '\n'.join(rows) + '\n'


def run_plan(shim, n_atoms, tile_atoms, pairs, lengths=None):
    """constraint k carries the length k + 0.5 unless told otherwise: the lengths must travel with their constraints"""
    lengths = [k + 0.5 for k in range(len(pairs))] if lengths is None else lengths
    out = subprocess.run([shim, 'plan'], input=lists_text(n_atoms, tile_atoms, pairs, lengths), capture_output=True, text=True,
                         check=True).stdout
    if out.startswith('error'):
        return out.strip()
    got = {}
    for line in out.strip().split('\n'):
        name, *vals = line.split()
        got[name] = np.array([float(x) for x in vals]) if name == 'con_d2' else np.array([int(x) for x in vals], dtype=int)
    return got


def check_plan(shim, n_atoms, tile_atoms, pairs):
    got, want = run_plan(shim, n_atoms, tile_atoms, pairs), plan_restated(n_atoms, pairs, tile_atoms)
    assert isinstance(got, dict), got
    s = got['scalars']
    assert list(s[:6]) == [n_atoms, tile_atoms, want['n_tiles'], want['n_clusters'], want['max_cluster'], len(pairs)]
    for name in ('tile_atom0', 'atom_id', 'tile_clu0', 'clu_atom0', 'clu_con0', 'con_slot', 'con_order'):
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got['con_d2'], np.array([(k + 0.5) ** 2 for k in want['con_order']]))
    sizes = np.diff(want['tile_atom0'])
    assert sizes.max() <= tile_atoms and sorted(got['atom_id']) == list(range(n_atoms))
    dims = [int(sizes.max()), int(np.diff(want['tile_clu0']).max()), int(np.diff(want['clu_con0'][want['tile_clu0']]).max())]
    assert list(s[6:9]) == dims
    a, c, q = dims
    assert s[9] == 8 * (4 * a + 4 * q) + 4 * (2 * q + c + 1) and s[10] == s[9] + 8 * 3 * q
    # within a cluster the caller's order is kept, a cluster's atoms ascend, and the slots name the constraint's atoms
    for c in range(want['n_clusters']):
        o = want['con_order'][want['clu_con0'][c]:want['clu_con0'][c + 1]]
        assert list(o) == sorted(o)
        atoms = want['atom_id'][want['clu_atom0'][c]:want['clu_atom0'][c + 1]]
        assert list(atoms) == sorted(atoms)
    for t in range(want['n_tiles']):
        a0 = want['tile_atom0'][t]
        for q in range(want['clu_con0'][want['tile_clu0'][t]], want['clu_con0'][want['tile_clu0'][t + 1]]):
            assert tuple(want['atom_id'][a0 + got['con_slot'][2 * q:2 * q + 2]]) == tuple(pairs[want['con_order'][q]])
    return want


def rigid_waters(n_mol, index=lambda m, k: 3 * m + k):
    return [(index(m, a), index(m, b)) for m in range(n_mol) for a, b in ((0, 1), (0, 2), (1, 2))]


STAR = [(0, 3), (0, 1), (0, 4), (0, 2)]
CHAIN = [(2, 3), (0, 1), (4, 5), (1, 2), (3, 4)]
TRIANGLE_TAIL = [(0, 1), (1, 2), (2, 0), (2, 3)]


def test_constants_match_the_python_side(shim):
    import ast
    out = subprocess.run([shim, 'consts'], capture_output=True, text=True, check=True).stdout.split()
    tree = ast.parse(open(ROOT + '/admp_amd/md.py').read())
    consts = {t.id: n.value.value for c in tree.body if isinstance(c, ast.ClassDef) and c.name == 'Constraints'
              for n in c.body if isinstance(n, ast.Assign) and isinstance(n.value, ast.Constant) for t in n.targets}
    assert int(out[0]) == consts['MAX_TILE_ATOMS'] and 1 <= int(out[1]) <= int(out[0])


@pytest.mark.parametrize('cap,tiles', [(3, 5), (4, 5), (7, 3), (15, 1)])
def test_five_waters(shim, cap, tiles):
    """a cluster is never split; with capacity 7 two waters share a tile"""
    want = check_plan(shim, 15, cap, rigid_waters(5))
    assert want['n_tiles'] == tiles and want['n_clusters'] == 5
    if cap == 7:
        assert list(np.diff(want['tile_atom0'])) == [6, 6, 3]


@pytest.mark.parametrize('pairs,n,size', [(STAR, 5, 5), (CHAIN, 6, 6), (TRIANGLE_TAIL, 4, 4)])
def test_star_chain_and_triangle_with_a_tail(shim, pairs, n, size):
    want = check_plan(shim, n + 2, size, pairs)      # two free atoms behind
    assert want['max_cluster'] == size and want['n_clusters'] == 3 and list(want['con_order']) == list(range(len(pairs)))
    assert isinstance(run_plan(shim, n + 2, size - 1, pairs), str)


def test_free_atoms_only_and_between_molecules(shim):
    want = check_plan(shim, 5, 2, [])
    assert want['n_tiles'] == 3 and want['n_clusters'] == 5 and len(want['con_slot']) == 0
    idx = lambda m, k: (1, 2, 3, 6, 7, 8)[3 * m + k]      # noqa: E731  atoms 0, 4, 5, 9 are free
    want = check_plan(shim, 10, 4, rigid_waters(2, idx))
    assert list(want['atom_id']) == list(range(10)) and list(np.diff(want['tile_atom0'])) == [4, 2, 4]
    assert check_plan(shim, 1, 64, [])['n_tiles'] == 1


def test_shuffled_atom_order(shim):
    """molecule m owns atoms m, 4 + m, 8 + m: packing follows the smallest atom, slots ascend within a molecule"""
    want = check_plan(shim, 12, 6, rigid_waters(4, lambda m, k: 4 * k + m))
    assert list(want['atom_id'][:6]) == [0, 4, 8, 1, 5, 9]
    perm = np.random.default_rng(2).permutation(17)
    pairs = [(int(perm[i]), int(perm[j])) for i, j in rigid_waters(2) + [(6 + i, 6 + j) for i, j in STAR] + [(11 + i, 11 + j) for i, j in CHAIN]]
    want = check_plan(shim, 17, 8, pairs)
    assert want['max_cluster'] == 6 and want['n_clusters'] == 4


def test_interleaved_caller_order(shim):
    """the constraints of two waters and a chain given alternately: each cluster's constraints are gathered, in the caller's order"""
    a, b, c = rigid_waters(2)[:3], rigid_waters(2)[3:], [(6 + i, 6 + j) for i, j in CHAIN]
    pairs = [c[0], a[0], b[0], c[1], a[1], c[2], b[1], b[2], c[3], a[2], c[4]]
    want = check_plan(shim, 12, 12, pairs)
    assert list(want['con_order']) == [1, 4, 9, 2, 6, 7, 0, 3, 5, 8, 10] and list(want['clu_con0']) == [0, 3, 6, 11]


def test_duplicates_are_kept(shim):
    pairs = [(3, 4), (0, 1), (1, 0), (0, 1), (4, 5), (0, 2)]
    want = check_plan(shim, 6, 3, pairs)
    assert want['n_tiles'] == 2 and list(want['clu_con0']) == [0, 4, 6] and list(want['con_order']) == [1, 2, 3, 5, 0, 4]


def test_refusals_of_the_plan(shim):
    chain = [(0, 1), (1, 2), (2, 3)]
    msg = run_plan(shim, 6, 3, chain)
    assert isinstance(msg, str) and 'a cluster of 4 atoms' in msg and 'smallest atom 0' in msg and 'tile_atoms 3' in msg
    assert plan_restated(6, chain, 3) == (4, 0)
    msg = run_plan(shim, 9, 3, [(6, 7)] + [(5, 2), (2, 8), (8, 4)])
    assert 'a cluster of 4 atoms' in msg and 'smallest atom 2' in msg
    consts = subprocess.run([shim, 'consts'], capture_output=True, text=True, check=True).stdout.split()
    for cap in (0, int(consts[0]) + 1):
        msg = run_plan(shim, 6, cap, chain)
        assert isinstance(msg, str) and 'tile_atoms %d outside 1..%s' % (cap, consts[0]) in msg
    assert isinstance(run_plan(shim, 6, int(consts[0]), chain), dict)
    for bad in ((0, 3), (-1, 2)):
        msg = run_plan(shim, 3, 3, [(0, 1), bad])
        assert 'constraint 1 (%d, %d)' % bad in msg and 'out of range' in msg
    msg = run_plan(shim, 3, 3, [(0, 1), (1, 2), (2, 2)])
    assert 'constraint 2 (2, 2)' in msg and 'itself' in msg
    for length in (0.0, -1.0, float('inf'), float('nan')):
        msg = run_plan(shim, 3, 3, [(0, 1), (1, 2)], [1.0, length])
        assert isinstance(msg, str) and 'constraint 1 (1, 2)' in msg and 'positive and finite' in msg, length
    # LDS: 250 atoms in one cluster with 1200 constraints (duplicates) need 8 (4 x 250 + 7 x 1200) + 4 (2400 + 2) > 64 KiB
    many = [(k, k + 1) for k in range(249)] + [(0, 1)] * 951
    msg = run_plan(shim, 250, 256, many, [1.0] * len(many))
    assert isinstance(msg, str) and '84808 bytes of LDS' in msg and 'limit 65536' in msg
    assert isinstance(run_plan(shim, 250, 256, many[:880], [1.0] * 880), dict)      # 64 328 bytes


# ---- the three runs --------------------------------------------------------------------------------------------------------
PAR = dict(dt=2.0, T=300.0, gamma=0.05, seed=11, step=3)
TOL = {'d': 1e-12, 'f': 1e-6}


@pytest.fixture(scope='module')
def run_case():
    """8 rigid waters, two of them wrapped across faces, a star, a star and a chain (40 atoms), shuffled; 300 K, a random
    gradient"""
    r, v, mass, con, wrapped = rigid_system(8, 0, 5, [((0, 0),), ((2, 1),)])
    assert sum(1 for w in wrapped if w) >= 2 and len(r) == 40 and len(con.pairs) == 24 + 8 + 5
    g = np.random.default_rng(6).normal(size=r.shape) * 30.0
    pert = r + np.random.default_rng(7).uniform(-0.05, 0.05, size=r.shape)
    return r, v, g, mass, con, pert


def run_shim(shim, op, prec, cap, con, a, b, c, im, hda, dt, c1, c2sq, seed, step, tol, max_sweeps, with_grad):
    n = len(a)
    text = lists_text(n, cap, con.pairs, con.lengths) + ' '.join('%.17g' % x for x in BOX.ravel()) + '\n'
    text += '%.17g %.17g %.17g %.17g %d %d %.17g %d %d\n' % (hda, dt, c1, c2sq, seed, step, tol, max_sweeps, with_grad)
    text += '\n'.join(' '.join('%.17g' % x for x in list(a[i]) + list(b[i]) + list(c[i]) + [im[i]]) for i in range(n)) + '\n'
    out = subprocess.run([shim, op, prec], input=text, capture_output=True, text=True, check=True).stdout
    vals = np.array(out.split(), dtype=np.float64)
    assert len(vals) == 6 * n + 3, out[:200]
    return vals[:3 * n].reshape(n, 3), vals[3 * n:6 * n].reshape(n, 3), int(vals[-3]), int(vals[-2]), vals[-1]


def both(fn, tol, *arrays):
    """fn(tol, arrays) on float64 and on float32 copies of the arrays; the float32 run, which is only the yardstick of the bar,
    with a tolerance that float32 can meet"""
    return fn(tol, *arrays), fn(max(tol, 1e-6), *[None if a is None else a.astype(np.float32) for a in arrays])


def report(what, name, got, ref, single, is_double, tol, d_max, per_dt=None):
    bar, dev = con_bars(single, ref, is_double, tol, d_max, per_dt)
    d = np.abs(got - ref).max()
    print('%s: |d%s| %.3e, bar %.3e (float32 restatement %.3e): share %.4f' % (what, name, d, bar, dev, d / bar))
    assert d <= bar, (what, name)


@pytest.mark.parametrize('prec', ['d', 'f'])
@pytest.mark.parametrize('cap', [6, 7, 64])
def test_step_kick_and_project_against_the_restatement(shim, run_case, prec, cap):
    r, v, g, mass, con, pert = run_case
    im, tol, dm = 1.0 / mass, TOL[prec], con.lengths.max()
    dt, c1 = PAR['dt'], np.exp(-PAR['gamma'] * PAR['dt'])
    hda, c2sq = 0.5 * dt * ACC, (1.0 - c1 * c1) * KB * PAR['T'] * ACC
    what = '%s cap %d' % (prec, cap)
    # first half
    ref, single = both(lambda t, r, v, g, im: step_restated(con, r, v, g, im, BOX, tol=t, max_sweeps=500, **PAR), tol, r, v, g, im)
    gr, gv, failed, most, _ = run_shim(shim, 'step', prec, cap, con, r, v, g, im, hda, dt, c1, c2sq, PAR['seed'], PAR['step'], tol, 500, 1)
    report(what + ' step', 'r', gr, ref[0], single[0], prec == 'd', tol, dm)
    report(what + ' step', 'v', gv, ref[1], single[1], prec == 'd', tol, dm, dt)
    same = ref if prec == 'd' else single      # the restatement in the program's precision: its sweep counts
    assert failed == 0 == same[2] and abs(most - same[3]) <= 1 and most > 1
    eps = 2.0 ** -52 if prec == 'd' else 2.0 ** -23
    assert constraint_errors(con, gr, BOX).max() <= tol + 4 * eps * np.abs(gr).max() / con.lengths.min()
    # second half, from the restatement's positions
    r1, v1 = ref[0], ref[1]
    kref, ksingle = both(lambda t, r, v, g, im: kick_restated(con, r, v, g, im, BOX, dt, t, 500), tol, r1, v1, g, im)
    _, kv, failed, most, ekin = run_shim(shim, 'kick', prec, cap, con, r1, v1, g, im, hda, dt, 1.0, 0.0, 0, 0, tol, 500, 1)
    report(what + ' kick', 'v', kv, kref[0], ksingle[0], prec == 'd', tol, dm, dt)
    ksame = kref if prec == 'd' else ksingle
    assert failed == 0 and abs(most - ksame[2]) <= 1 and abs(ekin - kref[3]) <= 1e-4 * kref[3]
    # a pure velocity projection and a position projection, along the directions of the start configuration and of itself
    pref, psingle = both(lambda t, r, v, im: kick_restated(con, r, v, None, im, BOX, 1.0, t, 500), tol, r1, v1 + 1e-3 * g * im[:, None], im)
    _, pv, failed, _, _ = run_shim(shim, 'kick', prec, cap, con, r1, v1 + 1e-3 * g * im[:, None], g, im, 0.0, 1.0, 1.0, 0.0, 0, 0, tol, 500, 0)
    report(what + ' velocity projection', 'v', pv, pref[0], psingle[0], prec == 'd', tol, dm, 1.0)
    assert failed == 0
    for name, along in (('itself', pert), ('start', r)):
        pref, psingle = both(lambda t, p, a, im: project_restated(con, p, a, im, BOX, t, 500), tol, pert, along, im)
        pr, _, failed, most, _ = run_shim(shim, 'project', prec, cap, con, pert, along, g, im, 0.0, 1.0, 1.0, 0.0, 0, 0, tol, 500, 0)
        report(what + ' projection along ' + name, 'r', pr, pref[0], psingle[0], prec == 'd', tol, dm)
        psame = pref if prec == 'd' else psingle
        assert failed == 0 == psame[1] and abs(most - psame[2]) <= 1
        assert constraint_errors(con, pr, BOX).max() <= tol + 4 * eps * np.abs(pr).max() / con.lengths.min()
        assert constraint_errors(con, pert, BOX).max() > 1e-2


@pytest.mark.parametrize('prec', ['d', 'f'])
def test_one_sweep_counts_the_unconverged_clusters(shim, run_case, prec):
    """max_sweeps = 1 on the perturbed configuration: every cluster with a constraint stops unconverged, the free ones do not
    count, and the outputs are finite; a useless reference direction (s.p <= 0) counts too and leaves the cluster alone"""
    r, v, g, mass, con, pert = run_case
    im = 1.0 / mass
    want = project_restated(con, pert, pert, im, BOX, TOL[prec], 1)
    pr, _, failed, most, _ = run_shim(shim, 'project', prec, 64, con, pert, pert, g, im, 0.0, 1.0, 1.0, 0.0, 0, 0, TOL[prec], 1, 0)
    assert failed == want[1] == len(con.sweep) == 11 and most == 1 and np.isfinite(pr).all()
    two = Con(2, [(0, 1)], [1.0])
    a, b = np.array([[0.0, 0, 0], [1.25, 0, 0]]), np.array([[0.0, 0, 0], [-1.0, 0, 0]])
    pr, _, failed, most, _ = run_shim(shim, 'project', prec, 64, two, a, b, a, np.ones(2), 0.0, 1.0, 1.0, 0.0, 0, 0, TOL[prec], 50, 0)
    assert failed == 1 == project_restated(two, a, b, np.ones(2), BOX, TOL[prec], 50)[1] and most == 1 and np.array_equal(pr, a)
