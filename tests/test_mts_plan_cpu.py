"""The multiple-time-step integrator without a GPU: the host plan (admp_amd/csrc/mts_plan.h) against a Python restatement
(union-find plus the packing rule), array for array, and the per-tile loop run serially by a stand-alone host program
(tests/mts_shim/main.cpp) with the arithmetic the kernel compiles (md_bonded_math.h, md_math.h) against a float64 numpy
restatement of the scheme.  tests/test_gpu_md_mts.py imports the restatements, the system builder and the bar rule.

Bar rule: the reference is the float64 restatement; a single-precision run may deviate by 16 x what the SAME restatement run
in float32 deviates from it (operation order and two libm's differ; a wrong inner step is off by 1e3 or more), a
double-precision run by that figure x 2^-29 (the ratio of the two machine epsilons).  A few-eps bar would be wrong: a position
rounding of eps L reaches the velocities through k_bond delta 1e-4 / m."""
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_md_random_cpu import CSRC, ROOT, normals

SHIM = ROOT + '/tests/mts_shim/main.cpp'
KB = 0.0083144626
ACC = 1e-4
MASS = (15.999, 1.008, 1.008)
K_BOND, R0, K_ANG, TH0 = 3765.6, 0.9572, 460.24, 1.82421813418
BOX = np.array([[12.4, 0.0, 0.0], [0.9, 12.1, 0.0], [-0.6, 0.7, 12.7]])
REF_PLUS, REF_MINUS, REF_CENTRE = 0, 1, 2


# ---- restatement of the plan ---------------------------------------------------------------------------------------------
def plan_restated(n_atoms, bonds, angles, tile_atoms):
    """dict of the plan's arrays, or the (size, smallest atom) of the first component that does not fit"""
    parent = list(range(n_atoms))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def join(a, b):
        a, b = find(a), find(b)
        parent[max(a, b)] = min(a, b)
    for i, j in bonds:
        join(i, j)
    for i, j, k in angles:
        join(i, j)
        join(j, k)
    comps = {}
    for i in range(n_atoms):
        comps.setdefault(find(i), []).append(i)
    tiles = []
    for root in sorted(comps):
        c = comps[root]
        if len(c) > tile_atoms:
            return len(c), root
        if not tiles or sum(map(len, tiles[-1])) + len(c) > tile_atoms:
            tiles.append([])
        tiles[-1].append(c)
    atom_id = [a for t in tiles for c in t for a in c]
    tile_atom0 = np.concatenate([[0], np.cumsum([sum(map(len, t)) for t in tiles])])
    tile_of, local = {}, {}
    for t, tl in enumerate(tiles):
        for s, a in enumerate(a for c in tl for a in c):
            tile_of[a], local[a] = t, s
    out = dict(tile_atom0=tile_atom0, atom_id=np.array(atom_id), n_tiles=len(tiles), max_component=max(map(len, comps.values())))
    refs = [[] for _ in range(n_atoms)]                     # by atom: bonds in the caller's order, then angles
    per_tile_b = [[k for k, b in enumerate(bonds) if tile_of[b[0]] == t] for t in range(len(tiles))]
    per_tile_a = [[k for k, a in enumerate(angles) if tile_of[a[0]] == t] for t in range(len(tiles))]
    for t in range(len(tiles)):
        for s, k in enumerate(per_tile_b[t]):
            refs[bonds[k][0]].append(4 * s + REF_MINUS)
            refs[bonds[k][1]].append(4 * s + REF_PLUS)
    for t in range(len(tiles)):
        for q, k in enumerate(per_tile_a[t]):
            s = len(per_tile_b[t]) + 2 * q
            refs[angles[k][0]].append(4 * s + REF_PLUS)
            refs[angles[k][1]].append(4 * s + REF_CENTRE)
            refs[angles[k][2]].append(4 * (s + 1) + REF_PLUS)
    out['tile_bond0'] = np.concatenate([[0], np.cumsum([len(x) for x in per_tile_b])])
    out['tile_angle0'] = np.concatenate([[0], np.cumsum([len(x) for x in per_tile_a])])
    out['bond_order'] = [k for x in per_tile_b for k in x]
    out['angle_order'] = [k for x in per_tile_a for k in x]
    out['bond_slot'] = np.array([local[a] for k in out['bond_order'] for a in bonds[k]], dtype=int)
    out['angle_slot'] = np.array([local[a] for k in out['angle_order'] for a in angles[k]], dtype=int)
    out['ref0'] = np.concatenate([[0], np.cumsum([len(refs[a]) for a in atom_id])])
    out['ref'] = np.array([x for a in atom_id for x in refs[a]], dtype=int)
    return out


# ---- restatement of the scheme (dtype of r throughout; float64 is the reference) ----------------------------------------
def bonded_restated(r, box, bonds, bpar, angles, apar):
    """(gradient, E_bonds, E_angles) with minimum-image vectors; energies summed in float64"""
    ty = r.dtype
    h, hinv = box.astype(ty), np.linalg.inv(box).astype(ty)

    def mi(d):
        s = d @ hinv
        return (s - np.floor(s + ty.type(0.5))) @ h
    g = np.zeros_like(r)
    eb = ea = 0.0
    if len(bonds):
        i, j = bonds[:, 0], bonds[:, 1]
        d = mi(r[j] - r[i])
        rr = np.sqrt((d * d).sum(1))
        k, dr = bpar[:, 0].astype(ty), rr - bpar[:, 1].astype(ty)
        s = (k * dr / rr)[:, None] * d
        np.add.at(g, j, s)
        np.add.at(g, i, -s)
        eb = float((0.5 * k.astype(np.float64) * dr.astype(np.float64) ** 2).sum())
    if len(angles):
        i, j, k3 = angles[:, 0], angles[:, 1], angles[:, 2]
        u, v = mi(r[i] - r[j]), mi(r[k3] - r[j])
        ru, rv = np.sqrt((u * u).sum(1)), np.sqrt((v * v).sum(1))
        c = np.clip((u * v).sum(1) / (ru * rv), -1.0, 1.0).astype(ty)
        th = np.arccos(c.astype(np.float64)).astype(ty)
        kt, dth = apar[:, 0].astype(ty), th - apar[:, 1].astype(ty)
        sn = np.maximum(np.sqrt(1 - c * c), ty.type(1e-8))
        f = (-kt * dth / sn)[:, None]
        gu = f * (v / (ru * rv)[:, None] - c[:, None] * u / (ru * ru)[:, None])
        gv = f * (u / (ru * rv)[:, None] - c[:, None] * v / (rv * rv)[:, None])
        np.add.at(g, i, gu)
        np.add.at(g, k3, gv)
        np.add.at(g, j, -(gu + gv))
        ea = float((0.5 * kt.astype(np.float64) * dth.astype(np.float64) ** 2).sum())
    return g, eb, ea


def kick_drift_restated(r, v, gs, im, box, lists, dt_outer, n, T, gamma, seed, s):
    """everything above the calculators of one outer step: (r, v, bonded gradient at r, E_bonds, E_angles)"""
    ty = r.dtype.type
    delta = dt_outer / n
    hdo, hdi, hd = ty(0.5 * dt_outer * ACC), ty(0.5 * dt_outer * ACC / n), ty(0.5 * delta)
    c1 = float(np.exp(-gamma * delta))
    sig = np.sqrt(ty((1.0 - c1 * c1) * KB * T * ACC) * im)[:, None]
    v = v - hdo * gs * im[:, None]
    f, eb, ea = bonded_restated(r, box, *lists)
    for k in range(n):
        v = v - hdi * f * im[:, None]
        r = r + hd * v
        if c1 < 1.0:
            v = ty(c1) * v + sig * normals(len(im), seed, (s * n + k) % 2 ** 64, 0).astype(r.dtype)
        r = r + hd * v
        f, eb, ea = bonded_restated(r, box, *lists)
        v = v - hdi * f * im[:, None]
    return r, v, f, eb, ea


def bars(single, ref, is_double):
    """the bar rule for one quantity: (bar, deviation of the float32 restatement from the float64 one)"""
    dev = float(np.abs(single.astype(np.float64) - ref).max())
    return 16.0 * dev * (2.0 ** -29 if is_double else 1.0), dev


# ---- the test system -------------------------------------------------------------------------------------------------------
def water_system(n_mol, n_free, seed, crossings, shuffle=True, temperature=300.0):
    """n_mol flexible waters on a grid in BOX plus n_free free atoms, every atom wrapped into the cell.  crossings: one tuple of
    (axis, side) pairs per forced molecule -- its oxygen sits 0.04 A inside those faces and it is turned until an atom lies
    beyond each of them, so the wrapped molecule spans the faces (three pairs: a corner).  Returns r, v, masses, bonds, bpar,
    angles, apar, wrapped (per molecule: the set of axes its atoms were wrapped differently on)."""
    rng = np.random.default_rng(seed)
    inv = np.linalg.inv(BOX)
    g = int(np.ceil(n_mol ** (1.0 / 3.0)))
    sites = [((i + 0.5) / g, (j + 0.5) / g, (k + 0.5) / g) for i in range(g) for j in range(g) for k in range(g)][:n_mol]
    local = np.array([[0.0, 0.0, 0.0], [np.sin(TH0 / 2), np.cos(TH0 / 2), 0.0], [-np.sin(TH0 / 2), np.cos(TH0 / 2), 0.0]])
    mols, wrapped = [], []
    for m in range(n_mol):
        frac = np.array(sites[m])
        want = crossings[m] if m < len(crossings) else ()
        for axis, side in want:
            frac[axis] = 0.003 if side == 0 else 0.997
        while True:
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            x = (local * (R0 * (1.0 + 0.03 * rng.normal(size=(3, 1))))) @ q.T + frac @ BOX
            cells = np.floor(x @ inv)
            if all(len(set(cells[:, axis])) > 1 for axis, _ in want):
                break
        mols.append(x)
        wrapped.append({a for a in range(3) if len(set(cells[:, a])) > 1})
    r = np.concatenate(mols + [rng.uniform(0.0, 1.0, size=(n_free, 3)) @ BOX])
    s = r @ inv
    r = (s - np.floor(s)) @ BOX
    mass = np.concatenate([np.tile(MASS, n_mol), np.full(n_free, 39.948)])
    o = 3 * np.arange(n_mol)
    bonds = np.stack([np.concatenate([o, o]), np.concatenate([o + 1, o + 2])], axis=1)
    angles = np.stack([o + 1, o, o + 2], axis=1)
    n = len(r)
    new = rng.permutation(n) if shuffle else np.arange(n)      # new[old] = the atom's index after the shuffle
    rs, ms = np.empty_like(r), np.empty_like(mass)
    rs[new], ms[new] = r, mass
    v = rng.normal(size=(n, 3)) * np.sqrt(ACC * KB * temperature / ms)[:, None]
    return (rs, v, ms, new[bonds], np.tile([K_BOND, R0], (2 * n_mol, 1)), new[angles], np.tile([K_ANG, TH0], (n_mol, 1)), wrapped)


# ---- the host program -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the headers cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('mts_shim') / 'mts_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I', CSRC, '-o', exe, SHIM])
    return exe


def lists_text(n_atoms, tile_atoms, bonds, bpar, angles, apar):
    rows = ['%d %d %d %d' % (n_atoms, tile_atoms, len(bonds), len(angles))]
    rows += ['%d %d %.17g %.17g' % (b[0], b[1], p[0], p[1]) for b, p in zip(bonds, bpar)]
    rows += ['%d %d %d %.17g %.17g' % (a[0], a[1], a[2], p[0], p[1]) for a, p in zip(angles, apar)]
    return '\n'.join(rows) + '\n'


def run_plan(shim, n_atoms, tile_atoms, bonds, angles):
    """bond k carries the parameters (k + 0.5, -k), angle k (k + 0.25, k): the parameters must travel with their items"""
    bpar = [(k + 0.5, -float(k)) for k in range(len(bonds))]
    apar = [(k + 0.25, float(k)) for k in range(len(angles))]
    out = subprocess.run([shim, 'plan'], input=lists_text(n_atoms, tile_atoms, bonds, bpar, angles, apar), capture_output=True,
                         text=True, check=True).stdout
    if out.startswith('error'):
        return out.strip()
    got = {}
    for line in out.strip().split('\n'):
        name, *vals = line.split()
        got[name] = np.array([float(x) for x in vals]) if name.endswith('par') else np.array([int(x) for x in vals], dtype=int)
    return got


def check_plan(shim, n_atoms, tile_atoms, bonds, angles):
    got, want = run_plan(shim, n_atoms, tile_atoms, bonds, angles), plan_restated(n_atoms, bonds, angles, tile_atoms)
    assert isinstance(got, dict), got
    s = got['scalars']
    assert list(s[:6]) == [n_atoms, tile_atoms, want['n_tiles'], want['max_component'], len(bonds), len(angles)]
    for name in ('tile_atom0', 'atom_id', 'tile_bond0', 'bond_slot', 'tile_angle0', 'angle_slot', 'ref0', 'ref'):
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got['bond_par'], np.array([(k + 0.5, -float(k)) for k in want['bond_order']]).ravel())
    assert np.array_equal(got['angle_par'], np.array([(k + 0.25, float(k)) for k in want['angle_order']]).ravel())
    sizes = np.diff(want['tile_atom0'])
    assert sizes.max() <= tile_atoms and sorted(got['atom_id']) == list(range(n_atoms))
    per_tile = lambda first: int(np.diff(first).max())      # noqa: E731
    dims = [int(sizes.max()), per_tile(want['tile_bond0']), per_tile(want['tile_angle0']), per_tile(want['ref0'][want['tile_atom0']])]
    assert list(s[6:10]) == dims
    a, b, g, nr = dims
    assert s[10] == 8 * (3 * a + 3 * (b + 2 * g) + 2 * b + 2 * g) + 4 * (2 * b + 3 * g + a + 1 + nr)
    return want


def waters(n_mol, index=lambda m, k: 3 * m + k):
    bonds = [(index(m, 0), index(m, h)) for h in (1, 2) for m in range(n_mol)]
    angles = [(index(m, 1), index(m, 0), index(m, 2)) for m in range(n_mol)]
    return bonds, angles


def test_constants_match_the_python_side(shim):
    import ast
    out = subprocess.run([shim, 'consts'], capture_output=True, text=True, check=True).stdout.split()
    tree = ast.parse(open(ROOT + '/admp_amd/md.py').read())
    consts = {t.id: n.value.value for c in tree.body if isinstance(c, ast.ClassDef) and c.name == 'MTSLangevin'
              for n in c.body if isinstance(n, ast.Assign) and isinstance(n.value, ast.Constant) for t in n.targets}
    assert int(out[0]) == consts['MAX_TILE_ATOMS'] and 1 <= int(out[1]) <= int(out[0])


def test_one_atom_without_items(shim):
    want = check_plan(shim, 1, 64, [], [])
    assert want['n_tiles'] == 1


@pytest.mark.parametrize('cap,tiles', [(3, 5), (4, 5), (7, 3), (15, 1)])
def test_five_waters(shim, cap, tiles):
    """a molecule is never split; with capacity 7 two waters share a tile"""
    want = check_plan(shim, 15, cap, *waters(5))
    assert want['n_tiles'] == tiles
    if cap == 7:
        assert list(np.diff(want['tile_atom0'])) == [6, 6, 3]


def test_scattered_indices(shim):
    """molecule m owns atoms m, 4 + m, 8 + m: packing follows the smallest atom, slots ascend within a molecule"""
    want = check_plan(shim, 12, 6, *waters(4, lambda m, k: 4 * k + m))
    assert list(want['atom_id'][:6]) == [0, 4, 8, 1, 5, 9]


def test_free_atoms_between_molecules(shim):
    idx = lambda m, k: (1, 2, 3, 6, 7, 8)[3 * m + k]      # noqa: E731  atoms 0, 4, 5, 9 are free
    want = check_plan(shim, 10, 4, *waters(2, idx))
    assert list(want['atom_id']) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9] and list(np.diff(want['tile_atom0'])) == [4, 2, 4]


def test_component_held_by_an_angle_alone(shim):
    want = check_plan(shim, 6, 3, [], [(4, 0, 2)])
    assert want['max_component'] == 3 and list(want['atom_id'][:3]) == [0, 2, 4]


def test_duplicate_bonds_and_any_order(shim):
    bonds = [(3, 4), (0, 1), (1, 0), (0, 1), (4, 5), (0, 2)]
    want = check_plan(shim, 6, 3, bonds, [(5, 4, 3), (1, 0, 2)])
    assert want['n_tiles'] == 2 and len(want['ref']) == 2 * 6 + 3 * 2


def test_refusals_of_the_plan(shim):
    chain = [(0, 1), (1, 2), (2, 3)]
    msg = run_plan(shim, 6, 3, chain, [])
    assert isinstance(msg, str) and '4 atoms' in msg and 'smallest atom 0' in msg
    assert plan_restated(6, chain, [], 3) == (4, 0)
    consts = subprocess.run([shim, 'consts'], capture_output=True, text=True, check=True).stdout.split()
    for cap in (0, int(consts[0]) + 1):
        msg = run_plan(shim, 6, cap, chain, [])
        assert isinstance(msg, str) and 'tile_atoms' in msg
    assert isinstance(run_plan(shim, 6, int(consts[0]), chain, []), dict)
    assert 'out of range' in run_plan(shim, 3, 3, [(0, 3)], [])


# ---- step mode ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def step_case():
    """8 waters, two of them wrapped across faces, 300 K, a random slow gradient; n = 4, gamma = 0.05 / fs, outer step 3"""
    r, v, mass, bonds, bpar, angles, apar, wrapped = water_system(8, 0, 5, [((0, 0),), ((2, 1),)])
    assert sum(1 for w in wrapped if w) >= 2
    gs = np.random.default_rng(6).normal(size=r.shape) * 30.0
    par = dict(dt_outer=2.0, n=4, T=300.0, gamma=0.05, seed=11, s=3)
    lists = (bonds, bpar, angles, apar)
    ref = kick_drift_restated(r, v, gs, 1.0 / mass, BOX, lists, **par)
    f32 = lambda a: a.astype(np.float32)      # noqa: E731
    single = kick_drift_restated(f32(r), f32(v), f32(gs), f32(1.0 / mass), BOX, lists, **par)
    return r, v, gs, mass, lists, par, ref, single


@pytest.mark.parametrize('prec', ['d', 'f'])
@pytest.mark.parametrize('cap', [3, 7, 64])
def test_step_against_the_restatement(shim, step_case, prec, cap):
    r, v, gs, mass, lists, par, ref, single = step_case
    n = len(r)
    c1 = np.exp(-par['gamma'] * par['dt_outer'] / par['n'])
    text = lists_text(n, cap, *lists) + ' '.join('%.17g' % x for x in BOX.ravel()) + '\n'
    text += '%d %.17g %.17g %.17g %.17g %d %d\n' % (par['n'], 0.5 * par['dt_outer'] * ACC, par['dt_outer'], c1,
                                                  (1.0 - c1 * c1) * KB * par['T'] * ACC, par['seed'], par['s'])
    text += '\n'.join(' '.join('%.17g' % x for x in list(r[i]) + list(v[i]) + list(gs[i]) + [1.0 / mass[i]]) for i in range(n)) + '\n'
    out = subprocess.run([shim, 'step', prec], input=text, capture_output=True, text=True, check=True).stdout
    vals = np.array(out.split(), dtype=np.float64)
    assert len(vals) == 9 * n + 2
    got = vals[:9 * n].reshape(3, n, 3)
    for name, q in (('r', 0), ('v', 1), ('f', 2)):
        bar, dev = bars(single[q], ref[q], prec == 'd')
        d = np.abs(got[q] - ref[q]).max()
        print('%s %s cap %d: |d%s| %.3e, bar %.3e (float32 restatement %.3e): ratio %.3f' % (prec, name, cap, name, d, bar, dev, d / bar))
        assert d <= bar, name
    # the energy words are those of the last evaluation: summed in double from rounded lengths and angles, 64 eps relative
    # to the sum of the terms' magnitudes is the chain dr -> dr^2 -> sum with room to spare
    eps = 2.0 ** -52 if prec == 'd' else 2.0 ** -23
    dr_rel = 64 * eps * max(R0, TH0) / 0.03      # a term k/2 x^2 with x = r - r0 (about 0.03 r0 here) carries the rounding of r
    assert abs(vals[-2] - ref[3]) <= dr_rel * ref[3] and abs(vals[-1] - ref[4]) <= dr_rel * max(ref[4], ref[3])
