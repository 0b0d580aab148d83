"""The molecular (centre-of-mass) cell scaling without a GPU: the host plan (admp_amd/csrc/mol_plan.h) against a Python
restatement, array for array, and the per-tile loops of the two kernels run serially by a stand-alone host program
(tests/mol_shim/main.cpp) with the arithmetic the kernels compile (md_mol_math.h) against a float64 numpy restatement of the
formulas.  tests/test_gpu_md_molecular_barostat.py imports the restatements and the bar rules.

Definitions restated (`mol_restated`): the anchor a of a group is its lowest-numbered atom; d_i = min_image(r_i - r_a), s_i =
(r_i - r_a) - d_i; R_c = r_a + sum m_i d_i / M, V_c = sum m_i v_i / M, R_c(i) = R_c + s_i.  Sums: kin = sum_c M_c V_c (x) V_c,
rg = sum_i R_c(i) (x) g_i.  One application: r_i += (mu - 1) R_c(i), v_i += (1/mu - 1) V_c.

Bars.  Sums: 64 eps_f64 sum|terms| per word (the bar of the atomic sums test); in single precision the image arithmetic runs
in float32, so the restatement takes the rounded inputs and forms d and s in float32 too, and the bar adds 16 x its deviation
from the same restatement with d and s in float64 (the rule of tests/test_mts_plan_cpu.py `bars`).  One application: 4 eps
max|r| and 4 eps max|v| (one rounded product, one sum)."""
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_con_plan_cpu import clusters_of, rigid_system
from tests.test_md_random_cpu import CSRC, ROOT
from tests.test_mts_plan_cpu import BOX

SHIM = ROOT + '/tests/mol_shim/main.cpp'
E64 = 2.0 ** -52


# ---- restatement of the plan ---------------------------------------------------------------------------------------------
def plan_restated(labels, tile_atoms):
    """dict of the plan's arrays, or the (size, smallest atom) of the first group that does not fit"""
    groups = {}
    for i, g in enumerate(labels):
        groups.setdefault(int(g), []).append(i)
    ordered = sorted(groups.values(), key=lambda c: c[0])
    tiles = []
    for c in ordered:
        if len(c) > tile_atoms:
            return len(c), c[0]
        if not tiles or sum(map(len, tiles[-1])) + len(c) > tile_atoms:
            tiles.append([])
        tiles[-1].append(c)
    return dict(n_tiles=len(tiles), n_groups=len(ordered), max_group=max(map(len, ordered)),
                tile_atom0=np.concatenate([[0], np.cumsum([sum(map(len, t)) for t in tiles])]),
                atom_id=np.array([a for c in ordered for a in c]),
                tile_grp0=np.concatenate([[0], np.cumsum([len(t) for t in tiles])]),
                grp_atom0=np.concatenate([[0], np.cumsum([len(c) for c in ordered])]),
                slot_grp=np.array([k for t in tiles for k, c in enumerate(t) for _ in c]))


def labels_of(n_atoms, pairs):
    """label = smallest atom of the connected component (what admp_amd.md.groups_of returns)"""
    lab = np.empty(n_atoms, dtype=np.int32)
    for root, atoms in clusters_of(n_atoms, pairs).items():
        lab[atoms] = root
    return lab


# ---- restatement of the formulas -------------------------------------------------------------------------------------------
def mol_restated(r, v, im, labels, box, image_dtype=np.float64):
    """per atom, in float64 from the arrays as given: Rc (n, 3) = R_c(i), Vc (n, 3), M (n), anchor (n), s (n, 3), d (n, 3).  The
    image arithmetic (d, s) runs in image_dtype, as on a handle of that precision; the sums run in float64 in atom order."""
    ty = np.dtype(image_dtype)
    labels = np.asarray(labels)
    n = len(labels)
    first = {}
    for i, g in enumerate(labels):
        first.setdefault(int(g), i)
    anchor = np.array([first[int(g)] for g in labels])
    rt = r.astype(ty)
    h, hinv = box.astype(ty), np.linalg.inv(box).astype(ty)
    raw = rt - rt[anchor]
    s = np.floor(raw @ hinv + ty.type(0.5)) @ h
    s = np.where(s == 0, ty.type(0), s)
    d = raw - s
    m = 1.0 / im.astype(np.float64)
    M, md, mv = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
    np.add.at(M, anchor, m)
    np.add.at(md, anchor, m[:, None] * d.astype(np.float64))
    np.add.at(mv, anchor, m[:, None] * v.astype(np.float64))
    M = M[anchor]
    Rc = (rt[anchor].astype(np.float64) + md[anchor] / M[:, None]) + s.astype(np.float64)
    return dict(Rc=Rc, Vc=mv[anchor] / M[:, None], M=M, anchor=anchor, s=s.astype(np.float64), d=d.astype(np.float64))


def _ext(t):
    return np.asarray(t.astype(np.longdouble).sum(axis=0), dtype=np.float64).reshape(3, 3)


def sums_restated(r, v, g, im, labels, box, image_dtype=np.float64):
    """(kin, rg, sum|terms| of kin, sum|terms| of rg): kin = sum_c M V_c (x) V_c (not divided by ACC), rg = sum_i R_c(i) (x) g_i;
    the terms in float64, their sums in long double"""
    q = mol_restated(r, v, im, labels, box, image_dtype)
    is_anchor = q['anchor'] == np.arange(len(labels))
    vc, m = q['Vc'][is_anchor], q['M'][is_anchor]
    kin_t = (vc[:, :, None] * vc[:, None, :] * m[:, None, None]).reshape(-1, 9)
    rg_t = (q['Rc'][:, :, None] * g.astype(np.float64)[:, None, :]).reshape(-1, 9)
    return _ext(kin_t), _ext(rg_t), _ext(np.abs(kin_t)), _ext(np.abs(rg_t))


def sums_bars(r, v, g, im, labels, box, is_double):
    """(kin, rg, bar of kin, bar of rg) for a handle (or host run) of that precision, from its own rounded inputs"""
    if is_double:
        kin, rg, ka, ra = sums_restated(r, v, g, im, labels, box)
        return kin, rg, 64 * E64 * ka, 64 * E64 * ra
    kin, rg, ka, ra = sums_restated(r, v, g, im, labels, box, np.float32)
    kin64, rg64, _, _ = sums_restated(r, v, g, im, labels, box, np.float64)
    return kin, rg, 64 * E64 * ka + 16.0 * np.abs(kin - kin64), 64 * E64 * ra + 16.0 * np.abs(rg - rg64)


def scale_restated(r, v, im, labels, box, mu_m1, inv_mu_m1):
    """float64: (r + (mu - 1) R_c(i), v + (1/mu - 1) V_c, the restatement's dict)"""
    q = mol_restated(r, v, im, labels, box)
    return r.astype(np.float64) + mu_m1 * q['Rc'], v.astype(np.float64) + inv_mu_m1 * q['Vc'], q


def group_vectors(r, labels, box):
    """float64 minimum-image vectors r_i - r_anchor(i), the box as given"""
    q = mol_restated(np.asarray(r, dtype=np.float64), np.zeros_like(r, dtype=np.float64), np.ones(len(r)), labels, box)
    return q['d']


# ---- the host program -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the headers cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('mol_shim') / 'mol_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I', CSRC, '-o', exe, SHIM])
    return exe


def labels_text(tile_atoms, labels):
    return '%d %d\n%s\n' % (len(labels), tile_atoms, ' '.join(str(int(x)) for x in labels))


def run_plan(shim, tile_atoms, labels):
    out = subprocess.run([shim, 'plan'], input=labels_text(tile_atoms, labels), capture_output=True, text=True, check=True).stdout
    if out.startswith('error'):
        return out.strip()
    got = {}
    for line in out.strip().split('\n'):
        name, *vals = line.split()
        got[name] = np.array([int(x) for x in vals], dtype=int)
    return got


def check_plan(shim, tile_atoms, labels):
    got, want = run_plan(shim, tile_atoms, labels), plan_restated(labels, tile_atoms)
    assert isinstance(got, dict), got
    n = len(labels)
    s = got['scalars']
    assert list(s[:5]) == [n, tile_atoms, want['n_tiles'], want['n_groups'], want['max_group']]
    for name in ('tile_atom0', 'atom_id', 'tile_grp0', 'grp_atom0', 'slot_grp'):
        assert np.array_equal(got[name], want[name]), name
    sizes = np.diff(want['tile_atom0'])
    assert sizes.max() <= tile_atoms and sorted(got['atom_id']) == list(range(n))
    a, g = int(sizes.max()), int(np.diff(want['tile_grp0']).max())
    assert list(s[5:7]) == [a, g]
    assert s[7] == 56 * g + 28 * a and s[8] == 56 * g + 56 * a
    assert s[9] == (64 if tile_atoms <= 64 else 128 if tile_atoms <= 128 else 256)
    # a group's atoms ascend, its first slot is its smallest atom, and its members carry one label
    for k in range(want['n_groups']):
        atoms = want['atom_id'][want['grp_atom0'][k]:want['grp_atom0'][k + 1]]
        assert list(atoms) == sorted(atoms) and len({int(labels[i]) for i in atoms}) == 1
    firsts = want['atom_id'][want['grp_atom0'][:-1]]
    assert list(firsts) == sorted(firsts)
    return want


def test_constants_match_the_python_side(shim):
    import ast
    out = subprocess.run([shim, 'consts'], capture_output=True, text=True, check=True).stdout.split()
    tree = ast.parse(open(ROOT + '/admp_amd/md.py').read())
    consts = {t.id: n.value.value for c in tree.body if isinstance(c, ast.ClassDef) and c.name == 'MolecularCRescaleBarostat'
              for n in c.body if isinstance(n, ast.Assign) and isinstance(n.value, ast.Constant) for t in n.targets}
    assert int(out[0]) == consts['MAX_TILE_ATOMS'] and 1 <= int(out[1]) <= int(out[0])


@pytest.mark.parametrize('cap,tiles', [(3, 5), (7, 3), (15, 1)])
def test_five_waters(shim, cap, tiles):
    """a group is never split; with capacity 7 two waters share a tile"""
    want = check_plan(shim, cap, np.repeat(np.arange(5), 3))
    assert want['n_tiles'] == tiles and want['n_groups'] == 5
    if cap == 7:
        assert list(np.diff(want['tile_atom0'])) == [6, 6, 3]


def test_singletons_only(shim):
    want = check_plan(shim, 2, np.arange(5))
    assert want['n_tiles'] == 3 and want['n_groups'] == 5 and list(want['atom_id']) == list(range(5))
    assert check_plan(shim, 64, [0])['n_tiles'] == 1
    want = check_plan(shim, 256, np.arange(1000))
    assert want['n_tiles'] == 4 and list(np.diff(want['tile_atom0'])) == [256, 256, 256, 232]


def test_sparse_and_shuffled_labels(shim):
    """the labels are names only: sparse, unordered, up to 2^31 - 1; the order of the groups is that of their smallest atom"""
    labels = [2 ** 31 - 1, 7, 7, 0, 2 ** 31 - 1, 1000000, 0, 7, 5]
    want = check_plan(shim, 4, labels)
    assert list(want['atom_id']) == [0, 4, 1, 2, 7, 3, 6, 5, 8] and list(want['grp_atom0']) == [0, 2, 5, 7, 8, 9]
    assert list(np.diff(want['tile_atom0'])) == [2, 3, 4]
    perm = np.random.default_rng(2).permutation(17)
    lab = np.empty(17, dtype=int)
    lab[perm] = np.repeat([40, 3, 900, 11, 12], [3, 3, 5, 5, 1])
    want = check_plan(shim, 8, lab)
    assert want['max_group'] == 5 and want['n_groups'] == 5


def test_interleaved_groups(shim):
    """molecule m owns atoms m, 4 + m, 8 + m: packing follows the smallest atom, slots ascend within a group"""
    want = check_plan(shim, 6, np.tile(np.arange(4), 3))
    assert list(want['atom_id'][:6]) == [0, 4, 8, 1, 5, 9] and list(want['slot_grp']) == [0, 0, 0, 1, 1, 1] * 2


def test_refusals_of_the_plan(shim):
    msg = run_plan(shim, 3, [0, 0, 1, 0, 0, 2])
    assert isinstance(msg, str) and 'a group of 4 atoms' in msg and 'smallest atom 0' in msg and 'tile_atoms 3' in msg
    assert plan_restated([0, 0, 1, 0, 0, 2], 3) == (4, 0)
    msg = run_plan(shim, 3, [5, 6, 9, 9, 6, 9, 8, 9])
    assert 'a group of 4 atoms' in msg and 'smallest atom 2' in msg
    consts = subprocess.run([shim, 'consts'], capture_output=True, text=True, check=True).stdout.split()
    for cap in (0, -1, int(consts[0]) + 1):
        msg = run_plan(shim, cap, [0, 0, 1])
        assert isinstance(msg, str) and 'tile_atoms %d outside 1..%s' % (cap, consts[0]) in msg
    assert isinstance(run_plan(shim, int(consts[0]), [0, 0, 1]), dict)
    msg = run_plan(shim, 3, [0, 4, -2, 1])
    assert isinstance(msg, str) and 'atom 2' in msg and 'negative group label -2' in msg
    msg = run_plan(shim, 3, [])
    assert isinstance(msg, str) and 'n_atoms must be positive' in msg


# ---- the two runs ----------------------------------------------------------------------------------------------------------
MU_M1 = float(np.expm1(2.5e-3 / 3.0))
INV_MU_M1 = float(np.expm1(-2.5e-3 / 3.0))


@pytest.fixture(scope='module')
def run_case():
    """8 rigid waters, two of them wrapped across faces, two stars and a chain (40 atoms), shuffled, triclinic; 300 K, a random
    gradient"""
    r, v, mass, con, wrapped = rigid_system(8, 0, 5, [((0, 0),), ((2, 1),)])
    labels = labels_of(len(r), con.pairs)
    assert sum(1 for w in wrapped if w) >= 2 and len(r) == 40 and len(set(labels)) == 11
    g = np.random.default_rng(6).normal(size=r.shape) * 30.0
    q = mol_restated(r, v, 1.0 / mass, labels, BOX)
    assert (np.abs(q['s']).sum(1) > 0).sum() >= 2                   # atoms in another image than their anchor
    assert np.abs(q['d']).max() < 4.0                                # every group is whole under the image
    return r, v, g, mass, labels


def run_shim(shim, op, prec, cap, labels, r, v, g, im):
    n = len(r)
    text = labels_text(cap, labels) + ' '.join('%.17g' % x for x in BOX.ravel()) + '\n%.17g %.17g\n' % (MU_M1, INV_MU_M1)
    text += '\n'.join(' '.join('%.17g' % x for x in list(r[i]) + list(v[i]) + list(g[i]) + [im[i]]) for i in range(n)) + '\n'
    out = subprocess.run([shim, op, prec], input=text, capture_output=True, text=True, check=True).stdout
    vals = np.array(out.split(), dtype=np.float64)
    assert len(vals) == (18 if op == 'sums' else 6 * n), out[:200]
    return vals


@pytest.mark.parametrize('prec', ['d', 'f'])
@pytest.mark.parametrize('cap', [6, 7, 64])
def test_sums_and_scale_against_the_restatement(shim, run_case, prec, cap):
    r, v, g, mass, labels = run_case
    ty = np.float64 if prec == 'd' else np.float32
    eps = float(np.finfo(ty).eps)
    rr, vr, gr, imr = (x.astype(ty) for x in (r, v, g, 1.0 / mass))      # what the program reads
    kin, rg, kin_bar, rg_bar = sums_bars(rr, vr, gr, imr, labels, BOX, prec == 'd')
    w = run_shim(shim, 'sums', prec, cap, labels, r, v, g, 1.0 / mass)
    dk, dg = np.abs(w[:9].reshape(3, 3) - kin), np.abs(w[9:].reshape(3, 3) - rg)
    print('%s cap %d sums: kin %.2e of %.2e, rg %.2e of %.2e' % (prec, cap, dk.max(), kin_bar.min(), dg.max(), rg_bar.min()))
    assert (dk <= kin_bar).all() and (dg <= rg_bar).all()
    assert np.abs(kin).max() > 1e-3 and np.abs(rg).max() > 100.0
    # the atomic sums differ by far more than the bar: the case can tell the two apart
    atomic = _ext(((rr.astype(np.float64))[:, :, None] * gr.astype(np.float64)[:, None, :]).reshape(-1, 9))
    assert np.abs(atomic - rg).max() > 1e3 * rg_bar.max()
    out = run_shim(shim, 'scale', prec, cap, labels, r, v, g, 1.0 / mass)
    n = len(r)
    r1, v1 = out[:3 * n].reshape(n, 3), out[3 * n:].reshape(n, 3)
    r_ref, v_ref, q = scale_restated(rr, vr, imr, labels, BOX, MU_M1, INV_MU_M1)
    dr, dv = np.abs(r1 - r_ref).max(), np.abs(v1 - v_ref).max()
    print('%s cap %d scale: |dr| %.2e of %.2e, |dv| %.2e of %.2e' % (prec, cap, dr, 4 * eps * np.abs(r).max(), dv, 4 * eps * np.abs(v).max()))
    assert dr <= 4 * eps * np.abs(r).max() and dv <= 4 * eps * np.abs(v).max()
    assert np.abs(r1 - rr).max() > 100 * eps * np.abs(r).max()
    # a group moves rigidly: every vector to the anchor is unchanged to 2 ulp of the coordinates, in the scaled cell
    d0, d1 = group_vectors(rr, labels, BOX), group_vectors(r1, labels, BOX * (1.0 + MU_M1))
    assert np.abs(d1 - d0).max() <= 2 * eps * np.abs(r).max()
    # atoms of a group in the same image receive the same displacement (the sum r + dr rounds once more: one ulp of r)
    same = (q['s'] == 0).all(axis=1)
    moved = r1 - rr.astype(np.float64)
    assert np.abs(moved[same] - moved[q['anchor'][same]]).max() <= eps * np.abs(r).max()


@pytest.mark.parametrize('prec', ['d', 'f'])
def test_results_do_not_depend_on_the_capacity(shim, run_case, prec):
    r, v, g, mass, labels = run_case
    outs = [run_shim(shim, 'scale', prec, cap, labels, r, v, g, 1.0 / mass) for cap in (6, 7, 40, 256)]
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


@pytest.mark.parametrize('prec', ['d', 'f'])
def test_singleton_groups_are_the_atomic_scaling(shim, run_case, prec):
    """every atom a group: R_c(i) = r_i, V_c = v_i, so the sums are the atomic ones and the update is r *= mu, v /= mu"""
    r, v, g, mass, _ = run_case
    ty = np.float64 if prec == 'd' else np.float32
    eps = float(np.finfo(ty).eps)
    n = len(r)
    rr, vr, gr = (x.astype(ty).astype(np.float64) for x in (r, v, g))
    m = 1.0 / (1.0 / mass).astype(ty).astype(np.float64)
    w = run_shim(shim, 'sums', prec, 7, np.arange(n)[::-1], r, v, g, 1.0 / mass)
    kin_t = (vr[:, :, None] * vr[:, None, :] * m[:, None, None]).reshape(-1, 9)
    rg_t = (rr[:, :, None] * gr[:, None, :]).reshape(-1, 9)
    assert (np.abs(w[:9].reshape(3, 3) - _ext(kin_t)) <= 64 * E64 * _ext(np.abs(kin_t))).all()
    assert (np.abs(w[9:].reshape(3, 3) - _ext(rg_t)) <= 64 * E64 * _ext(np.abs(rg_t))).all()
    out = run_shim(shim, 'scale', prec, 7, np.arange(n)[::-1], r, v, g, 1.0 / mass)
    assert np.abs(out[:3 * n].reshape(n, 3) - rr * (1.0 + MU_M1)).max() <= 4 * eps * np.abs(r).max()
    assert np.abs(out[3 * n:].reshape(n, 3) - vr * (1.0 + INV_MU_M1)).max() <= 4 * eps * np.abs(v).max()
