"""The dipole observable restated in float64 numpy (include/admp_hip.h admp_pme_dipoles; admp_amd/csrc/dipole_math.h), its test
cases, and the bars of tests/test_dipole_cpu.py and tests/test_gpu_dipoles.py.

Definitions.  Groups are labels; a group's anchor a is its lowest-numbered atom; for atom i of group c

    d_i  = minimum image of r_i - r_a              D_c = sum m_i d_i / M_c
    p_i  = x_loc X_i + y_loc Y_i + z_loc Z_i       (z_loc, x_loc, y_loc) = Q_local[i, 1:4]; X, Y, Z the rows of the local frame
    mu_c = sum_i [ q_i (d_i - D_c) + p_i + U_i ]   M = sum_c mu_c

The frames are oracle.construct_local_frames; a site without a z atom has the identity frame.

Bars.  Every word comes with sum |terms|, the magnitudes of what was added to make it:

    charge part     |q_i| (a_i,k + sum_j m_j a_j,k / M_c),  a_i,k = |(r_i - r_a)_k| + |s_i,k|
                    d_i is the difference r_i - r_a minus the lattice translation s_i the image applied, a sum of lattice
                    vectors that is itself rounded: both magnitudes count (s_i = 0: a_i = |d_i|); the second term is what entered D_c
    permanent part  (|x_loc| + |y_loc| + |z_loc|) f_i,  f_i = max(1, max over the site's axis atoms j of
                    (|r_j - r_i|_inf + |s_ij|_inf) / |d_ij|)
                    a frame row is a unit vector: the rounding error of each of its components scales with its length, 1, not
                    with the component, and it is made of the unit vectors d_ij / |d_ij|, whose error is that of d_ij -- the
                    magnitudes as above -- over its length
    induced part    |U_i,k|

T_c,k is their sum over a group's atoms.  sum |mu_c| and max |mu_c| move by at most sum_k (error of mu_c,k): their terms are sum_c
sum_k T_c,k and max_c sum_k T_c,k; |mu_c|^2 moves by 2 |mu_c| times that and |mu_c| <= sum_k T_c,k: 2 sum_c (sum_k T_c,k)^2.
A double handle is held to 64 eps_f64 sum |terms| per word, the rule of check_sums in tests/test_gpu_md_barostat.py; a single
handle to 4 SINGLE_RATIO eps_f32 sum |terms| (SINGLE_RATIO: below).

Cases: water64 (64 waters translated by half a lattice spacing and wrapped atom by atom, so that molecules straddle faces) and
general (300 groups -- 120 single atoms, 179 triples, one compact group of 70 --, every axis rule, random Q_local and U, atom
order shuffled, labels neither dense nor sorted, atoms moved out of the cell by whole lattice vectors), each in a cubic and a
triclinic cell.  The general geometry is drawn so that no frame is ill-conditioned: the angles between the axis vectors of a
site stay between 30 and 150 degrees and a Z-only site's z axis stays away from the switch of its x axis, so that frames formed
in single and in double do not differ by more than roundoff."""
import functools

import numpy as np

from admp_amd import systems as S
from oracle import admp_oracle as O
from tests.pair_ref import TILT

EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23
# the largest err / (eps_f32 sum |terms|) of the host program of dipole_math.h in float arithmetic against this file, over every
# word and every mu_c of the four cases (tests/test_dipole_cpu.py measures it again and holds it to this figure).  Measured:
# water64 0.237, water64_tric 0.236, general 0.577, general_tric 0.509.
SINGLE_RATIO = 0.58
MASS_WATER = (15.999, 1.008, 1.008)
CASES = ('water64', 'water64_tric', 'general', 'general_tric')


def _ro(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def wrap(pos, box):
    """every atom on its own into the cell"""
    s = pos @ np.linalg.inv(box)
    return (s - np.floor(s)) @ box


def min_image(d, box):
    s = d @ np.linalg.inv(box)
    return d - np.floor(s + 0.5) @ box


def _water(tric):
    n_mol = 64
    pos, box = S.synthetic_water_box(n_mol, seed=20240)
    if tric:
        box = box @ TILT
    a = box / 4.0                                                      # the lattice of the 4 x 4 x 4 molecules
    whole = pos + 0.5 * a.sum(axis=0)
    pos = wrap(whole, box)
    moved = np.abs(pos - whole).max(axis=1) > 1e-9
    straddles = [len(set(moved[3 * m:3 * m + 3])) == 2 for m in range(n_mol)]
    at, ai, _ = S.water_topology(n_mol)
    par = S.water_parameters(n_mol, polarizable=True)
    rng = np.random.default_rng(411)
    U = rng.normal(size=(3 * n_mol, 3)) * 0.05 * (par['pol'] > 0)[:, None]
    return dict(pos=pos, box=box, Q_local=par['Q_local'].copy(), U=U, masses=np.tile(MASS_WATER, n_mol),
                axis_type=at.astype(np.int32), axis_idx=ai.astype(np.int32), labels=np.repeat(np.arange(n_mol), 3).astype(np.int32),
                n_straddling=int(np.sum(straddles)))


def _unit(v):
    return v / np.linalg.norm(v)


def _conditioned(kind, vz, vx=None, vy=None):
    vs = [v for v in (vz, vx, vy) if v is not None]
    for a in range(len(vs)):
        for b in range(a + 1, len(vs)):
            if np.linalg.norm(np.cross(vs[a], vs[b])) < 0.5:
                return False
    if kind == 4:
        return abs(abs(vz[0]) - 0.5) > 0.05
    if kind == 2:
        return np.linalg.norm(vx + vy) > 0.5 and np.linalg.norm(np.cross(vz, _unit(vx + vy))) > 0.3
    if kind == 3:
        s = vz + vx + vy
        return np.linalg.norm(s) > 0.5 and np.linalg.norm(np.cross(vx, _unit(s))) > 0.3
    return True


def _general(tric):
    rng = np.random.default_rng(5077)
    L = 30.0
    box = L * (TILT if tric else np.eye(3))
    sizes = [1] * 120 + [3] * 179 + [70]
    rng.shuffle(sizes)
    sites = rng.permutation(7 ** 3)[:len(sizes)]
    centres = (np.stack(np.unravel_index(sites, (7, 7, 7)), axis=1) + 0.5) / 7.0 @ box
    pos, at, ai, grp = [], [], [], []
    for g, (n, c) in enumerate(zip(sizes, centres)):
        first = len(pos)
        if n == 1:
            pos.append(c + rng.normal(size=3) * 0.2)
            at.append(None)                                           # filled in below: an axis atom of another group
            ai.append(None)
        elif n == 3:
            kinds = [int(rng.integers(0, 2)), int(rng.integers(0, 2)), 4]      # Z-then-X or bisector twice, one Z-only site
            while True:
                p = c + rng.normal(size=(3, 3)) * 0.7
                ok = True
                for k in range(3):
                    z, x = (k + 1) % 3, (k + 2) % 3
                    vz, vx = _unit(p[z] - p[k]), _unit(p[x] - p[k])
                    ok = ok and (_conditioned(4, vz) if kinds[k] == 4 else _conditioned(kinds[k], vz, vx))
                if ok and min(np.linalg.norm(p[a] - p[b]) for a, b in ((0, 1), (0, 2), (1, 2))) > 0.6:
                    break
            for k in range(3):
                pos.append(p[k])
                at.append(kinds[k])
                ai.append([first + (k + 1) % 3, first + (k + 2) % 3 if kinds[k] != 4 else -1, -1])
        else:
            p = c + rng.uniform(-1.0, 1.0, size=(n, 3)) * 2.4            # compact: 4.8 A wide in a 30 A cell
            for k in range(n):
                kind = (2, 3, 0, 1)[k % 4]                            # Z-bisect and threefold need three axis atoms
                for _ in range(1000):
                    z, x, y = rng.choice([j for j in range(n) if j != k], size=3, replace=False)
                    vz, vx, vy = (_unit(p[j] - p[k]) for j in (z, x, y))
                    if _conditioned(kind, vz, vx, vy if kind in (2, 3) else None):
                        break
                else:
                    raise RuntimeError('no well-conditioned frame')
                pos.append(p[k])
                at.append(kind)
                ai.append([first + z, first + x, first + y if kind in (2, 3) else -1])
        grp += [g] * n
    pos = np.array(pos)
    n_atoms = len(pos)
    singles = [i for i in range(n_atoms) if at[i] is None]
    for j, i in enumerate(singles):
        if j % 3 == 0:
            at[i], ai[i] = 5, [-1, -1, -1]                             # no axes: the identity frame
        elif j == 1:
            at[i], ai[i] = 0, [-1, -1, -1]                             # a rule without a z atom: the identity frame too
        else:                                                         # Z-only on an atom of another group
            while True:
                z = int(rng.integers(0, n_atoms))
                if z != i and _conditioned(4, _unit(min_image(pos[z] - pos[i], box))):
                    break
            at[i], ai[i] = 4, [z, -1, -1]
    at, ai, grp = np.array(at, dtype=np.int32), np.array(ai, dtype=np.int32), np.array(grp)
    assert set(at.tolist()) == {0, 1, 2, 3, 4, 5}
    # shuffle the atom order (groups are no runs of consecutive atoms any more) and give the groups arbitrary labels
    new = rng.permutation(n_atoms)                                     # old atom i becomes atom new[i]
    old = np.argsort(new)
    remap = np.concatenate([new, [-1]])                                # (-1 stays -1)
    labels = (rng.permutation(1000)[:len(sizes)] - 300)[grp]
    Q = rng.normal(size=(n_atoms, 9)) * np.array([1, .5, .5, .5, .3, .3, .3, .3, .3])
    U = rng.normal(size=(n_atoms, 3)) * 0.1
    masses = rng.uniform(1.0, 20.0, size=n_atoms)
    pos, at, ai, labels = pos[old], at[old], remap[ai[old]].astype(np.int32), labels[old].astype(np.int32)
    lattice = rng.integers(-2, 3, size=(n_atoms, 3)) * (rng.random(n_atoms) < 0.3)[:, None]
    pos = wrap(pos, box) + lattice @ box
    return dict(pos=pos, box=box, Q_local=Q, U=U, masses=masses, axis_type=at, axis_idx=ai, labels=labels, sizes=sizes)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _water(name.endswith('_tric')) if name.startswith('water64') else _general(name.endswith('_tric'))
    c['name'], c['n'] = name, len(c['pos'])
    return _ro(c)


def groups_brute(labels):
    """lists of atoms, ascending, the groups ordered by their smallest atom: the slow way"""
    out = {}
    for i, lab in enumerate(np.asarray(labels).tolist()):
        out.setdefault(lab, []).append(i)
    return sorted(out.values(), key=lambda a: a[0])


def frames(c, pos):
    at = np.where(c['axis_idx'][:, 0] < 0, 5, c['axis_type'])          # no z atom: the identity frame
    return O.construct_local_frames(np.array(pos), np.array(c['box']), at, c['axis_idx']).numpy()


def image_parts(raw, box):
    """(d, |raw| + |s|) of differences raw: the minimum image and the magnitudes that went into it"""
    s = np.floor(raw @ np.linalg.inv(box) + 0.5) @ box
    return raw - s, np.abs(raw) + np.abs(s)


def frame_scales(c, pos):
    """f_i of the module docstring"""
    at, ai = c['axis_type'], c['axis_idx']
    f = np.ones(len(pos))
    used = [(at != 5) & (ai[:, 0] >= 0), np.isin(at, (0, 1, 2, 3)) & (ai[:, 0] >= 0), np.isin(at, (2, 3)) & (ai[:, 0] >= 0)]
    for col, on in enumerate(used):
        i = np.nonzero(on)[0]
        d, a = image_parts(pos[ai[i, col]] - pos[i], c['box'])
        f[i] = np.maximum(f[i], a.max(axis=1) / np.linalg.norm(d, axis=1))
    return f


def reference(c, pos=None, Q_local=None, U='case', masses=None):
    """words (16), mu (n_groups, 3) and the sum |terms| of each (word_terms, mu_terms), in float64 with extended sums, of the
    case's arrays or of the ones given (what a device tensor holds, say); U=None: no induced dipoles"""
    pos = np.asarray(c['pos'] if pos is None else pos, dtype=np.float64)
    Q = np.asarray(c['Q_local'] if Q_local is None else Q_local, dtype=np.float64)
    U = c['U'] if isinstance(U, str) else U
    U = np.zeros_like(pos) if U is None else np.asarray(U, dtype=np.float64)
    m = np.asarray(c['masses'] if masses is None else masses, dtype=np.float64)
    box = c['box']
    F = frames(c, pos)
    p = Q[:, 2:3] * F[:, 0] + Q[:, 3:4] * F[:, 1] + Q[:, 1:2] * F[:, 2]
    tp = (np.abs(Q[:, 1:4]).sum(axis=1) * frame_scales(c, pos))[:, None] * np.ones(3)
    groups = groups_brute(c['labels'])
    ext = lambda a: np.asarray(a.astype(np.longdouble).sum(axis=0), dtype=np.float64)      # noqa: E731
    parts, terms = np.zeros((len(groups), 9)), np.zeros((len(groups), 9))
    for g, atoms in enumerate(groups):
        d, a = image_parts(pos[atoms] - pos[atoms[0]], box)
        M = ext(m[atoms])
        D = ext(m[atoms, None] * d) / M
        Dabs = ext(m[atoms, None] * a) / M
        q = Q[atoms, 0:1]
        parts[g] = np.concatenate([ext(q * (d - D)), ext(p[atoms]), ext(U[atoms])])
        terms[g] = np.concatenate([ext(np.abs(q) * (a + Dabs)), ext(tp[atoms]), ext(np.abs(U[atoms]))])
    mu = parts[:, 0:3] + parts[:, 3:6] + parts[:, 6:9]
    mu_terms = terms[:, 0:3] + terms[:, 3:6] + terms[:, 6:9]
    length = np.sqrt((mu * mu).sum(axis=1))
    T = mu_terms.sum(axis=1)
    words, wt = np.zeros(16), np.zeros(16)
    words[0:9], wt[0:9] = ext(parts), ext(terms)
    words[9], wt[9] = ext(length), ext(T)
    words[10], wt[10] = ext(length * length), 2.0 * ext(T * T)
    words[11], wt[11] = length.max(), T.max()
    words[12] = len(groups)
    return dict(words=words, mu=mu, word_terms=wt, mu_terms=mu_terms, groups=groups)


def excess(got_words, got_mu, ref, eps_bar):
    """the largest |got - ref| / (eps_bar sum |terms|) over the words and over mu (a word without terms must be exact)"""
    out = []
    for got, want, t in ((np.asarray(got_words), ref['words'], ref['word_terms']), (np.asarray(got_mu), ref['mu'], ref['mu_terms'])):
        err = np.abs(got - want)
        assert got.shape == want.shape
        assert (err[t == 0] == 0).all(), (got[t == 0], want[t == 0])
        out.append((err[t > 0] / (eps_bar * t[t > 0])).max())
    return max(out)
