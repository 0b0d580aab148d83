"""Float64 reference of the neighbour search, the float32 band rule, and the seeded test systems shared by
tests/test_neighbour_ref_cpu.py (conditions on the inputs, no GPU) and tests/test_gpu_neighbour.py (the kernels of
admp_amd/csrc/cell_kernels.hip and nbr_kernels.hip).  Plain module: numpy (and the torch oracle for the energies) only.

brute_pairs   all i < j with d = r_i - r_j, s = d box^-1, d = (s - floor(s + 1/2)) box, |d| < rc in float64: the reference's
              rounding rule (admp/spatial.py:13-32), which is the arithmetic of min_image (admp_amd/csrc/pme_math.h).
band          the distance from rc within which a float32 evaluation of the same arithmetic may classify a pair differently:
              8 * 2^-24 * (max |position component| + largest column sum of |box|).  Inputs rounded to f32 (relative 2^-24
              each), one subtraction, two 3-term products: every step adds at most a few 2^-24 of the largest magnitude it
              handles, which the two terms bound (|r| for the subtraction, the column sum for s . box with |s| <= 1/2 ... 1).
emulate_f32   the same arithmetic step by step in numpy float32, box^-1 computed in double and rounded, the test d.d < (f32)rc^2
              as in the kernels.  test_neighbour_ref_cpu.py proves on every single-precision case that it differs from the
              reference only inside the band; the GPU test then measures where the kernels differ.
"""
import functools

import numpy as np

BAND_FACTOR = 8.0 * 2.0 ** -24
MSCALES = np.array([0.1, 0.3, 0.7, 1.0, 1.0])


# ---- reference ------------------------------------------------------------------------------------------------------------
def _min_image_rows(pi, pj, box, inv, dtype):
    """minimum-image vectors of pi - pj (broadcast), every operation in `dtype`, sums in the kernels' order"""
    d = (pi - pj).astype(dtype, copy=False)
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    s = [d0 * inv[0, k] + d1 * inv[1, k] + d2 * inv[2, k] for k in range(3)]
    half = dtype(0.5)
    s = [x - np.floor(x + half) for x in s]
    return [s[0] * box[0, k] + s[1] * box[1, k] + s[2] * box[2, k] for k in range(3)]


def _sweep(pos, box, rc, dtype, chunk=256):
    """(pairs (n, 2) int64 in lexicographic order, |d| of each) with the test made in `dtype`"""
    pos64 = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    box64 = np.asarray(box, dtype=np.float64).reshape(3, 3)
    inv = np.linalg.inv(box64).astype(dtype)
    p, b = pos64.astype(dtype), box64.astype(dtype)
    n = len(p)
    out_i, out_j, out_r = [], [], []
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        d = _min_image_rows(p[i0:i1, None, :], p[None, i0:, :], b, inv, dtype)        # columns j >= i0 only
        d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if dtype is np.float64:
            r = np.sqrt(d2)
            hit = r < rc
        else:
            r = np.sqrt(d2.astype(np.float64))
            hit = d2 < dtype(rc * rc)
        hit &= np.arange(i0, n)[None, :] > np.arange(i0, i1)[:, None]
        ii, jj = np.nonzero(hit)
        out_i.append(ii + i0)
        out_j.append(jj + i0)
        out_r.append(r[ii, jj])
    if not out_i:
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    pairs = np.stack([np.concatenate(out_i), np.concatenate(out_j)], axis=1).astype(np.int64)
    return pairs, np.concatenate(out_r).astype(np.float64)


def brute_pairs(pos, box, rc):
    """float64 reference: (pairs (n, 2) int64, rows i < j in lexicographic order; distances (n,))"""
    return _sweep(pos, box, rc, np.float64)


def emulate_f32(pos, box, rc):
    """the pair set a float32 evaluation of min_image gives (numpy, one rounding per operation)"""
    return _sweep(pos, box, rc, np.float32)[0]


def pair_distances(pos, box, pairs):
    """float64 minimum-image distance of the given (n, 2) rows"""
    pos = np.asarray(pos, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64).reshape(3, 3)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        return np.zeros(0)
    d = _min_image_rows(pos[pairs[:, 0]], pos[pairs[:, 1]], box, np.linalg.inv(box), np.float64)
    return np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def band(pos, box):
    pos = np.asarray(pos, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64).reshape(3, 3)
    return BAND_FACTOR * (np.abs(pos).max() + np.abs(box).sum(axis=0).max())


def heights(box):
    inv = np.linalg.inv(np.asarray(box, dtype=np.float64).reshape(3, 3))
    return 1.0 / np.sqrt((inv * inv).sum(axis=0))


def as_set(pairs):
    return set(map(tuple, np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist()))


# ---- comparison helpers (the GPU tests call these; the CPU suite feeds them mutated references: they must fail) -------------
def check_pair_list(got, pos, box, rc, ref_pairs, prec):
    """Structure of a half pair list and its content against the reference.  double: the sets and counts are equal.  single:
    every pair of the symmetric difference lies within band of rc, and the counts differ by no more than there are such
    pairs.  Returns the largest |r - rc| / band over the differing pairs (0.0 when the sets are equal)."""
    got = np.asarray(got, dtype=np.int64).reshape(-1, 2)
    na = len(pos)
    assert len(got) == 0 or (got.min() >= 0 and got.max() < na), 'index out of range'
    assert (got[:, 0] < got[:, 1]).all(), 'a row with i >= j'
    assert (np.diff(got[:, 0]) >= 0).all(), 'rows are not grouped by non-decreasing i'
    key = got[:, 0] * np.int64(max(na, 1)) + got[:, 1]
    assert len(np.unique(key)) == len(key), 'duplicate rows'
    a, b = as_set(got), as_set(ref_pairs)
    diff = sorted(a ^ b)
    if prec == 'double':
        assert not diff and len(got) == len(ref_pairs), \
            '%d pairs differ (first %s), %d rows against %d' % (len(diff), diff[:4], len(got), len(ref_pairs))
        return 0.0
    w = band(pos, box)
    if not diff:
        assert len(got) == len(ref_pairs)
        return 0.0
    off = np.abs(pair_distances(pos, box, np.array(diff)) - rc)
    assert off.max() <= w, 'pair %s differs at |r - rc| = %.3e, band %.3e' % (diff[int(off.argmax())], off.max(), w)
    assert abs(len(got) - len(ref_pairs)) <= len(diff)
    return float(off.max() / w)


def tt_reference(sysm, pairs, mScales=MSCALES, want_mscale=True):
    """Tang-Toennies energy, gradient and dE/dmScales of `pairs` (float64, oracle.admp_oracle); rows are taken as they are,
    so a row listed twice counts twice (the reference's own behaviour).  dE/dmScales[k] = energy at the one-hot mScales e_k:
    the energy is linear in them."""
    import torch
    from oracle import admp_oracle as O
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    par = sysm['params']
    if len(pairs) == 0:
        return dict(E=0.0, grad=np.zeros_like(sysm['pos']), dm=np.zeros(len(mScales)))
    pos, box = np.array(sysm['pos']), np.array(sysm['box'])
    out = O.tt_energy_and_grad(pos, box, pairs, mScales, sysm['cov'], *par)
    if want_mscale:
        T = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64))   # noqa: E731
        cls = (O.pair_nbonds(sysm['cov'], pairs) - 1) % len(mScales)      # the entry of mScales each pair reads
        ones = T(np.ones(len(mScales)))
        dm = []
        for k in range(len(mScales)):
            sub = pairs[cls == k]                                         # one-hot mScales = the energy of that class alone
            dm.append(float(O.tt_damping_energy(T(pos), T(box), sub, ones, sysm['cov'], *[T(p) for p in par])) if len(sub) else 0.0)
        out['dm'] = np.array(dm)
    return out


def tt_band_slack(sysm, ref_pairs, ref_r, rc, mScales=MSCALES):
    """(sum |pair energy|, sum |pair gradient|, sum |pair dE/dmScales|) over the reference pairs within band of rc: what a
    single-precision run may gain or lose by classifying them differently.  From the reference alone."""
    w = band(sysm['pos'], sysm['box'])
    near = np.nonzero(np.abs(ref_r - rc) <= w)[0]
    e = g = m = 0.0
    for k in near:
        one = tt_reference(sysm, ref_pairs[k:k + 1], mScales)
        e += abs(one['E'])
        g += np.linalg.norm(one['grad'])
        m += np.abs(one['dm']).max()
    return e, g, m


def check_tt(got, ref, prec, slack=(0.0, 0.0, 0.0), n_pairs_ref=None, n_band=0):
    """got = dict(E, grad, dm (optional), n_pairs) of the HIP calculator against tt_reference.  double: 1e-11 relative
    (energy to |E|, gradient in L2, dE/dmScales to its largest entry).  single: 2e-5 / 2e-4 / 2e-4 plus the band slack."""
    tolE, tolG = (1e-11, 1e-11) if prec == 'double' else (2e-5, 2e-4)
    if n_pairs_ref is not None:
        assert abs(got['n_pairs'] - n_pairs_ref) <= (0 if prec == 'double' else n_band), (got['n_pairs'], n_pairs_ref)
    assert abs(got['E'] - ref['E']) <= tolE * abs(ref['E']) + slack[0], (got['E'], ref['E'])
    dg = np.linalg.norm(np.asarray(got['grad'], dtype=np.float64) - ref['grad'])
    assert dg <= tolG * np.linalg.norm(ref['grad']) + slack[1], (dg, np.linalg.norm(ref['grad']))
    if got.get('dm') is not None:
        dd = np.abs(np.asarray(got['dm']) - ref['dm']).max()
        assert dd <= tolG * np.abs(ref['dm']).max() + slack[2], (got['dm'], ref['dm'])


# ---- inputs: pair-list cases (a) ---------------------------------------------------------------------------------------------
def _shuffled(rng, pos):
    pos = np.asarray(pos, dtype=np.float64)
    return pos[rng.permutation(len(pos))]


def _clusters(rng, box_diag, n_clusters, per, spread):
    c = rng.uniform(0, 1, (n_clusters, 1, 3)) * box_diag
    return (c + rng.uniform(-spread, spread, (n_clusters, per, 3))).reshape(-1, 3)


def _dimers_across(rng, box_diag, axes_list, n_each, lo=1.0, hi=3.5):
    """dimers whose two atoms sit on either side of the periodic faces named by axes_list (1 axis: a face, 2: an edge,
    3: a corner); separation lo..hi"""
    out = []
    for axes in axes_list:
        for _ in range(n_each):
            c = rng.uniform(0.1, 0.9, 3) * box_diag
            u = rng.normal(size=3)
            for ax in axes:
                c[ax] = 0.0
                u[ax] = abs(u[ax]) + 0.3
            u *= 0.5 * rng.uniform(lo, hi) / np.linalg.norm(u)
            out += [c - u, c + u + (box_diag * np.isin(np.arange(3), axes))]    # second atom one lattice vector further
    return np.array(out)


def _gen_pairlist_case(name, seed):
    """-> dict(pos, box, rc, precs, exact) ; exact: the case holds pairs at r = rc on purpose (exempt from the 1e-9 rule)"""
    rng = np.random.default_rng(seed)
    cube = lambda L: np.diag([float(L)] * 3)      # noqa: E731
    precs, exact = ('double', 'single'), False
    if name.startswith('na'):
        n = int(name[2:])
        box, rc = cube(20), 5.0
        pos = rng.uniform(0, 20, (n, 3))
    elif name == 'two_far':
        box, rc = cube(20), 5.0
        pos = np.array([[1.0, 2.0, 3.0], [9.5, 11.0, 12.5]])
    elif name == 'two_cells':
        box, rc, precs, exact = cube(20), 10.0, ('double',), True
        pos = rng.uniform(0, 20, (596, 3))
        planted = np.array([[1.0, 3.25, 7.5], [11.0, 3.25, 7.5],                        # r = rc exactly: absent
                            [2.0, 14.5, 1.25], [2.0, 14.5, 1.25 + 10.0 * (1 - 1e-12)]])    # just inside: present
        pos = np.concatenate([pos, planted])
        perm = rng.permutation(len(pos))
        inv = np.argsort(perm)
        return dict(pos=pos[perm], box=box, rc=rc, precs=precs, exact=True,
                    absent=(int(inv[596]), int(inv[597])), present=(int(inv[598]), int(inv[599])))
    elif name == 'three_cells':
        box, rc = np.diag([15.0, 20.0, 31.0]), 5.0
        pos = rng.uniform(0, 1, (500, 3)) * np.diag(box)
    elif name == 'mixed_cells':
        box, rc = np.diag([10.5, 15.5, 40.0]), 5.0
        pos = rng.uniform(0, 1, (500, 3)) * np.diag(box)
    elif name == 'multiple_rc':
        box, rc = cube(20), 5.0
        pos = rng.uniform(0, 20, (488, 3))
        planted = []
        for ax in range(3):                       # separation rc (1 - 1e-7) along one axis, straddling a cell face
            for face in (5.0, 15.0):
                a = rng.uniform(0, 20, 3)
                a[ax] = face - rng.uniform(0.5, 4.5)
                b = a.copy()
                b[ax] = a[ax] + rc * (1 - 1e-7)
                planted += [a, b]
        pos = np.concatenate([pos, np.array(planted)])
    elif name == 'faces':
        box, rc = cube(21), 5.0                   # 4 cells of width 5.25 on every axis
        f = np.array([0.0, 0.25, 0.5, 0.75, 1.0, -1e-17, 1 - 2.0 ** -53])
        grid = np.stack(np.meshgrid(f, f, f, indexing='ij'), axis=-1).reshape(-1, 3)
        grid = grid[rng.permutation(len(grid))[:120]]
        corners = np.stack(np.meshgrid(f[[0, 4, 5, 6]], f[[0, 4, 5, 6]], f[[0, 4, 5, 6]], indexing='ij'), axis=-1).reshape(-1, 3)
        special = np.concatenate([grid, corners[rng.permutation(len(corners))[:16]]]) * 21.0
        u = rng.normal(size=(len(special), 2, 3))
        u *= rng.uniform(1.0, 4.5, (len(special), 2, 1)) / np.linalg.norm(u, axis=2, keepdims=True)
        partners = (special[:, None, :] + u).reshape(-1, 3)              # on every side of the faces, edges and corners
        pos = np.concatenate([special, partners, rng.uniform(0, 21, (100, 3))])
    elif name in ('far50', 'far3'):
        box, rc = cube(20), 5.0
        m = 50 if name == 'far50' else 3
        precs = ('double',) if name == 'far50' else ('double', 'single')
        pos = rng.uniform(0, 20, (400, 3)) + rng.integers(-m, m + 1, (400, 3)) * 20.0
    elif name == 'tri_a':
        box, rc = np.array([[14.0, 0, 0], [2.5, 13.0, 0], [-1.5, 2.0, 15.0]]), 5.0
        pos = rng.uniform(-5, 20, (400, 3))
    elif name == 'tri_b':
        box, rc = np.array([[16.0, 0, 0], [7.5, 13.0, 0], [-6.0, 5.0, 15.0]]), 6.0
        pos = rng.uniform(0, 1, (450, 3)) @ box
    elif name == 'block':
        box, rc = cube(40), 11.0
        g = np.stack(np.meshgrid(*[np.arange(7.0)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)
        pos = np.concatenate([g + 12.0 + rng.uniform(-0.1, 0.1, g.shape), rng.uniform(0, 40, (200, 3))])
    elif name == 'clamp1024':
        box, rc = np.diag([5000.0, 30.0, 30.0]), 4.0      # 1250 cells along x, clamped to 1024
        d = np.diag(box)
        pos = np.concatenate([_clusters(rng, d, 20, 5, 2.0), _dimers_across(rng, d, [(0,)], 25)])
    elif name == 'halving':
        box, rc = cube(5000), 4.0                         # 1024^3 cells, halved twice to 256^3
        d = np.diag(box)
        axes = [(0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)]
        pos = np.concatenate([_clusters(rng, d, 24, 5, 2.0), _dimers_across(rng, d, axes, 5), _clusters(rng, d, 5, 2, 1.5)])
    else:
        raise KeyError(name)
    return dict(pos=_shuffled(rng, pos), box=np.asarray(box, dtype=np.float64), rc=float(rc), precs=precs, exact=exact)


DOUBLE_ONLY = ('two_cells', 'far50')       # exact r = rc planted; shifts of +-50 cells
PAIRLIST_CASES = ['na1', 'na2', 'na63', 'na64', 'na65', 'na127', 'na128', 'na129', 'na257', 'two_far', 'two_cells',
                  'three_cells', 'mixed_cells', 'multiple_rc', 'faces', 'far50', 'far3', 'tri_a', 'tri_b', 'block',
                  'clamp1024', 'halving']


def _clear_of_rc(pos, box, rc, margin=1e-9, lo=0.0):
    """no float64 pair distance within `margin` of rc (searched with a slightly larger radius), none below lo"""
    rr = rc + 2 * margin
    _, r = brute_pairs(pos, box, rr)
    return not (np.abs(r - rc) < margin).any() and (len(r) == 0 or r.min() >= lo)


@functools.lru_cache(maxsize=None)
def pairlist_case(name):
    """the case, reseeded until no reference pair lies within 1e-9 of rc (cases built around r = rc are exempt), with its
    float64 reference: keys pos, box, rc, precs, exact, ref_pairs, ref_r"""
    base = 1000 + 17 * PAIRLIST_CASES.index(name)
    for k in range(50):
        c = _gen_pairlist_case(name, base + k)
        if c['exact'] or _clear_of_rc(c['pos'], c['box'], c['rc']):
            break
    else:
        raise RuntimeError('no seed keeps %s clear of rc' % name)
    c['ref_pairs'], c['ref_r'] = brute_pairs(c['pos'], c['box'], c['rc'])
    for v in (c['pos'], c['box'], c['ref_pairs'], c['ref_r']):
        v.setflags(write=False)
    return c


# ---- inputs: systems of the table builders (b), (c) --------------------------------------------------------------------------
TRI_BIG = 2.0 * np.array([[16.0, 0, 0], [7.5, 13.0, 0], [-6.0, 5.0, 15.0]])


def _lattice_gas(rng, n, box, jitter=0.25):
    """n atoms on distinct sites of a g^3 fractional grid of `box`, jittered by +-jitter (Cartesian), in shuffled order"""
    g = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    while g ** 3 < n:
        g += 1
    sites = rng.permutation(g ** 3)[:n]
    f = np.stack([sites // (g * g), (sites // g) % g, sites % g], axis=1) / float(g)
    return f @ box + rng.uniform(-jitter, jitter, (n, 3))


def _params(rng, n):
    """per-atom a, b, q, c6: a, b > 0 (square roots), b r >= 1.5 * 1.89 at the closest approach, so every term is finite"""
    return (rng.uniform(0.5, 2.0, n), rng.uniform(1.5, 2.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(0.5, 2.0, n))


def _chain_cov(n):
    """molecules of three consecutive atoms (in the SHUFFLED order: partners lie anywhere): 0-1, 1-2 class 1, 0-2 class 2"""
    import scipy.sparse as sp
    i = np.arange(0, n - 2, 3)
    r = np.concatenate([i, i + 1, i + 1, i + 2, i, i + 2])
    c = np.concatenate([i + 1, i, i + 2, i + 1, i + 2, i])
    v = np.concatenate([np.ones(4 * len(i)), 2 * np.ones(2 * len(i))]).astype(np.int32)
    return sp.csr_matrix((v, (r, c)), shape=(n, n), dtype=np.int32)


def _star_system(rng, n_stars, box):
    """a centre bonded to 8 leaves (centre-leaf class 1, leaf-leaf class 2): every atom has 8 covalent partners, two more
    than the row kernels keep in registers.  Centres on a jittered grid, leaves on the corners of a cube around them."""
    import scipy.sparse as sp
    g = int(np.ceil(n_stars ** (1.0 / 3.0) - 1e-9))
    L = np.diag(box)[0]
    sites = rng.permutation(g ** 3)[:n_stars]
    c = (np.stack([sites // (g * g), (sites // g) % g, sites % g], axis=1) + 0.5) * (L / g)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * 0.7
    pos = np.concatenate([c[:, None, :], c[:, None, :] + corners[None]], axis=1)        # (stars, 9, 3)
    pos = (pos + rng.uniform(-0.05, 0.05, pos.shape)).reshape(-1, 3)
    n = 9 * n_stars
    perm = rng.permutation(n)                    # perm[new] = old
    new_of = np.argsort(perm)
    r, cc, v = [], [], []
    for a in range(9):
        for b in range(9):
            if a != b:
                r.append(np.arange(n_stars) * 9 + a)
                cc.append(np.arange(n_stars) * 9 + b)
                v.append(np.full(n_stars, 1 if (a == 0 or b == 0) else 2))
    r, cc, v = new_of[np.concatenate(r)], new_of[np.concatenate(cc)], np.concatenate(v).astype(np.int32)
    return pos[perm], sp.csr_matrix((v, (r, cc)), shape=(n, n), dtype=np.int32)


def _gen_table_system(name, seed):
    rng = np.random.default_rng(seed)
    rc = 5.0
    if name.startswith('gas'):                   # gasN / gasN_tri
        n = int(name[3:].split('_')[0])
        if name.endswith('_tri'):
            box = TRI_BIG.copy()
            pos = _lattice_gas(rng, n, box, jitter=0.15)
        else:
            g = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
            L = max(12.0, 1.6 * g)
            box = np.diag([L] * 3)
            pos = _lattice_gas(rng, n, box)
        cov = _chain_cov(n)
    elif name.startswith('stars'):
        ns = int(name[5:])
        g = int(np.ceil(ns ** (1.0 / 3.0) - 1e-9))
        box = np.diag([max(12.0, 3.1 * g)] * 3)
        pos, cov = _star_system(rng, ns, box)
        n = len(pos)
    elif name == 'dilute':                       # no pair within rc 4 (minimum distance checked), pairs at rc 25
        n, rc = 50, 4.0
        box = np.diag([60.0] * 3)
        pos = _lattice_gas(rng, n, box, jitter=1.0)     # 4^3 grid of spacing 15
        cov = _chain_cov(n)
    elif name == 'switch65':                     # (c): clusters of exactly 65 and 66 mutually paired atoms, rows of 64 and 65
        rc = 8.0
        box = np.diag([40.0] * 3)
        g = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), np.arange(3.0), indexing='ij'), axis=-1).reshape(-1, 3) * 1.2
        g = g[rng.permutation(len(g))]
        pos = np.concatenate([g[:65] + 3.0, g[:66] + 23.0]) + rng.uniform(-0.08, 0.08, (131, 3))
        n = len(pos)
        cov = _chain_cov(n)
    elif name == 'sort_paths':                   # (c): degrees 342 (x343), <= 64 (gas) and 65..256 (blob) in one table
        rc = 11.0
        box = np.diag([40.0] * 3)
        g = np.stack(np.meshgrid(*[np.arange(7.0)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)
        block = g + 2.0 + rng.uniform(-0.1, 0.1, g.shape)             # x, y, z in 1.9 .. 8.1: all 343 within 10.8 of each other
        gas = _lattice_gas(rng, 200, np.diag([40.0, 40.0, 11.0]), jitter=0.3) + np.array([0, 0, 19.5])   # > 11 from the block
        b5 = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), np.arange(4.0), indexing='ij'), axis=-1).reshape(-1, 3)
        blob = b5 * 1.6 + np.array([24.0, 24.0, 2.0]) + rng.uniform(-0.1, 0.1, b5.shape)    # > 11 from block and gas
        pos = np.concatenate([block, gas, blob])          # NOT shuffled: the three row populations are index ranges
        n = len(pos)
        cov = _chain_cov(n)
    else:
        raise KeyError(name)
    params = _params(rng, n)
    if name == 'dilute':                         # neighbours are 13 A and more apart: a slower decay keeps the terms of size
        params = (params[0], 0.1 * params[1], params[2], params[3])
    return dict(pos=pos, box=box, rc=rc, cov=cov, params=params)


TABLE_SYSTEMS = ['gas1', 'gas15', 'gas16', 'gas17', 'gas1023', 'gas1024', 'gas1025', 'gas4096', 'gas4097', 'gas4200',
                 'gas4097_tri', 'gas4200_tri', 'stars40', 'stars470', 'dilute', 'gas5000', 'gas2000', 'sort_paths', 'switch65']


@functools.lru_cache(maxsize=None)
def table_system(name):
    """system of the table-builder tests, reseeded until no pair lies within 1e-9 of rc and none is closer than 1 A (0.75 A in
    the 1.0 A block of sort_paths); with the float64 reference pairs at its rc (ref_pairs, ref_r)"""
    base = 5000 + 13 * TABLE_SYSTEMS.index(name)
    for k in range(50):
        s = _gen_table_system(name, base + k)
        if _clear_of_rc(s['pos'], s['box'], s['rc'], lo=0.75 if name == 'sort_paths' else 1.0):
            break
    else:
        raise RuntimeError('no seed keeps %s clear of rc' % name)
    s['ref_pairs'], s['ref_r'] = brute_pairs(s['pos'], s['box'], s['rc'])
    for v in (s['pos'], s['box'], s['ref_pairs'], s['ref_r']):
        v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def table_reference(name, rc=None):
    """(ref_pairs, ref_r, tt_reference, band slack, pairs within band) of a table system at rc (default: its own)"""
    s = table_system(name)
    rc = s['rc'] if rc is None else rc
    if rc == s['rc']:
        pairs, r = s['ref_pairs'], s['ref_r']
    else:
        assert _clear_of_rc(s['pos'], s['box'], rc), (name, rc)
        pairs, r = brute_pairs(s['pos'], s['box'], rc)
    ref = tt_reference(s, pairs)
    slack = tt_band_slack(s, pairs, r, rc)
    n_band = int((np.abs(r - rc) <= band(s['pos'], s['box'])).sum())
    return pairs, r, ref, slack, n_band
