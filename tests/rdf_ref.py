"""Cases and float64 reference of the radial distribution functions (admp_md_rdf: admp_amd/csrc/rdf_math.h, rdf_plan.h,
rdf_kernels.hip), shared by tests/test_rdf_cpu.py (the host program of the headers) and tests/test_gpu_rdf.py.

The reference is computed on the positions as a handle of the precision under test holds them (`held`), in float64, and yields
per channel the sorted distances of the counted pairs.  The minimum image is taken by brute force over 27 translations: with
s = (r_i - r_j) box^-1, n0 = rint(s) and d0 = (r_i - r_j) - n0 box, the shortest of |d0 - t box|, t in {-1, 0, 1}^3.

Why this equals the fractional wrap (t = 0) for r < half the smallest height, and why the brute force may be spared for most
pairs: the component of a vector along the normal of the lattice plane d is its fractional coordinate times the perpendicular
height h_d, so |x| >= |f_d| h_d for every d.  After the wrap |s_d - n0_d| <= 1/2, so an image with t_d != 0 has
|f_d| >= 1 - |s_d - n0_d| >= 1/2 and is at least h_d / 2 long: anything shorter than half the smallest height is the t = 0 image.
By the same bound a pair can have an image below R only if |d0| < R or (1 - |s_d - n0_d|) h_d < R for some d; the 27
translations are evaluated for exactly those pairs (R = r_max plus a margin far above any delta), and every other pair is
provably beyond r_max.

Acceptance rule (`violations`), on cumulative counts so that nothing can hide: with C_ref(d) the reference pairs of a channel
with r < d and C_got(k) the sum of the bins below k, for every channel and every edge e_k = k dr, k = 1 .. n_bins,
C_ref(e_k - delta) <= C_got(k) <= C_ref(e_k + delta), delta = rho eps_T S, S = max |coordinate| + the largest row sum of |box|.
In double rho = 64.  In single rho is measured: the host program in float arithmetic gives the largest |r_f32 - r_f64| /
(eps_f32 S) over the pairs below r_max of all cases (tests/test_rdf_cpu.py prints it), recorded below as SINGLE_RATIO, and the
GPU bar is four times it -- the convention of dipole_ref.SINGLE_RATIO: the factor covers another contraction order on the device.

Coordinates are random, never a lattice: a lattice puts distances exactly on bin edges."""
import functools
import itertools

import numpy as np

EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)
DOUBLE_RATIO = 64.0
# measured by tests/test_rdf_cpu.py::test_float_ratio_is_measured_and_within_the_recorded_figure (largest over the cases: 1.104,
# case n513_unwrapped), recorded with a little room
SINGLE_RATIO = 1.11
NOT_COUNTED = 15
KBRUTE = 4096          # admp_amd/csrc/cell_plan.h kBruteMax: the auto choice takes the tile form up to here


def channel(a, b, n_types):
    a, b = (a, b) if a <= b else (b, a)
    return a * n_types - a * (a - 1) // 2 + (b - a)


def heights(box):
    inv = np.linalg.inv(box)
    return 1.0 / np.sqrt((inv * inv).sum(axis=0))


def make_tags(types, groups):
    return (np.asarray(types, dtype=np.int64) | (np.asarray(groups, dtype=np.int64) << 4)).astype(np.int32)


def _box(kind, h):
    """a cell with (about) the perpendicular heights h: orthorhombic, or skewed by off-diagonal rows (heights recomputed)"""
    h = np.asarray(h, dtype=np.float64)
    if kind == 'ortho':
        return np.diag(h)
    return np.array([[h[0], 0.0, 0.0], [0.31 * h[0], h[1], 0.0], [-0.23 * h[0], 0.37 * h[1], h[2]]])


def _case(name, seed, n, box, r_frac, n_bins, n_types=2, groups='atoms', unwrap=0, uncounted=0.0, single=True, cluster=None,
          faces=None, raw_types=False):
    """r_max = r_frac x the smallest height.  groups: 'atoms' (no exclusions), 'triples' (molecules of 3), 'one' (all excluded)"""
    rng = np.random.default_rng(seed)
    box = np.asarray(box, dtype=np.float64)
    s = rng.random((n, 3))
    if cluster is not None:                      # all atoms inside one cell of the grid `cluster` (the others stay empty)
        s = (np.array([1.0, 0.0, 2.0]) + 0.05 + 0.9 * s) / np.asarray(cluster, dtype=np.float64)
    if faces is not None:                        # some atoms with one fractional coordinate exactly on a cell face or the fold
        g = np.asarray(faces, dtype=np.float64)
        for i in range(0, n, 5):
            d = i % 3
            s[i, d] = (i // 5 % (int(g[d]) + 1)) / g[d]
    if unwrap:
        s = s + rng.integers(-unwrap, unwrap + 1, size=(n, 3))
    pos = s @ box
    types = rng.integers(0, n_types, size=n)
    if n_types <= n:
        types[:n_types] = np.arange(n_types)     # every type occurs
    if raw_types:                                # tag types 8 .. 14, which count as "not counted"
        types = np.where(rng.random(n) < 0.3, rng.integers(8, 15, size=n), types)
    if uncounted:
        types = np.where(rng.random(n) < uncounted, NOT_COUNTED, types)
    grp = {'atoms': np.arange(n), 'triples': np.arange(n) // 3, 'one': np.zeros(n, dtype=np.int64)}[groups]
    r_max = r_frac * heights(box).min()
    return dict(name=name, n=n, pos=pos, box=box, types=types, groups=grp, tags=make_tags(types, grp), n_types=n_types,
                r_max=float(r_max), n_bins=n_bins, single=single)


def _water64(name, kind):
    """64 waters (types O = 0, H = 1; groups = molecules) at random places and orientations, then wrapped atom by atom so that
    molecules straddle the faces"""
    rng = np.random.default_rng(64)
    box = _box(kind, [12.4, 12.9, 13.3])
    centres = rng.random((64, 3)) @ box
    pos = np.zeros((192, 3))
    for m in range(64):
        q = rng.normal(size=(3, 3))
        q, _ = np.linalg.qr(q)
        local = np.array([[0.0, 0, 0], [0.9572 * np.sin(0.912), 0, 0.9572 * np.cos(0.912)], [-0.9572 * np.sin(0.912), 0, 0.9572 * np.cos(0.912)]])
        pos[3 * m:3 * m + 3] = centres[m] + local @ q
    s = pos @ np.linalg.inv(box)
    pos = (s - np.floor(s)) @ box
    types = np.tile([0, 1, 1], 64)
    grp = np.arange(192) // 3
    c = dict(name=name, n=192, pos=pos, box=box, types=types, groups=grp, tags=make_tags(types, grp), n_types=2,
             r_max=float(0.49 * heights(box).min()), n_bins=60, single=True)
    c['n_straddling'] = int(sum(np.abs(pos[3 * m + 1:3 * m + 3] - pos[3 * m]).max() > 3.0 for m in range(64)))
    return c


# name -> maker.  The heights are given in units of r_max through r_frac and the box: a grid of g cells along a direction
# needs g <= height / r_max < g + 1 (cell_plan.h cell_grid_dims).
_MAKERS = {
    'n1': lambda: _case('n1', 1, 1, _box('ortho', [9.0, 10.0, 11.0]), 0.3, 16, n_types=1),
    'n2': lambda: _case('n2', 2, 2, _box('ortho', [3.0, 3.2, 3.4]), 0.49, 16),
    'n255': lambda: _case('n255', 3, 255, _box('ortho', [9.0, 9.6, 10.4]), 0.3, 40),                  # 3 x 3 x 3 cells
    'n256': lambda: _case('n256', 4, 256, _box('skew', [9.5, 9.9, 10.4]), 0.3, 40),
    'n257': lambda: _case('n257', 5, 257, _box('ortho', [15.9, 9.3, 12.7]), 0.333, 40, n_types=3),    # 5 x 3 x 4 cells
    'n513': lambda: _case('n513', 6, 513, _box('skew', [11.0, 12.0, 13.0]), 0.45, 50, n_types=2, uncounted=0.2),
    'n513_unwrapped': lambda: _case('n513_unwrapped', 7, 513, _box('skew', [10.0, 9.0, 11.0]), 0.3, 50, unwrap=3),
    'water64': lambda: _water64('water64', 'ortho'),
    'water64_skew': lambda: _water64('water64_skew', 'skew'),
    'one_type': lambda: _case('one_type', 8, 300, _box('ortho', [9.0, 9.5, 10.0]), 0.4, 32, n_types=1, groups='triples'),
    'eight_types': lambda: _case('eight_types', 9, 300, _box('skew', [9.0, 9.5, 10.0]), 0.4, 32, n_types=8, uncounted=0.1),
    'raw_types': lambda: _case('raw_types', 10, 300, _box('ortho', [9.0, 9.5, 10.0]), 0.4, 32, n_types=3, raw_types=True),
    'one_group': lambda: _case('one_group', 11, 300, _box('ortho', [9.0, 9.5, 10.0]), 0.4, 32, groups='one'),
    # two cells along x and y at r_max = 0.499 of the smallest height (x); z has three
    'two_cells': lambda: _case('two_cells', 12, 400, _box('ortho', [8.0, 8.3, 13.0]), 0.499, 40),
    'two_cells_skew': lambda: _case('two_cells_skew', 13, 400, _box('skew', [8.0, 13.0, 8.4]), 0.499, 40, uncounted=0.1),
    'faces': lambda: _case('faces', 14, 300, _box('ortho', [9.0, 12.0, 15.0]), 0.3333, 40, faces=[3, 4, 5]),
    'cluster': lambda: _case('cluster', 15, 300, _box('ortho', [9.0, 9.0, 9.0]), 0.3, 40, cluster=[3, 3, 3]),   # 300 > one chunk
    'bins_1': lambda: _case('bins_1', 16, 257, _box('ortho', [9.0, 10.0, 11.0]), 0.3, 1),
    'bins_16384': lambda: _case('bins_16384', 17, 257, _box('ortho', [9.0, 10.0, 11.0]), 0.3, 16384, n_types=1, single=False),
    'bins_36x455': lambda: _case('bins_36x455', 18, 257, _box('ortho', [9.0, 10.0, 11.0]), 0.3, 455, n_types=8),
    'n4096': lambda: _case('n4096', 19, 4096, _box('ortho', [30.0, 31.0, 32.0]), 0.3, 100, groups='triples'),
    'n4097': lambda: _case('n4097', 20, 4097, _box('ortho', [30.0, 31.0, 32.0]), 0.3, 100, groups='triples'),
}
CASES = tuple(_MAKERS)
SMALL_CASES = tuple(k for k in CASES if k not in ('n4096', 'n4097'))      # what the host program walks pair by pair
# the grids the cell form must report for these cases (tests/test_rdf_cpu.py checks them against the plan)
GRIDS = {'n255': (3, 3, 3), 'n257': (5, 3, 4), 'two_cells': (2, 2, 3), 'two_cells_skew': (2, 3, 2), 'faces': (3, 4, 5),
         'cluster': (3, 3, 3), 'n4097': (3, 3, 3)}


@functools.lru_cache(maxsize=None)
def case(name):
    return _MAKERS[name]()


def held(c, prec):
    """the positions as a handle of that precision holds them, as float64"""
    return np.asarray(c['pos'], dtype=np.float32 if prec in ('f', 'single') else np.float64).astype(np.float64)


def scale(c, pos):
    """S of the acceptance rule"""
    return float(np.abs(pos).max() + np.abs(c['box']).sum(axis=1).max())


def delta(c, pos, prec):
    """delta of the acceptance rule for the host program ('f', 'd') or a GPU handle ('single': 4 x the measured ratio, 'double')"""
    rho_eps = {'d': DOUBLE_RATIO * EPS64, 'double': DOUBLE_RATIO * EPS64, 'f': SINGLE_RATIO * EPS32, 'single': 4.0 * SINGLE_RATIO * EPS32}
    return rho_eps[prec] * scale(c, pos)


_SHIFTS = np.array(list(itertools.product((-1, 0, 1), repeat=3)), dtype=np.float64)


def counted_pairs(c, pos=None, tags=None):
    """(i, j, r, channel) of every counted pair (i < j) with r below R = 1.001 r_max + 1e-3, by the rule of the module docstring"""
    pos = c['pos'] if pos is None else pos
    tags = c['tags'] if tags is None else np.asarray(tags)
    box, n, nt = c['box'], len(pos), c['n_types']
    inv, h = np.linalg.inv(box), heights(box)
    R = 1.001 * c['r_max'] + 1e-3
    ty, gr = tags.astype(np.int64) & 15, tags.astype(np.int64) >> 4
    T = _SHIFTS @ box
    out = []
    for i0 in range(0, n, 512):
        i = np.arange(i0, min(i0 + 512, n))
        d = pos[i][:, None, :] - pos[None, :, :]
        s = d @ inv
        n0 = np.rint(s)
        d0 = d - n0 @ box
        f = np.abs(s - n0)
        cand = (np.sqrt((d0 * d0).sum(axis=2)) < R) | (((1.0 - f) * h) < R).any(axis=2)
        cand &= (i[:, None] < np.arange(n)[None, :])
        cand &= (ty[i][:, None] < nt) & (ty[None, :] < nt) & (gr[i][:, None] != gr[None, :])
        a, b = np.nonzero(cand)
        if len(a) == 0:
            continue
        img = d0[a, b][:, None, :] - T[None, :, :]
        r = np.sqrt((img * img).sum(axis=2)).min(axis=1)
        keep = r < R
        ta, tb = ty[i[a[keep]]], ty[b[keep]]
        lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
        out.append((i[a[keep]], b[keep], r[keep], lo * nt - lo * (lo - 1) // 2 + (hi - lo)))
    if not out:
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros(0), z
    return tuple(np.concatenate(x) for x in zip(*out))


def reference(c, pos=None, tags=None):
    """per channel the sorted distances (below R) of the counted pairs"""
    _, _, r, ch = counted_pairs(c, pos, tags)
    return [np.sort(r[ch == k]) for k in range(c['n_types'] * (c['n_types'] + 1) // 2)]


def exact_histogram(c, ref):
    """the histogram of the reference distances in exact arithmetic: what a double result must equal when no pair lies within
    delta of an edge"""
    edges = np.arange(c['n_bins'] + 1) * (c['r_max'] / c['n_bins'])
    edges[-1] = c['r_max']
    return np.stack([np.diff(np.searchsorted(r, edges, side='left')) for r in ref]).astype(np.uint64)


def violations(c, ref, got, dlt):
    """the acceptance rule: the number of (channel, edge) pairs at which C_ref(e - delta) <= C_got <= C_ref(e + delta) fails"""
    got = np.asarray(got)
    assert got.shape == (len(ref), c['n_bins']), got.shape
    e = np.arange(1, c['n_bins'] + 1) * (c['r_max'] / c['n_bins'])
    bad = 0
    for r, row in zip(ref, got):
        cum = np.cumsum(row.astype(np.int64))
        lo, hi = np.searchsorted(r, e - dlt, side='left'), np.searchsorted(r, e + dlt, side='left')
        bad += int(((cum < lo) | (cum > hi)).sum())
    return bad


def near_edges(c, ref, dlt):
    """(pairs within delta of any edge k dr, k = 1 .. n_bins; counted pairs below r_max + delta; the smallest distance of a pair
    to an edge over delta)"""
    dr = c['r_max'] / c['n_bins']
    near, total, closest = 0, 0, np.inf
    for r in ref:
        r = r[r < c['r_max'] + dlt]
        k = np.clip(np.rint(r / dr), 1, c['n_bins'])
        gap = np.abs(r - k * dr)
        near += int((gap <= dlt).sum())
        total += len(r)
        if len(r):
            closest = min(closest, float(gap.min()) / dlt)
    return near, total, closest
