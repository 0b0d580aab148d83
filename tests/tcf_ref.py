"""Float64 reference of the time correlation functions (admp_md_tcf; admp_amd.md.CorrelationRecorder) and the cases the CPU and
GPU tests share.  The unwrap runs in np.longdouble; the sums are brute force over all (origin, lag) pairs.

The observable: d_i(0) = 0, d_i(f) = d_i(f - 1) + min_image(pos_i(f) - pos_i(f - 1)) in the cell of frame f; for every counted type
a and lag k = 0 .. L - 1

    MSD_sum[a][k]  = sum_{f >= k} sum_{i of type a} |d_i(f) - d_i(f - k)|^2
    VACF_sum[a][k] = sum_{f >= k} sum_{i of type a} v_i(f) . v_i(f - k)

with M[a][k] = N_a max(0, frames - k) terms each.  The reference removes the image as delta - n . box with the integers
n = round(delta . box^-1), so it does not depend on how well the inverse is known.  A large jump is a (frame >= 1, counted atom)
whose minimum image has a fractional component |s| >= 0.25.

The acceptance bar (u = 2^-53; nothing below is tuned to what the code gives)

  VACF.  A term is a dot product of values the ring holds unchanged: three products and two additions of doubles, each rounded
  once, are within 3 u A of the exact term, A = sum_c |v_c v'_c|.  Summing M such terms in ANY order (lanes, waves, tiles, the
  accumulation over the frames; zeros of padding add no rounding) adds at most (M - 1) u sum A to first order.  With room for the
  second-order terms and for the additions into a pre-filled accumulator the bar is (M + 16) u sum A: sum A is the module's
  `vacf_abs`, the condition number's numerator, not |sum|.
  MSD.  Given the d the ring holds, the same count applies to the squares ((M + 16) u sum |term|: three differences, three
  squares, two additions; the terms are positive, so sum A = the sum itself).  The d themselves carry an error e per component:
      e = (28 G + 3) frames u P  +  eps_ring D  [+ 2 eps_held P]
    * the accumulator: per frame and component the difference pos - last (one rounding, |delta| <= 2 P), three products and two
      additions for each fractional component with an inverse known to a few u (together <= 11 u |delta| G_s), the same count
      back to Cartesian (<= 3 u more on top of the propagated 11), and the addition into the accumulator (u D).  With G = max_c
      sum_j |h_jc| sum_k |hinv_kj| >= 1 (1 for an orthorhombic cell), the factor by which a relative error in the fractional
      components comes back, this is at most u (2 P 14 G + 2 P + D) <= (28 G + 3) u P per frame, P = the largest of |pos|,
      the cell's row sums and D = max |d|.
    * the ring: d rounded once to the handle's precision, eps_ring = 2^-24 for a single-precision handle (0 for double: the
      ring holds the accumulator itself).
    * only where a trajectory is compared with the reference of ANOTHER input (the wrapped trajectory against the unwrapped
      one's reference, the reference against an analytic value): the sum of the minimum images telescopes to pos(f) - pos(0) plus
      lattice vectors, so the two inputs' d differ by the rounding of two held positions, 2 eps_held P, eps_held = 2^-53 or 2^-24.
  A difference of two d is then off by at most 2 e per component, and a term |dd|^2 by at most 2 |dd|_1 2e + 3 (2e)^2.  Summed:
      bar_MSD = (M + 16) u sum |term| + 4 e sum |dd|_1 + 12 M e^2.
The GPU is held to the same bar: its arithmetic is the same double arithmetic, and contraction only removes roundings.
"""
import functools

import numpy as np

U = 2.0 ** -53
EPS32 = 2.0 ** -24
LAGS_PER_WORKGROUP = 16      # admp_amd/csrc/tcf_plan.h kTcfLagsPerWg


def heights(box):
    inv = np.linalg.inv(box)
    return 1.0 / np.sqrt((inv * inv).sum(axis=0))


SKEW = np.array([[11.0, 0.0, 0.0], [3.1, 12.0, 0.0], [-2.3, 4.1, 12.6]])


def _walk(name, seed, types, n_lags, frames, box=None, step=0.04, scale_per_frame=1.0, n_types=None):
    """a random walk: every frame every atom moves by up to `step` of the cell along each lattice direction; atoms are NOT
    wrapped, so they leave the cell.  Velocities are independent normal draws (0.01 A/fs: thermal)."""
    rng = np.random.default_rng(seed)
    types = np.asarray(types, dtype=np.int64)
    n = len(types)
    box = np.diag([10.0, 10.6, 11.2]) if box is None else np.asarray(box, dtype=np.float64)
    boxes = np.stack([box * scale_per_frame ** f for f in range(frames)])
    s = rng.random((n, 3))
    pos = np.zeros((frames, n, 3))
    for f in range(frames):
        if f:
            s = s + step * (2.0 * rng.random((n, 3)) - 1.0)
        pos[f] = s @ boxes[f]
    vel = 0.01 * rng.normal(size=(frames, n, 3))
    return dict(name=name, types=types, n_types=int(types.max()) + 1 if n_types is None else n_types, n_lags=n_lags, pos=pos, vel=vel,
                box=boxes, dt=2.0)


def _types_gap():
    """types {0, 2} of 0..2: one atom of type 0, 300 of type 2, 40 not counted (-1 and -3), interleaved so that the sort matters"""
    t = np.array([2] * 300 + [0] + [-1] * 25 + [-3] * 15, dtype=np.int64)
    return np.random.default_rng(11).permutation(t)


def _water(kind):
    """64 waters (O = 0, H = 1) in a skewed cell over 20 frames: whole molecules drift, so atoms cross faces; 'wrapped': the caller
    wraps every atom into the cell every frame; 'unwrapped': the same trajectory as it is"""
    rng = np.random.default_rng(640)
    frames, n_mol = 20, 64
    centre = rng.random((n_mol, 3)) @ SKEW
    arms = 0.96 * rng.normal(size=(n_mol, 2, 3)) / np.sqrt(3.0)
    drift = 0.03 * (2.0 * rng.random((n_mol, 3)) - 1.0)
    pos = np.zeros((frames, 3 * n_mol, 3))
    for f in range(frames):
        c = centre + (f * drift + 0.01 * rng.normal(size=(n_mol, 3))) @ SKEW
        pos[f, 0::3] = c
        pos[f, 1::3] = c + arms[:, 0] + 0.02 * rng.normal(size=(n_mol, 3))
        pos[f, 2::3] = c + arms[:, 1] + 0.02 * rng.normal(size=(n_mol, 3))
    crossings = 0
    if kind == 'wrapped':
        cells = np.floor(pos @ np.linalg.inv(SKEW))
        crossings = int((np.abs(np.diff(cells, axis=0)).sum(axis=2).sum(axis=0) > 0).sum())      # atoms that change cell at least once
        pos = pos - cells @ SKEW
    vel = 0.01 * rng.normal(size=(frames, 3 * n_mol, 3))
    return dict(name=kind + '_triclinic', types=np.tile([0, 1, 1], n_mol), n_types=2, n_lags=8, pos=pos, vel=vel,
                box=np.stack([SKEW] * frames), dt=2.0, crossings=crossings)


def _jumps():
    c = _walk('jumps', 77, np.zeros(50, dtype=np.int64), 6, 9, step=0.045)
    box = c['box'][0]
    big = np.zeros((50, 3))
    for i, (s, d) in enumerate([(0.3, 0), (0.4, 1), (-0.3, 2), (-0.4, 0), (0.3, 1)]):
        big[i, d] = s
    c['pos'][4:] += big @ box            # between frames 3 and 4, for good
    c['jumpers'] = 5
    return c


def _ballistic():
    rng = np.random.default_rng(5)
    n, frames, dt = 30, 12, 2.0
    box = np.diag([9.0, 9.0, 9.0])
    v = 0.15 * rng.normal(size=(n, 3))
    p0 = rng.random((n, 3)) @ box
    pos = np.stack([p0 + v * (f * dt) for f in range(frames)])
    return dict(name='ballistic', types=np.zeros(n, dtype=np.int64), n_types=1, n_lags=8, pos=pos, vel=np.stack([v] * frames),
                box=np.stack([box] * frames), dt=dt)


def _lags(L):
    """40 atoms of two types over 2 L + 3 frames; the tests stop at L - 1, L, L + 1 and 2 L + 3 frames: the ring not full, exactly
    full, wrapped once and wrapped twice"""
    c = _walk('lags_%d' % L, 100 + L, np.arange(40) % 2, L, 2 * L + 3, step=0.02)
    c['checkpoints'] = tuple(f for f in (L - 1, L, L + 1, 2 * L + 3) if f >= 1)
    return c


_MAKERS = {
    'n1': lambda: _walk('n1', 1, [0], 4, 6),
    'n255': lambda: _walk('n255', 2, np.zeros(255, dtype=np.int64), 5, 7),
    'n256': lambda: _walk('n256', 3, np.zeros(256, dtype=np.int64), 5, 7, box=SKEW),
    'n257': lambda: _walk('n257', 4, np.zeros(257, dtype=np.int64), 5, 7),
    'types_gap': lambda: _walk('types_gap', 5, _types_gap(), 6, 8, n_types=3),
    'lags_1': lambda: _lags(1),
    'lags_7': lambda: _lags(7),
    'lags_33': lambda: _lags(33),
    'lags_65': lambda: _lags(65),
    'wrapped_triclinic': lambda: _water('wrapped'),
    'unwrapped_triclinic': lambda: _water('unwrapped'),
    'npt': lambda: _walk('npt', 9, np.arange(90) % 3, 6, 10, box=SKEW, scale_per_frame=1.001),
    'jumps': _jumps,
    'ballistic': _ballistic,
}
CASES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _MAKERS[name]()
    assert len(c['types']) <= 700 and len(c['pos']) <= 140
    return c


def held(c, prec, frames=None):
    """(positions, velocities) of the first `frames` frames (None: all) as a handle of that precision holds them, as float64"""
    t = np.float32 if prec in ('f', 'single') else np.float64
    return np.asarray(c['pos'][:frames], dtype=t).astype(np.float64), np.asarray(c['vel'][:frames], dtype=t).astype(np.float64)


def checkpoints(c):
    """the frame counts at which the tests compare the sums with the reference"""
    return c.get('checkpoints', (len(c['pos']),))


def layout(types, tile_atoms):
    """restatement of admp_amd.md.tcf_layout: (slot_atom, tile_type)"""
    types = np.asarray(types)
    slot_atom, tile_type = [], []
    for a in range(max(int(types.max()) + 1, 1) if len(types) else 1):
        atoms = [i for i, t in enumerate(types) if t == a]
        while atoms:
            run, atoms = atoms[:tile_atoms], atoms[tile_atoms:]
            slot_atom += run + [-1] * (tile_atoms - len(run))
            tile_type.append(a)
    return np.array(slot_atom, dtype=np.int32), np.array(tile_type, dtype=np.int32)


def unwrap(pos, box):
    """(d as longdouble (frames, n, 3), large jumps counted per atom and frame as a bool array, the fractional minimum images)"""
    ld = np.longdouble
    frames, n, _ = pos.shape
    d = np.zeros((frames, n, 3), dtype=ld)
    jump = np.zeros((frames, n), dtype=bool)
    frac = np.zeros((frames, n, 3))
    for f in range(1, frames):
        delta = pos[f].astype(ld) - pos[f - 1].astype(ld)
        s = (pos[f] - pos[f - 1]) @ np.linalg.inv(box[f])
        nint = np.floor(s + 0.5)
        d[f] = d[f - 1] + (delta - nint.astype(ld) @ box[f].astype(ld))
        frac[f] = s - nint
        jump[f] = (np.abs(frac[f]) >= 0.25).any(axis=1)
    return d, jump, frac


def reference(c, pos, vel):
    """dict: msd, vacf (n_types, L) float64 sums; vacf_abs = sum of sum_c |v_c v'_c|; dd_abs = sum of |dd|_1; terms M; jumps (counted
    atoms only); d_max, p_scale, g_factor for the bar"""
    types, nt, L = c['types'], c['n_types'], c['n_lags']
    frames = len(pos)
    d, jump, _ = unwrap(pos, c['box'])
    d64 = d.astype(np.float64)
    out = {k: np.zeros((nt, L)) for k in ('msd', 'vacf', 'vacf_abs', 'dd_abs', 'terms')}
    counted = (types >= 0) & (types < nt)
    for a in range(nt):
        sel = types == a
        for k in range(min(L, frames)):
            dd = (d[k:, sel] - d[:frames - k, sel]).astype(np.float64) if k else np.zeros((frames, int(sel.sum()), 3))
            vv = vel[k:, sel] * vel[:frames - k, sel]
            out['msd'][a, k] = (dd * dd).sum()
            out['dd_abs'][a, k] = np.abs(dd).sum()
            out['vacf'][a, k] = vv.sum()
            out['vacf_abs'][a, k] = np.abs(vv).sum()
            out['terms'][a, k] = sel.sum() * (frames - k)
    out['jumps'] = int(jump[:, counted].sum())
    out['origins'] = np.maximum(0, frames - np.arange(L))
    out['d_max'] = float(np.abs(d64[:, counted]).max()) if counted.any() else 0.0
    hs = np.abs(c['box'])
    out['p_scale'] = max(float(np.abs(pos).max()), float(hs.sum(axis=2).max()), out['d_max'])
    out['g_factor'] = max(float((np.abs(np.linalg.inv(b)).sum(axis=0) @ np.abs(b)).max()) for b in c['box'])
    out['frames'] = frames
    return out


def bar(ref, prec, other_input=False):
    """the acceptance bar of the module docstring, (2, n_types, L): [0] MSD, [1] VACF"""
    single = prec in ('f', 'single')
    e = (28.0 * ref['g_factor'] + 3.0) * ref['frames'] * U * ref['p_scale'] + (EPS32 * ref['d_max'] if single else 0.0)
    if other_input:
        e += 2.0 * (EPS32 if single else U) * ref['p_scale']
    M = ref['terms']
    msd = (M + 16.0) * U * ref['msd'] + 4.0 * e * ref['dd_abs'] + 12.0 * M * e * e
    vacf = (M + 16.0) * U * ref['vacf_abs']
    return np.stack([msd, vacf])


def worst_ratio(ref, prec, msd, vacf, other_input=False):
    """max err / bar over every (quantity, type, lag); an entry whose bar is 0 must be exact (then the ratio is 0, else inf)"""
    b = bar(ref, prec, other_input)
    err = np.stack([np.abs(np.asarray(msd) - ref['msd']), np.abs(np.asarray(vacf) - ref['vacf'])])
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())
