"""Float64 reference and case builder for the real-space pair kernels (admp_amd/csrc/pair_kernels.hip: k_pair_full,
k_pair_field), used by tests/test_pair_ref_cpu.py (no GPU: the cases and the reference are proved sound there) and by
tests/test_gpu_pair_kernels.py (the kernels' raw rows through the C entry admp_pair_real).

Reference: oracle.admp_oracle.pme_real in float64 with positions, Q_global and U_harm as autograd leaves; Q_global and U_harm
are formed from Q_local / U the way energy_pme_parts forms them.  Outputs: E, grad = dE/dr at fixed global multipoles,
pot = dE/dQ_global, fld = dE/dU_harm, and S_E = sum |e_pair|, the scale of the energy error.

Cases: general sites, not water.  Three-site groups with bisector / Z-then-X frames (every site can carry all moments),
parameters drawn per site, explicit pair lists, covalent classes 1..5 on chosen pairs, mScales = [0, .2, .5, .8, 1],
pScales = [0, 0, 1, 1, 1] (non-bonded pairs read the last entry: the reference's index wrap).  Sizes by the workgroup
arithmetic of the kernels (256 lanes per workgroup, XCD remap in eighths): 3, 67, 577 atoms (3 / 5 / 10 / 19 / 37 / 73
workgroups at 1 .. 32 lanes per row: partial last workgroups, padded grids, and above 64 a wrap of the energy words) and
2309 atoms with short rows (10 workgroups at one lane per row).

Every case has a variant 'B' in which the charge-only sites were given higher moments: what a caller does who changes
parameters between two evaluations (the neighbour table's site classes are then stale, and recompiled one call later)."""
import contextlib
import ctypes
import functools

import numpy as np
import torch

from oracle import admp_oracle as O
from tests.hostshim_util import lib, dp, c64, i32, scale_tables

F64 = torch.float64
MSCALES = np.array([0.0, 0.2, 0.5, 0.8, 1.0])
PSCALES = np.array([0.0, 0.0, 1.0, 1.0, 1.0])
KAPPA = 0.41
LROW = 32                       # the widest row split; its boundaries contain those of 1 .. 16 lanes
RC_LIST, RC_SHORT, SKIN = 6.0, 3.2, 1.0
FLOOR_FACTOR = 8.0              # single precision: the device may be this many host-f32 floors away from the reference


def T(x):
    return torch.as_tensor(np.array(x, dtype=np.float64))      # (a copy: the cases' arrays are read-only)


def oracle_pair(pos, box, pairs, nbonds_dense, Qg, Uh, pol, thole, mS, pS, kappa, lpol):
    """E and (dE/dpos, dE/dQ_global[, dE/dU_harm]) of the listed pairs: oracle.admp_oracle.pme_real under autograd"""
    p = T(pos).requires_grad_(True)
    q = T(Qg).requires_grad_(True)
    u = T(Uh).requires_grad_(True)
    e = O.pme_real(p, T(box), pairs, q, u if lpol else None, T(pol) if lpol else None,
                   T(thole) if lpol else None, T(mS), T(pS) if lpol else None, nbonds_dense, kappa, 2, lpol)
    gs = torch.autograd.grad(e, [p, q] + ([u] if lpol else []))
    return float(e.detach()), [g.numpy() for g in gs]


# ---- topology and geometry -----------------------------------------------------------------------------------------------------
def topology(n):
    """groups of three consecutive atoms: bisector frame on the first, Z-then-X on the other two; atoms left over take a
    Z-then-X frame on the two atoms before them"""
    at = np.zeros(n, dtype=np.int32)
    ai = -np.ones((n, 3), dtype=np.int32)
    for a in range(0, n - n % 3, 3):
        at[a] = 1
        ai[a] = [a + 1, a + 2, -1]
        ai[a + 1] = [a, a + 2, -1]
        ai[a + 2] = [a, a + 1, -1]
    for i in range(n - n % 3, n):
        ai[i] = [i - 1, i - 2, -1]
    return at, ai


TILT = np.array([[1.0, 0, 0], [0.09, 0.97, 0], [-0.06, 0.07, 1.04]])


def lattice(rng, n, spacing, tric, jitter=0.45):
    """n atoms on distinct sites of a g^3 grid of the cell (shuffled), jittered; a tenth of them moved out of the cell by
    whole lattice vectors"""
    g = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    box = np.eye(3) * (g * spacing)
    if tric:
        box = TILT * (g * spacing)
    sites = rng.permutation(g ** 3)[:n]
    f = (np.stack([sites // (g * g), (sites // g) % g, sites % g], axis=1) + 0.5) / float(g)
    pos = f @ box + rng.uniform(-jitter, jitter, (n, 3))
    out = rng.random(n) < 0.1
    pos[out] += rng.integers(-1, 2, (int(out.sum()), 3)) @ box
    return pos, box


def distances(pos, box, pairs):
    """minimum-image distances the way the kernels and the oracle take them (rounded fractional coordinates)"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    d = pos[pairs[:, 0]] - pos[pairs[:, 1]]
    s = d @ np.linalg.inv(box)
    d = d - np.floor(s + 0.5) @ box
    return np.sqrt((d * d).sum(1))


def pairs_within(pos, box, rc):
    i, j = np.triu_indices(len(pos), 1)
    allp = np.stack([i, j], axis=1)
    return allp[distances(pos, box, allp) < rc].astype(np.int32)


def random_classes(rng, n, pairs, frac=0.15):
    cov = np.zeros((n, n), dtype=np.int32)
    sel = pairs[rng.random(len(pairs)) < frac]
    cls = rng.integers(1, 6, len(sel))
    cov[sel[:, 0], sel[:, 1]] = cls
    cov[sel[:, 1], sel[:, 0]] = cls
    return cov


def draw_sites(rng, n):
    Q = rng.normal(size=(n, 9)) * np.array([1, .5, .5, .5, .3, .3, .3, .3, .3])
    pol = rng.uniform(0.3, 1.5, n)
    thole = rng.uniform(0.2, 9.0, n)
    U = rng.normal(size=(n, 3)) * 0.1
    return Q, pol, thole, U


def make_mono(c, mask):
    """charge-only sites: a charge and nothing else (no moments, not polarizable, no dipole)"""
    mask = np.asarray(mask, dtype=bool)
    c['Q_local'][mask, 1:] = 0.0
    c['pol'][mask] = 0.0
    c['thole'][mask] = 0.0
    c['U'][mask] = 0.0


def finish(c, rng):
    """common tail: dipoles only where there is a polarizability, variant B, read-only arrays"""
    n = c['n']
    c.setdefault('kappa', KAPPA)
    c.setdefault('lpol', True)
    c.setdefault('cutoff', 0.0)
    c['U'][c['pol'] == 0.0] = 0.0
    if not c['lpol']:
        c['pol'][:] = 0.0
        c['thole'][:] = 0.0
        c['U'][:] = 0.0
    c['axis_type'], c['axis_indices'] = topology(n)
    c['mono'] = mono_mask(c['Q_local'], c['pol'], c['U'])
    QB = c['Q_local'].copy()
    QB[c['mono'], 1:] = (rng.normal(size=(n, 8)) * 0.3)[c['mono']]
    c['Q_local_B'] = QB
    c['pairs'] = np.ascontiguousarray(c['pairs'], dtype=np.int32)
    paired = np.zeros(n, dtype=bool)
    paired[c['pairs'].reshape(-1)] = True
    c['isolated'] = np.nonzero(~paired)[0]
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def mono_mask(Q_local, pol, U):
    return (np.abs(Q_local[:, 1:]).max(1) == 0) & (pol == 0) & (np.abs(U).max(1) == 0)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _case_na3(rng):
    box = np.array([[12.0, 0, 0], [1.0, 11.5, 0], [-0.7, 0.9, 12.5]])
    pos = np.array([[1.0, 1.2, 0.8], [1.9, 1.4, 1.1], [0.7, 2.1, 1.3]]) + box[0]      # all three outside the cell
    Q, pol, thole, U = draw_sites(rng, 3)
    c = dict(n=3, pos=pos, box=box, Q_local=Q, pol=pol, thole=thole, U=U,
             pairs=np.array([[0, 1], [0, 2], [1, 2]]))
    cov = np.zeros((3, 3), dtype=np.int32)
    cov[0, 1] = cov[1, 0] = cov[0, 2] = cov[2, 0] = 1
    cov[1, 2] = cov[2, 1] = 2
    c['cov'] = cov
    make_mono(c, [False, True, False])
    c['pol'][2] = 0.0                                  # not polarizable, but a dipole and a quadrupole: not charge-only
    return c


ROW_SHAPES = ([(0, 0), (1, 0), (0, 1)] +
              [s for t in (LROW - 1, LROW, LROW + 1, 2 * LROW + 1, 3 * LROW) for s in ((t, 0), (0, t))] +
              [(1, LROW - 2), (1, LROW - 1), (LROW, 1), (LROW + 1, LROW), (LROW, LROW + 1), (LROW, 2 * LROW), (LROW + 1, 2 * LROW - 1)])
N_ROW_ATOMS = 2 * len(ROW_SHAPES)


def _case_rows67(rng):
    """Rows of prescribed shape in one hand-made list.  Atom 2 s is a fully equipped site and atom 2 s + 1 a charge-only site
    whose row has ROW_SHAPES[s] = (full-moment partners, charge-only partners); the partners come from a pool of 14 fully
    equipped and 13 charge-only atoms (the other 27 of the 67), taken in turn -- rows longer than the pool list its atoms
    more than once, which the list compiler and the reference both count as often as listed.  Totals 0, 1, L-1, L, L+1,
    2L+1 and 3L for L = 32, each with full-moment partners only, charge-only partners only, and both (full-moment runs of 0,
    1, L and L+1)."""
    n = 67
    pos, box = lattice(rng, n, 2.2, False, jitter=0.3)
    Q, pol, thole, U = draw_sites(rng, n)
    c = dict(n=n, pos=pos, box=box, Q_local=Q, pol=pol, thole=thole, U=U)
    full_pool = np.arange(N_ROW_ATOMS, N_ROW_ATOMS + 14)
    mono_pool = np.arange(N_ROW_ATOMS + 14, n)
    mono = np.zeros(n, dtype=bool)
    mono[1:N_ROW_ATOMS:2] = True
    mono[mono_pool] = True
    rows = []
    for s, (nf, nm) in enumerate(ROW_SHAPES):
        for i in (2 * s, 2 * s + 1):
            rows += [(i, full_pool[(t + i) % len(full_pool)]) for t in range(nf)]
            rows += [(i, mono_pool[(t + i) % len(mono_pool)]) for t in range(nm)]
    c['pairs'] = np.array(rows, dtype=np.int32)[rng.permutation(len(rows))]
    c['cov'] = random_classes(rng, n, np.unique(c['pairs'], axis=0), 0.2)
    make_mono(c, mono)
    c['shapes'] = np.array(ROW_SHAPES)
    return c


def _general(rng, n, rc, tric, lonely=True):
    pos, box = lattice(rng, n, 2.6, tric)
    pairs = pairs_within(pos, box, rc)
    if lonely:                                         # one atom without partners
        pairs = pairs[(pairs != n // 2).all(1)]
    pairs = pairs[rng.permutation(len(pairs))]
    Q, pol, thole, U = draw_sites(rng, n)
    return dict(n=n, pos=pos, box=box, Q_local=Q, pol=pol, thole=thole, U=U, pairs=pairs,
                cov=random_classes(rng, n, pairs))


def _mix(kind, tric):
    def build(rng):
        n = 577
        c = _general(rng, n, RC_LIST, tric)
        idx = np.arange(n)
        if kind == 'nomono':
            pass
        elif kind == 'allmono_nopol':
            c['lpol'] = False
            make_mono(c, np.ones(n, dtype=bool))
        elif kind == 'allmono_lpol':
            make_mono(c, np.ones(n, dtype=bool))
        elif kind == 'third':                            # the water ratio: one fully equipped site in three
            make_mono(c, idx % 3 != 0)
        elif kind == 'onefull':
            make_mono(c, idx != 100)
        elif kind == 'onemono':
            make_mono(c, idx == 100)
        elif kind == 'params':
            # pol = 0 with a dipole (not charge-only, dmp at its floor); pol > 0 without higher moments; thole = 0 on
            # single sites and on runs of neighbours (both sites of their pairs); pol down to 1e-3; a third charge-only
            make_mono(c, idx % 3 == 1)
            sel = rng.permutation(np.nonzero(idx % 3 != 1)[0])
            c['pol'][sel[:60]] = 0.0
            c['Q_local'][sel[60:120], 1:] = 0.0
            c['thole'][sel[120:150]] = 0.0
            near = np.argsort(distances(c['pos'], c['box'], np.stack([np.full(n, sel[150]), idx], 1)))[:25]
            c['thole'][near[idx[near] % 3 != 1]] = 0.0
            c['pol'][sel[180:240]] = 10.0 ** rng.uniform(-3.0, -0.5, 60)
        elif kind == 'nopol_third':                      # non-polarizable handle, one fully equipped site in three
            c['lpol'] = False
            make_mono(c, idx % 3 != 0)
        else:
            raise KeyError(kind)
        return c
    return build


def _case_cut(rng):
    """a Verlet list with a skin, evaluated with admp_set_cutoff: the reference takes the listed pairs below the cutoff"""
    for _ in range(20):
        c = _general(rng, 577, RC_LIST + SKIN, True)
        if np.abs(distances(c['pos'], c['box'], c['pairs']) - RC_LIST).min() > 1e-5:
            break
    else:
        raise RuntimeError('no geometry keeps the listed pairs 1e-5 A away from the cutoff')
    c['cutoff'] = RC_LIST
    make_mono(c, np.arange(577) % 3 != 0)
    return c


def _case_short(rng):
    c = _general(rng, 2309, RC_SHORT, False)
    make_mono(c, np.arange(2309) % 3 != 0)
    return c


def _dimers(rng, n_groups, spacing=7.0):
    """groups of three on a coarse grid (so that nothing but the listed pairs is close), water-like inside"""
    n = 3 * n_groups + 1
    g = int(np.ceil((n_groups + 1) ** (1.0 / 3.0) - 1e-9))
    box = np.eye(3) * (g * spacing)
    sites = rng.permutation(g ** 3)[:n_groups + 1]
    org = (np.stack([sites // (g * g), (sites // g) % g, sites % g], axis=1) + 0.5) * spacing
    pos = np.zeros((n, 3))
    for k in range(n_groups):
        pos[3 * k] = org[k]
        pos[3 * k + 1] = org[k] + [0.96, 0.0, 0.0]
        pos[3 * k + 2] = org[k] + 0.96 * np.array([np.cos(1.82), np.sin(1.82), 0.0])
    pos[n - 1] = org[n_groups]
    return n, pos, box


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _edge(kind):
    """pairs at prescribed separations, nothing else listed but the pairs inside the groups.
    short: 0.7, 0.96 and 1.5 A on classes with mscale 0 and 0.5 (the (m - 1) + B_n branch of the kernels).
    far:   kappa r = 2.9, 3.3 and 3.7 (3.7: what a skin list gives without a cutoff).
    thole: a_w r / dmp = 0.1, 5, 49 and 51 (the two sides of the `< 50` branch), and dmp at its floor (pol = 0 on one site)."""
    def build(rng):
        n, pos, box = _dimers(rng, 22)
        Q, pol, thole, U = draw_sites(rng, n)
        cov = np.zeros((n, n), dtype=np.int32)
        pairs, want = [], []

        def place(j, i, r, cls):
            """atom j (with its group) at distance r from atom i"""
            shift = pos[i] + r * _unit(rng) - pos[j]
            gj = 3 * (j // 3)
            pos[gj:gj + 3] += shift
            pairs.append((min(i, j), max(i, j)))
            cov[i, j] = cov[j, i] = cls
            want.append(r)

        if kind == 'short':
            k = 0
            for cls in (1, 3):
                for r in (0.7, 0.96, 1.5):
                    place(6 * k + 3, 6 * k, r, cls)
                    k += 1
        elif kind == 'far':
            for k, x in enumerate((2.9, 3.3, 3.7, 2.9, 3.3, 3.7)):
                place(6 * k + 3, 6 * k, x / KAPPA, 0 if k < 3 else 4)
        else:
            k = 0
            for au in (0.1, 5.0, 49.0, 51.0):
                for cls in (0, 3):                     # pscale 1 on both: a_w = thole_i + thole_j
                    i, j = 6 * k, 6 * k + 3
                    pol[i] = pol[j] = 1.0
                    thole[i] = thole[j] = au / 3.0 / 2.0
                    place(j, i, 3.0, cls)
                    k += 1
            i, j = 6 * k, 6 * k + 3                    # pscale 0: the default width 0.3, a_w r / dmp = 5
            pol[i] = pol[j] = (0.3 * 3.0 / 5.0) ** 3
            place(j, i, 3.0, 1)
            k += 1
            i, j = 6 * k, 6 * k + 3                    # dmp = (pol_i pol_j)^(1/6) at its floor
            pol[j] = 0.0
            place(j, i, 3.0, 0)
        if kind != 'thole':                            # the pairs inside the groups, water-like classes
            for a in range(0, n - 1, 3):
                for (x, y, cls) in ((a, a + 1, 1), (a, a + 2, 1), (a + 1, a + 2, 2)):
                    pairs.append((x, y))
                    cov[x, y] = cov[y, x] = cls
        c = dict(n=n, pos=pos, box=box, Q_local=Q, pol=pol, thole=thole, U=U, pairs=np.array(pairs), cov=cov)
        c['placed'] = np.array(pairs[:len(want)])
        c['placed_r'] = np.array(want)
        mono = np.zeros(n, dtype=bool)
        if kind != 'thole':
            mono[np.arange(n) % 3 == 2] = True         # never one of the placed atoms (those are first in their groups)
        make_mono(c, mono)
        return c
    return build


BUILDERS = {
    'na3': _case_na3, 'rows67': _case_rows67,
    'edge_short': _edge('short'), 'edge_far': _edge('far'), 'edge_thole': _edge('thole'),
    'nomono': _mix('nomono', True), 'allmono_nopol': _mix('allmono_nopol', False), 'allmono_lpol': _mix('allmono_lpol', True),
    'third': _mix('third', False), 'onefull': _mix('onefull', True), 'onemono': _mix('onemono', False),
    'params': _mix('params', True), 'nopol_third': _mix('nopol_third', True),
    'cut': _case_cut, 'short2309': _case_short,
}
CASES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(7100 + 17 * CASES.index(name))
    c = BUILDERS[name](rng)
    c['name'] = name
    return finish(c, rng)


def listed_pairs(c):
    """the pairs an evaluation walks: the list, or with a cutoff its rows below it"""
    if not c['cutoff']:
        return c['pairs']
    return c['pairs'][distances(c['pos'], c['box'], c['pairs']) < c['cutoff']]


# ---- reference -------------------------------------------------------------------------------------------------------------------
def global_moments(c, variant='A'):
    """Q_global and U_harm from Q_local and U, as oracle.admp_oracle.energy_pme_parts forms them"""
    Ql = c['Q_local_B'] if variant == 'B' else c['Q_local']
    frames = O.construct_local_frames(T(c['pos']), T(c['box']), c['axis_type'], c['axis_indices'])
    Qg = O.rot_local2global(T(Ql), frames, 2).numpy()
    Uh = (T(c['U']) @ O._C1_C2H.T).numpy()
    return Qg, Uh


def pair_energy_scale(c, pairs, Qg, Uh):
    """S_E = sum over the pairs of |e_pair| (pme_real_pair_energies on the rows of _pme_real_rows)"""
    pairs = np.asarray(pairs, dtype=np.int64)
    if len(pairs) == 0:
        return 0.0
    with torch.no_grad():
        pos, box = T(c['pos']), T(c['box'])
        nb = O.pair_nbonds(c['cov'], pairs)
        pi, pj = torch.as_tensor(pairs[:, 0]), torch.as_tensor(pairs[:, 1])
        r1, r2 = pos[pi], pos[pj]
        dr = O.pbc_shift(r1 - r2, box, torch.linalg.inv(box))
        norm = torch.linalg.norm(dr, dim=-1)
        Ri = O.build_quasi_internal(r1, r2, dr, norm)
        q = T(Qg)
        QI, QJ = O.rot_global2local(q[pi], Ri, 2), O.rot_global2local(q[pj], Ri, 2)
        m = O._scale_lookup(T(MSCALES), nb)
        if c['lpol']:
            u, pol, th = T(Uh), T(c['pol']), T(c['thole'])
            e = O.pme_real_pair_energies(norm, QI, QJ, O.rot_ind_global2local(u[pi], Ri), O.rot_ind_global2local(u[pj], Ri),
                                         th[pi], th[pj], (pol[pi] * pol[pj]) ** (1.0 / 6.0), m,
                                         O._scale_lookup(T(PSCALES), nb), c['kappa'], 2, True)
        else:
            e = O.pme_real_pair_energies(norm, QI, QJ, None, None, None, None, None, m, None, c['kappa'], 2, False)
    return e.abs().numpy()


def reference_on(c, pairs, variant='A', cov=None):
    Qg, Uh = global_moments(c, variant)
    cov = c['cov'] if cov is None else cov
    n = c['n']
    if len(pairs) == 0:
        return dict(E=0.0, grad=np.zeros((n, 3)), pot=np.zeros((n, 9)), fld=np.zeros((n, 3)), S_E=0.0, e_abs=np.zeros(0))
    E, g = oracle_pair(c['pos'], c['box'], np.asarray(pairs, dtype=np.int64), cov, Qg, Uh, c['pol'], c['thole'], MSCALES,
                       PSCALES, c['kappa'], c['lpol'])
    e_abs = pair_energy_scale(dict(c, cov=cov), pairs, Qg, Uh)
    return dict(E=E, grad=g[0], pot=g[1], fld=g[2] if c['lpol'] else np.zeros((n, 3)), S_E=float(e_abs.sum()), e_abs=e_abs)


@functools.lru_cache(maxsize=None)
def reference(name, variant='A'):
    c = case(name)
    return reference_on(c, listed_pairs(c), variant)


# ---- host shim (the kernels' per-pair functions compiled for the host) -------------------------------------------------------------
def shim(c, variant, prec, mode, pairs=None, moments=None):
    """shim_pair_real on the case: prec 8 / 4, mode 0 (half list), 1 (both ends, what the kernels do), 2 (with the charge-only
    dispatch).  mode 3: shim_pair_field with the charge-only partners' short form (fld only).  moments: (Q_global, U_harm)
    in place of the variant's."""
    Qg, Uh = global_moments(c, variant) if moments is None else moments
    pairs = i32(listed_pairs(c) if pairs is None else pairs)
    n = c['n']
    nb = i32(c['cov'][pairs[:, 0], pairs[:, 1]]) if len(pairs) else i32(np.zeros(0))
    mtab, ptab, w0 = scale_tables(MSCALES, PSCALES)
    grad, pot, fld = np.zeros((n, 3)), np.zeros((n, 9)), np.zeros((n, 3))
    p6 = c64(c['pol'] ** (1.0 / 6.0))
    args = (prec, n, dp(c64(c['pos'])), dp(c64(Qg)), dp(c64(Uh)), dp(p6), dp(c64(c['thole'])), dp(c64(c['box'])),
            ctypes.c_long(len(pairs)), dp(pairs), dp(nb))
    if mode == 3:
        lib().shim_pair_field_mono(*args, dp(ptab), dp(w0), ctypes.c_double(c['kappa']), dp(fld))
        return dict(fld=fld)
    e = lib().shim_pair_real(*args, dp(mtab), dp(ptab), dp(w0), ctypes.c_double(c['kappa']), int(c['lpol']), mode,
                             dp(grad), dp(pot), dp(fld))
    return dict(E=e, grad=grad, pot=pot, fld=fld)


def errors(got, ref, rows=None):
    """err(X) = max |X - ref| / max |ref| for grad, pot, fld (over `rows[X]` where given, relative to the whole array's
    largest entry) and |E - E_ref| / S_E; an output that `got` does not have is left out"""
    out = {}
    if got.get('E') is not None:
        out['E'] = abs(got['E'] - ref['E']) / ref['S_E'] if ref['S_E'] > 0 else abs(got['E'] - ref['E'])
    for k in ('grad', 'pot', 'fld'):
        if got.get(k) is None:
            continue
        a, b = np.asarray(got[k], dtype=np.float64), ref[k]
        if rows is not None and k in rows:
            a, b = a[rows[k]], b[rows[k]]
        scale = np.abs(ref[k]).max()
        d = np.abs(a - b).max() if a.size else 0.0
        out[k] = d / scale if scale > 0 else d
    return out


@functools.lru_cache(maxsize=None)
def floors(name, variant='A'):
    """what f32 storage and summation cost with exact library functions: errors() of the host shim at prec 4 (mode 1, the
    kernels' general arithmetic) against the float64 reference"""
    c = case(name)
    return errors(shim(c, variant, 4, 1), reference(name, variant))


# ---- the increment of the SCF field (k_pair_field_ind): fld_i = sum over the polarizable partners of T_ij dU_j -------------------
def jacobi_field(c):
    """the total field F of a Jacobi step whose dU = -pol F / DIELECTRIC is about 0.01 per component on the polarizable sites"""
    rng = np.random.default_rng(900 + c['n'] + len(c['pairs']))
    act = c['pol'] > 0
    F = np.zeros((c['n'], 3))
    F[act] = -(rng.normal(size=(c['n'], 3)) * 0.01)[act] * O.DIELECTRIC / c['pol'][act, None]
    return F


def jacobi_step(c, F, prec):
    """dU bit for bit as k_jacobi_delta forms it in the handle's type: s = -pol * T(1 / DIELECTRIC), dU = F * s (two products
    of rounded operands: nothing an FMA could contract)"""
    t = np.float64 if prec == 'double' else np.float32
    s = (-c['pol'].astype(t)) * t(1.0 / O.DIELECTRIC)
    return (F.astype(t) * s[:, None]).astype(np.float64)


def _ind_moments(c, prec):
    dU = jacobi_step(c, jacobi_field(c), prec)
    return np.zeros((c['n'], 9)), (T(dU) @ O._C1_C2H.T).numpy()


@functools.lru_cache(maxsize=None)
def reference_ind(name, prec):
    """the oracle at Q = 0 and U = dU: E = sum over the pairs of dU_i T_ij dU_j, so dE/dU_i is the increment, without a
    difference of two fields; rows of sites that are not polarizable are not the kernel's: zero"""
    c = case(name)
    Qg, Uh = _ind_moments(c, prec)
    pairs = np.asarray(listed_pairs(c), dtype=np.int64)
    E, g = oracle_pair(c['pos'], c['box'], pairs, c['cov'], Qg, Uh, c['pol'], c['thole'], MSCALES, PSCALES, c['kappa'], True)
    fld = np.where((c['pol'] > 0)[:, None], g[2], 0.0)
    return dict(E=E, fld=fld, S_E=abs(E))


@functools.lru_cache(maxsize=None)
def floors_ind(name, prec='single'):
    c = case(name)
    got = shim(c, 'A', 4, 1, moments=_ind_moments(c, prec))
    return errors({'fld': got['fld']}, reference_ind(name, prec), {'fld': c['pol'] > 0})


def double_bars(ref):
    """the bars of the host test of the same functions (tests/test_kernel_math_cpu.py): energy 1e-10 max(1, |E|); arrays rtol
    1e-9 with atol 1e-8 (grad) or 1e-9 (pot, fld) times the array's largest entry"""
    return dict(E=1e-10 * max(1.0, abs(ref['E'])), rtol=1e-9,
                atol={k: f * np.abs(ref[k]).max() for k, f in (('grad', 1e-8), ('pot', 1e-9), ('fld', 1e-9)) if k in ref})


def double_excess(got, ref, rows=None):
    """per output, the largest |got - ref| / (atol + rtol |ref|) (energy: / its bar): <= 1 passes the double bars"""
    bars = double_bars(ref)
    out = {}
    if got.get('E') is not None:
        out['E'] = abs(got['E'] - ref['E']) / bars['E']
    for k in ('grad', 'pot', 'fld'):
        if got.get(k) is None:
            continue
        a, b = np.asarray(got[k], dtype=np.float64), ref[k]
        if rows is not None and k in rows:
            a, b = a[rows[k]], b[rows[k]]
        tol = bars['atol'][k] + bars['rtol'] * np.abs(b)
        if not a.size:
            out[k] = 0.0
        elif (tol > 0).all():
            out[k] = float((np.abs(a - b) / tol).max())
        else:
            out[k] = 0.0 if np.array_equal(a, b) else np.inf
    return out


# ---- what a subtly wrong kernel would give ---------------------------------------------------------------------------------------
@contextlib.contextmanager
def erfc_off(rel):
    """the oracle forms erfc as 1 - erf (its b[1] = -erf): erfc (1 + rel) = 1 - (erf - rel (1 - erf))"""
    real = torch.erf
    torch.erf = lambda x: real(x) - rel * (1.0 - real(x))
    try:
        yield
    finally:
        torch.erf = real


def table_rows(c):
    """{atom: partners in the order of its row}: the listed pairs from both ends, charge-only partners behind the others"""
    pairs = listed_pairs(c)
    rows = {}
    for a, b in pairs:
        rows.setdefault(int(a), []).append(int(b))
        rows.setdefault(int(b), []).append(int(a))
    return {i: sorted(p, key=lambda j: (bool(c['mono'][j]), j)) for i, p in rows.items()}


def perturbed(name, what):
    """the reference of a wrong evaluation: 'pair' one pair missing (the one of median |e_pair|), 'class' that pair in another
    covalent class, 'last' the last partner of that pair's first atom missing from its row (a one-sided loss: the partner's
    own row is whole), 'erfc' erfc off by a relative 1e-6"""
    c, ref = case(name), reference(name)
    pairs = listed_pairs(c)
    k = int(np.argsort(ref['e_abs'])[len(pairs) // 2])
    if what == 'pair':
        return reference_on(c, np.delete(pairs, k, axis=0))
    if what == 'class':
        i, j = pairs[k]
        cov = c['cov'].copy()
        cov[i, j] = cov[j, i] = cov[i, j] % 5 + 1
        return reference_on(c, pairs, cov=cov)
    if what == 'last':
        i = int(pairs[k][0])
        j = table_rows(c)[i][-1]
        hit = np.nonzero(((pairs[:, 0] == i) & (pairs[:, 1] == j)) | ((pairs[:, 0] == j) & (pairs[:, 1] == i)))[0][-1]
        less = reference_on(c, np.delete(pairs, hit, axis=0))
        out = {key: np.array(v) if isinstance(v, np.ndarray) else v for key, v in ref.items()}
        for key in ('grad', 'pot', 'fld'):
            out[key][i] = less[key][i]
        out['E'] = 0.5 * (ref['E'] + less['E'])
        return out
    if what == 'erfc':
        with erfc_off(1e-6):
            return reference_on(c, pairs)
    raise KeyError(what)
