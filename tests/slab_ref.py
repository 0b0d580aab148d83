"""The decomposition of a slab rank (admp_amd/csrc/slab_kernels.hip, SlabDecomp::decompose) restated in plain numpy, float64, from
the RULE and not from the kernels, and the systems the list tests run on (tests/test_slab_ref_cpu.py checks this module on
the CPU, tests/test_gpu_slab_lists.py compares the device's arrays with it word by word).

The rule.
* Owner.  Atom i belongs to the slab [floor(s K0 / N), floor((s + 1) K0 / N)) that contains the lowest plane of its order-6
  stencil, (ceil(u_i) - 3) mod K0 with u_i = K0 * frac_x(r_i), frac = r . box^-1 (not wrapped: the mod does that).
* The table.  admp_set_pairs keeps the rows 0 <= i < j < Na of the list it is handed (the reference's own filter
  pairs[pairs[:, 0] < pairs[:, 1]]; rows the other way round, self pairs and padding are dropped) and a row of the table
  holds both directions of every pair kept.  pair_table() restates that; the CPU test pins it.
* What rank r reads: the partners of its home rows in that table, and the axis atoms of its home frames -- one for Zonly,
  two for ZThenX / Bisector, three for ZBisect / ThreeFold, none for NoAxisType.
* Imports of r from t: the atoms t owns and r reads.  Exports of r to t: r's atoms that t reads -- computed here from r's
  side alone, as a rank has to: through the symmetry of the table (t reads i if a row of t holds i, that is if row i holds
  an atom of t) and through the INVERSE frame map (the sites whose frame uses i).  That the two agree is the CPU test's
  first assertion.
* act: the polarizable (pol > 0) home atoms of a polarizable handle.  Migrants: from the owners of two consecutive
  evaluations.  Every list ascending (rows, the pair kernels' order of the home rows, is a permutation of home).
* bits, the word per atom: home atoms kHome | (kPolar) | export mask; atoms the rank reads without owning them
  1 << owner; every other atom 0.
"""
import math

import numpy as np

K_HOME, K_POLAR = 1 << 30, 1 << 29
ZTHENX, BISECTOR, ZBISECT, THREEFOLD, ZONLY, NOAXIS = 0, 1, 2, 3, 4, 5
N_AXIS_ATOMS = {ZTHENX: 2, BISECTOR: 2, ZBISECT: 3, THREEFOLD: 3, ZONLY: 1, NOAXIS: 0}
MARGIN = 1e-3                               # no atom closer than this to a plane, in u units (module docstring of the CPU test)
RC = 4.0


# ---- the rule --------------------------------------------------------------------------------------------------------------
def slab_edges(K0, N):
    return [(s * K0) // N for s in range(N + 1)]


def u_of(pos, box, K0):
    return K0 * (np.asarray(pos, dtype=np.float64) @ np.linalg.inv(np.asarray(box, dtype=np.float64)))[:, 0]


def plane_distance(pos, box, K0, shift=0.0):
    """distance of every atom from the nearest mesh plane along x, in u units (shift: all atoms moved by that many planes)"""
    u = u_of(pos, box, K0) + shift
    return np.abs(u - np.round(u))


def owners(pos, box, K0, N):
    base = np.mod(np.ceil(u_of(pos, box, K0)).astype(np.int64) - 3, K0)
    edges = np.array(slab_edges(K0, N))
    own = np.searchsorted(edges, base, side='right') - 1
    assert ((edges[own] <= base) & (base < edges[own + 1])).all()
    return own.astype(np.int64)


def pair_table(pairs, na):
    """[sorted partners of atom i]: both directions of the rows 0 <= i < j < na of the list"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    p = p[(p[:, 0] >= 0) & (p[:, 0] < p[:, 1]) & (p[:, 1] < na)]
    rows = [[] for _ in range(na)]
    for i, j in p:
        rows[i].append(int(j))
        rows[j].append(int(i))
    return [sorted(set(r)) for r in rows]


def axis_atoms(axis_type, axis_indices):
    out = []
    for t, idx in zip(np.asarray(axis_type), np.asarray(axis_indices)):
        out.append([int(a) for a in idx[:N_AXIS_ATOMS[int(t)]] if a >= 0])
    return out


def inverse_frames(axes):
    """inv[a] = the sites whose frame uses atom a as an axis atom"""
    inv = [[] for _ in axes]
    for i, ax in enumerate(axes):
        for a in ax:
            if i not in inv[a]:
                inv[a].append(i)
    return inv


def reads(r, owner, table, axes):
    """set of the atoms rank r reads without owning them"""
    out = set()
    for i in np.nonzero(owner == r)[0]:
        out.update(j for j in table[i] if owner[j] != r)
        out.update(a for a in axes[i] if owner[a] != r)
    return out


def decomposition(owner, table, axes, pol, lpol, N):
    """[per rank: dict(home, act, imports[t], exports[t], bits)] -- imports from the reader's side, exports from the owner's"""
    na = len(owner)
    inv = inverse_frames(axes)
    out = []
    for r in range(N):
        home = np.nonzero(owner == r)[0]
        rd = reads(r, owner, table, axes)
        imports = [sorted(j for j in rd if owner[j] == t) for t in range(N)]
        mask = np.zeros(na, dtype=np.int64)
        for i in home:
            for j in table[i]:                         # row j holds i as well: the owner of j reads i
                if owner[j] != r:
                    mask[i] |= 1 << int(owner[j])
            for s in inv[i]:                           # site s builds its frame from i
                if owner[s] != r:
                    mask[i] |= 1 << int(owner[s])
        exports = [[int(i) for i in home if (mask[i] >> t) & 1] if t != r else [] for t in range(N)]
        bits = np.zeros(na, dtype=np.int64)
        bits[home] = K_HOME | mask[home]
        if lpol:
            bits[home[np.asarray(pol)[home] > 0]] |= K_POLAR
        for j in rd:
            bits[j] = 1 << int(owner[j])
        act = [int(i) for i in home if lpol and pol[i] > 0]
        out.append(dict(home=[int(i) for i in home], act=act, imports=imports, exports=exports, bits=bits))
    return out


def migrants(owner_prev, owner_now, r, N):
    """(mig_in[t]: atoms r took over from t, mig_out[t]: atoms r gave to t), ascending"""
    mig_in = [[int(i) for i in np.nonzero((owner_now == r) & (owner_prev == t))[0]] if t != r else [] for t in range(N)]
    mig_out = [[int(i) for i in np.nonzero((owner_prev == r) & (owner_now == t))[0]] if t != r else [] for t in range(N)]
    return mig_in, mig_out


# ---- systems ---------------------------------------------------------------------------------------------------------------
def _clear_planes(pos, box, K0, shifts):
    """Atoms closer than 2 MARGIN to a plane (in any of the configurations `shifts`, in planes) are moved along x by a
    hundredth of a plane spacing until none is.  Seeds cannot do this at 4098 atoms: 8 of them lie within 1e-3 of a plane on
    average.  The spacing of a molecule changes by 0.003 A at most, which no list cares about."""
    pos = pos.copy()
    step = 0.01 * box[0, 0] / K0
    for _ in range(100):
        near = np.zeros(len(pos), dtype=bool)
        for s in shifts:
            near |= plane_distance(pos, box, K0, s) < 2 * MARGIN
        if not near.any():
            return pos
        pos[near, 0] += step
    raise RuntimeError('could not clear the planes')


def water_case(name, n_mol, seed, N, K0=48, frames='water', lpol=True, shift_planes=None, from_positions=False):
    """A water box with WRAPPED positions (molecules straddle the slab and cell faces), a hand-set mesh of K0 planes along x.
    frames = 'general': O takes a ZBisect frame, H1 a ThreeFold frame, both with a third axis atom in the molecule two lattice planes
    further along x (a frame across slabs, often across non-adjacent ones), H2 a Zonly frame.  pol > 0 on every site but a seeded third.
    shift_planes: a second configuration, every atom moved along x by that many plane spacings."""
    from admp_amd import systems as S
    pos, box = S.synthetic_water_box(n_mol, seed=seed)
    at, ai, cov = S.water_topology(n_mol)
    par = S.water_parameters(n_mol, polarizable=True)
    na = 3 * n_mol
    frac = pos @ np.linalg.inv(box)
    pos = (frac - np.floor(frac)) @ box
    pos = _clear_planes(pos, box, K0, (0.0,) if shift_planes is None else (0.0, shift_planes))
    if frames == 'general':
        at = at.copy()
        ai = ai.copy()
        o = 3 * np.arange(n_mol)
        g = int(math.ceil(n_mol ** (1.0 / 3.0) - 1e-9))      # (molecules are numbered along z, then y, then x of a g^3 lattice)
        nxt = 3 * ((np.arange(n_mol) + 2 * g * g) % n_mol)
        at[o], at[o + 1], at[o + 2] = ZBISECT, THREEFOLD, ZONLY
        ai[o, 2] = nxt
        ai[o + 1, 2] = nxt + 1
        ai[o + 2, 1] = -1
    rng = np.random.default_rng(1000 + seed)
    pol = np.where(np.arange(na) % 3 == 0, S.POL_O, 0.1)
    pol[rng.permutation(na)[:na // 3]] = 0.0
    par = dict(par, pol=pol, tholes=np.full(na, S.THOLE_O))
    c = dict(name=name, n_mol=n_mol, na=na, N=N, K0=K0, pos=pos, box=box, at=at, ai=ai, cov=cov, par=par, lpol=lpol, rc=RC,
             pairs=S.build_pairs(pos, box, RC), shift_planes=shift_planes, from_positions=from_positions, exact=False)
    if shift_planes is not None:
        c['pos2'] = pos + np.array([shift_planes * box[0, 0] / K0, 0.0, 0.0])
    return c


def exact_case(name, N):
    """An orthorhombic cell of 16 A with 32 planes along x: u = 2 x exactly in both types.  32 waters, molecule m with its O ON
    plane m (u = m: base m - 3, so a third of the slab faces is hit exactly), H1 on the next plane and H2 half way between;
    some molecules a whole cell outside (u < 0, u >= K0)."""
    from admp_amd import systems as S
    n_mol, K0 = 32, 32
    na = 3 * n_mol
    box = np.eye(3) * 16.0
    pos = np.zeros((na, 3))
    for m in range(n_mol):
        y0, z0 = 1.0 + 3.0 * (m % 5), 1.0 + 3.0 * ((m // 5) % 5)
        pos[3 * m] = [0.5 * m, y0, z0]
        pos[3 * m + 1] = [0.5 * m + 0.5, y0 + 0.75, z0 + 0.5]
        pos[3 * m + 2] = [0.5 * m + 0.25, y0 - 0.5, z0 + 0.75]
        if m % 7 == 3:
            pos[3 * m:3 * m + 3, 0] += 16.0 if m % 2 else -16.0
    at, ai, cov = S.water_topology(n_mol)
    par = S.water_parameters(n_mol, polarizable=True)
    pol = np.where(np.arange(na) % 3 == 0, S.POL_O, 0.1)
    pol[np.arange(na) % 5 == 2] = 0.0
    par = dict(par, pol=pol, tholes=np.full(na, S.THOLE_O))
    return dict(name=name, n_mol=n_mol, na=na, N=N, K0=K0, pos=pos, box=box, at=at, ai=ai, cov=cov, par=par, lpol=True, rc=RC,
                pairs=S.build_pairs(pos, box, RC), shift_planes=None, from_positions=False, exact=True)


# name -> builder.  192, 1026 and 4098 atoms cross the 64-lane chunk and the 1024-atom workgroup span of the compaction by two
# atoms; at N = 8 a slab is 6 planes of 48, thinner than the cutoff in the two smaller boxes (1.6 and 2.7 A against 4 A).
CASES = {}
for _n_mol, _tag, _seed in ((64, 'w64', 7), (342, 'w342', 11), (1366, 'w1366', 13)):
    for _N in (2, 3, 5, 8):
        CASES['%s_n%d' % (_tag, _N)] = (lambda n=_n_mol, s=_seed, N=_N, t=_tag: water_case('%s_n%d' % (t, N), n, s, N))
CASES['general_n5'] = lambda: water_case('general_n5', 64, 17, 5, frames='general')
CASES['general_n8'] = lambda: water_case('general_n8', 64, 19, 8, frames='general')
CASES['nopol_n3'] = lambda: water_case('nopol_n3', 64, 23, 3, lpol=False)
CASES['exact_n5'] = lambda: exact_case('exact_n5', 5)
CASES['exact_n2'] = lambda: exact_case('exact_n2', 2)
CASES['migrants_n3'] = lambda: water_case('migrants_n3', 342, 29, 3, shift_planes=1.5)
CASES['migrants_n8'] = lambda: water_case('migrants_n8', 342, 31, 8, shift_planes=1.5)
CASES['positions_n3'] = lambda: water_case('positions_n3', 64, 37, 3, from_positions=True)
GROUPS = {'w64': [k for k in CASES if k.startswith('w64_')], 'w342': [k for k in CASES if k.startswith('w342_')],
          'w1366': [k for k in CASES if k.startswith('w1366_')],
          'frames': ['general_n5', 'general_n8', 'nopol_n3'], 'exact': ['exact_n5', 'exact_n2'],
          'moves': ['migrants_n3', 'migrants_n8', 'positions_n3']}

_BUILT = {}


def case(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


_REF = {}


def reference(name):
    """dict(owner, ranks=[...], [owner2, ranks2, mig=[(mig_in, mig_out) per rank]]) of a case; computed once"""
    if name not in _REF:
        c = case(name)
        table = pair_table(c['pairs'], c['na'])
        axes = axis_atoms(c['at'], c['ai'])
        own = owners(c['pos'], c['box'], c['K0'], c['N'])
        ref = dict(owner=own, ranks=decomposition(own, table, axes, c['par']['pol'], c['lpol'], c['N']))
        if c['shift_planes'] is not None:
            own2 = owners(c['pos2'], c['box'], c['K0'], c['N'])
            ref['owner2'] = own2
            ref['ranks2'] = decomposition(own2, table, axes, c['par']['pol'], c['lpol'], c['N'])
            ref['mig'] = [migrants(own, own2, r, c['N']) for r in range(c['N'])]
        _REF[name] = ref
    return _REF[name]
