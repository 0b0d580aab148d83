"""Float64 reference and case builder for the first and the last stage of an evaluation: the site table (k_prepare_sites,
atom_kernels.hip) and the closing kernels (k_finish_pull<4>, k_finish_pull<1>, k_finish_groups, k_finish_rows, the closing
epilogue of k_gather_staged<.., FIN> in recip_kernels.hip, k_frame_virial).  Used by tests/test_site_ref_cpu.py (no GPU: cases,
reference, floors and expected launch forms are proved sound there) and by tests/test_gpu_site_close.py (the kernels alone
through the C entries admp_site_table / admp_site_close).

Reference, in float64 through oracle.admp_oracle and torch autograd:

    site table   Qg = rot_local2global(Q_local, construct_local_frames(pos, box, at, ai)), U in harmonic order (z, x, y),
                 p6 = pol^(1/6), charge-only mark = pair_ref.mono_mask
    closing      Qt = Qg (+ U_harm on l = 1), P = pot_in - 2 D f_l Qt, grad = d/dpos sum_i P_i . Qg_i(pos) at fixed P (the frame
                 adjoint: what the closing kernel adds to a zeroed gradient), dQ_local = rot_global2local(P) (P itself on
                 axis-free sites), E_self = pme_self(Qt), E_pen = pol_penalty(U, pol)
    frame virial V[a][b] = sum over the sites and their used axis atoms m of sh_a(i, m) g_b(i, m), sh = n . box the lattice
                 translation the minimum image removes from pos[m] - pos[i] (n = floor(d . box^-1 + 1/2), image_shift of
                 pme_math.h), g(i, m) = dL/d(position of m) through the frame of site i alone.  With the cell strained as
                 box (1 + eps) at fixed positions, dL/d eps_ab = -V_ab (checked against central differences on the CPU).

The gradient is taken on an EXTENDED system in which every site owns private copies of its axis atoms, so that autograd returns
the four contributions of every frame separately (to the site, its z, x and y atom): their scatter is the gradient, their
products with the shifts the virial, and what a subtly wrong kernel would give (`perturbed`) is a scatter with a term missing.

Cases: general sites, not water -- every site with a frame carries all moments, parameters drawn per site, pot_in unit normal
scaled per l.  Frame groups of 1 .. 4 consecutive atoms: a centre with one to three mates at 0.82 .. 0.88 under about 90 degrees;
ThreeFold and Bisector sit on centres, Z-then-X, Z-bisect and Z-only on mates, single atoms are axis-free charge-only sites, and
the atoms of a group are stored in a random order, so that every rule appears at every place of a group.  A third of the groups
lie across a cell face.  Sizes by the kernels' own constants (256 atoms per run of k_finish_rows and per workgroup of
k_prepare_sites, 32 per run of the gather's epilogue, E_WORDS = 146 energy words).

Conditioning, asserted when a case is built (`check_conditioning`): every angle between the unit vectors that enter a
Gram-Schmidt or bisect step within 40 .. 140 degrees, every site-axis atom distance within 0.8 .. 1.3 in cells of edge >= 8,
and |vz0.x| of a Z-only site at least 0.05 away from 0.5, where the reference's choice of x axis jumps."""
import functools

import numpy as np
import torch

from oracle import admp_oracle as O
from tests.hostshim_util import lib, dp, c64, i32
from tests.pair_ref import mono_mask, FLOOR_FACTOR, TILT

F64 = torch.float64
KAPPA = 0.41
K_MESH = (6, 7, 8)              # the smallest legal mesh has 6 points an axis; three lengths so that no two axes can be confused
POT_SCALE = np.array([1.0] + [0.6] * 3 + [0.3] * 5)
FINISH_BLOCK, GATHER_RUN, MAX_GROUP, ATOM_BLOCK, E_WORDS = 256, 32, 4, 256, 146
ZTHENX, BISECTOR, ZBISECT, THREEFOLD, ZONLY, NOAXIS = 0, 1, 2, 3, 4, 5
BOX_ORTHO = np.diag([9.0, 8.5, 10.0])
BOX_TRIC = TILT * 9.0
F32_FLOOR_CAP = 1e-5            # a case whose host f32 floor is above this is ill-conditioned: redraw it


def T(x):
    return torch.as_tensor(np.array(x, dtype=np.float64))


# ---- topology ------------------------------------------------------------------------------------------------------------------
def used_slots(at):
    """(Na,3) bool: which of the (z, x, y) index slots the axis rule of a site uses"""
    at = np.asarray(at)
    return np.stack([at != NOAXIS, (at != NOAXIS) & (at != ZONLY), (at == ZBISECT) | (at == THREEFOLD)], axis=1)


def group_layout(at, ai):
    """What admp_set_topology derives (admp_amd/csrc/topology_plan.h `topology_plan`, restated here; compared array for array
    by tests/test_topology_plan_cpu.py): the inverse frame map and, when every connected component of "site i uses
    atom m" is a run of at most 4 consecutive atoms, the frame groups and their runs.  Returns dict(inv, groups, rows_blk,
    gath_blk); groups is None when the topology is not made of groups."""
    at, ai = np.asarray(at), np.asarray(ai)
    n = len(at)
    use = used_slots(at)
    inv = [[] for _ in range(n)]
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i in range(n):
        if at[i] == NOAXIS or ai[i, 0] < 0:
            inv[i].append(i)
            continue
        mem = [i] + [int(ai[i, k]) if use[i, k] else -1 for k in range(3)]
        for m in range(4):
            if mem[m] >= 0 and mem[m] not in mem[:m]:
                inv[mem[m]].append(i)
        for m in mem[1:]:
            if m >= 0:
                a, b = find(i), find(m)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    gp, ok, prev = [], True, -1
    for i in range(n):
        r = find(i)
        if r != prev:
            if r != i:
                ok = False
                break
            gp.append(i)
            prev = r
        elif i - r >= MAX_GROUP:
            ok = False
            break
    gp.append(n)
    out = dict(inv=inv, groups=None, rows_blk=None, gath_blk=None)
    if ok:
        out['groups'] = np.array(gp)
        for key, cap in (('rows_blk', FINISH_BLOCK), ('gath_blk', GATHER_RUN)):
            blk = [0]
            for g in range(len(gp) - 1):
                if gp[g + 1] - blk[-1] > cap:
                    blk.append(gp[g])
            blk.append(n)
            out[key] = np.array(blk)
    return out


def expected_info(c, form, groups_on=True, lanes4=True, rows_grid=1024):
    """info of admp_site_close for the form a test selects (launch_finish's rules, atom_kernels.hip): `form` is the form asked
    for through the per-call switches ('rows', 'groups', 'pull', 'gather'); groups_on: ADMP_FINISH_GROUPS, lanes4:
    ADMP_FINISH4_MAX above the atom count.  Returns the dict the wrapper returns, or None where the call must be refused."""
    lay = group_layout(c['axis_type'], c['axis_indices'])
    have = groups_on and lay['groups'] is not None
    ng = len(lay['groups']) - 1 if have else 0
    nrow = len(lay['rows_blk']) - 1 if have else 0
    if form == 'gather':
        return dict(form='gather_epilogue', ngathblk=len(lay['gath_blk']) - 1) if have else None
    if form in ('rows', 'groups') and have:
        grid = min(nrow, max(1, min(1024, rows_grid))) if form == 'rows' else 0
        return dict(form=form, ngroups=ng, nrowblk=nrow, rows_grid=grid)
    return dict(form='pull4' if lanes4 else 'pull1', ngroups=ng, nrowblk=nrow, rows_grid=0)


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _min_image(d, box):
    s = d @ np.linalg.inv(box)
    n = np.floor(s + 0.5)
    return d - n @ box, n


def _angle(a, b):
    return np.degrees(np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0)))


def conditioning(pos, box, at, ai):
    """the angles (degrees) that enter a bisect or Gram-Schmidt step, the site-axis atom distances, the largest fractional
    displacement and | |vz0.x| - 0.5 | of the Z-only sites, each as a flat array over the sites that have them"""
    at, ai = np.asarray(at), np.asarray(ai)
    use = used_slots(at)
    angles, bonds, fracs, zonly = [], [], [], []
    for i in range(len(at)):
        if at[i] == NOAXIS:
            continue
        v = []
        for k in range(3):
            if use[i, k]:
                d, _ = _min_image(pos[ai[i, k]] - pos[i], box)
                bonds.append(np.linalg.norm(d))
                fracs.append(np.abs(d @ np.linalg.inv(box)).max())
                v.append(_unit(d))
            else:
                v.append(None)
        vz, vx, vy = v
        t = at[i]
        if t == ZTHENX:
            angles.append(_angle(vx, vz))
        elif t == BISECTOR:
            angles += [_angle(vz, vx), _angle(vx, _unit(vz + vx))]
        elif t == ZBISECT:
            angles += [_angle(vx, vy), _angle(_unit(vx + vy), vz)]
        elif t == THREEFOLD:
            angles += [_angle(vz, vx), _angle(vz, vy), _angle(vx, vy), _angle(vx, _unit(vz + vx + vy))]
        else:
            xz = np.floor(abs(vz[0]) + 0.5)
            angles.append(_angle(np.array([1.0 - xz, xz, 0.0]), vz))
            zonly.append(abs(abs(vz[0]) - 0.5))
    return dict(angles=np.array(angles), bonds=np.array(bonds), fracs=np.array(fracs), zonly=np.array(zonly))


def check_conditioning(pos, box, at, ai):
    q = conditioning(pos, box, at, ai)
    assert np.linalg.norm(box, axis=1).min() >= 8.0
    if q['angles'].size:
        assert q['angles'].min() >= 40.0 and q['angles'].max() <= 140.0, (q['angles'].min(), q['angles'].max())
        assert q['bonds'].min() >= 0.8 and q['bonds'].max() <= 1.3, (q['bonds'].min(), q['bonds'].max())
        assert q['fracs'].max() < 0.25
    if q['zonly'].size:
        assert q['zonly'].min() >= 0.05, q['zonly'].min()
    return q


def _group_rules(size, variant):
    """axis rules of a group of `size` atoms, centre first: (type, z, x, y) per member with member numbers as indices"""
    if size == 1:
        return [(NOAXIS, -1, -1, -1)]
    if size == 2:      # two Z-only sites, or a Z-only site whose axis atom is an axis-free charge-only site
        return [[(ZONLY, 1, -1, -1), (ZONLY, 0, -1, -1)], [(NOAXIS, -1, -1, -1), (ZONLY, 0, -1, -1)]][variant % 2]
    if size == 3:
        return [[(BISECTOR, 1, 2, -1), (ZTHENX, 0, 2, -1), (ZONLY, 0, -1, -1)],
                [(BISECTOR, 2, 1, -1), (ZONLY, 0, -1, -1), (ZTHENX, 0, 1, -1)],
                [(BISECTOR, 1, 2, -1), (ZTHENX, 0, 2, -1), (ZTHENX, 0, 1, -1)]][variant % 3]
    return [[(THREEFOLD, 1, 2, 3), (ZBISECT, 2, 0, 3), (ZTHENX, 0, 3, -1), (ZONLY, 0, -1, -1)],
            [(BISECTOR, 3, 1, -1), (ZTHENX, 0, 2, -1), (ZBISECT, 1, 0, 3), (ZONLY, 0, -1, -1)],
            [(THREEFOLD, 3, 1, 2), (ZONLY, 0, -1, -1), (ZBISECT, 3, 0, 1), (ZTHENX, 0, 1, -1)]][variant % 3]


def _group_shape(rng, size):
    """member positions relative to the centre: mates at 0.82 .. 0.88 along three jittered orthogonal directions, in a random
    orientation"""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    dirs = _unit(q + rng.normal(size=(3, 3)) * 0.04)
    out = np.zeros((size, 3))
    out[1:] = dirs[:size - 1] * rng.uniform(0.82, 0.88, (size - 1, 1))
    return out


def build_groups(rng, sizes, box, straddle=True):
    """positions and topology of consecutive frame groups of the sizes given; every group is redrawn until it meets the
    conditioning, placed at a random point of the cell -- every third one on a face -- and its atoms are wrapped into the cell"""
    n = int(np.sum(sizes))
    pos, at, ai = np.zeros((n, 3)), np.full(n, NOAXIS, dtype=np.int32), -np.ones((n, 3), dtype=np.int32)
    a0 = 0
    for g, size in enumerate(sizes):
        rules = _group_rules(size, g // 2)
        perm = rng.permutation(size)               # member m is stored at a0 + perm[m]
        for _ in range(2000):
            shape = _group_shape(rng, size)
            lt = np.array([r[0] for r in rules], dtype=np.int32)
            li = np.array([r[1:] for r in rules], dtype=np.int32)
            try:
                check_conditioning(shape, np.eye(3) * 50.0, lt, li)
                break
            except AssertionError:
                continue
        else:
            raise RuntimeError('no well-conditioned group of %d found' % size)
        f = 0.15 + 0.7 * rng.random(3)      # (well inside: the groups across a face are the chosen ones)
        if straddle and g % 3 == 0:
            f[(g // 3) % 3] = rng.uniform(-0.01, 0.01)
        centre = f @ box
        for m, r in enumerate(rules):
            i = a0 + perm[m]
            pos[i] = centre + shape[m]
            at[i] = r[0]
            ai[i] = [a0 + perm[k] if k >= 0 else -1 for k in r[1:]]
        a0 += size
    frac = pos @ np.linalg.inv(box)
    pos = (frac - np.floor(frac)) @ box
    return pos, at, ai


def draw_parameters(rng, at, pol_frac=0.6):
    """Q_local, pol, thole, U per site.  Axis-free sites are charge-only.  Of the others about pol_frac are polarizable and
    carry a dipole, and a few take each of the states next to charge-only that the mark must tell apart: charge-only on a site
    with a frame; a charge and a polarizability; a charge and a dipole handed in without a polarizability (tiny, so that its
    penalty at the clamped polarizability 1e-8 does not swamp the energy)."""
    n = len(at)
    Q = rng.normal(size=(n, 9)) * np.array([1, .5, .5, .5, .3, .3, .3, .3, .3])
    pol = np.where(rng.random(n) < pol_frac, rng.uniform(0.3, 1.5, n), 0.0)
    thole = rng.uniform(0.2, 9.0, n)
    U = rng.normal(size=(n, 3)) * 0.1
    U[pol == 0] = 0.0
    kind = rng.integers(0, 12, n)
    bare = (kind < 3) & (at != NOAXIS)
    Q[bare, 1:] = 0.0
    pol[bare & (kind != 1)] = 0.0
    U[bare] = 0.0
    lone_u = bare & (kind == 2)
    U[lone_u] = rng.normal(size=(n, 3))[lone_u] * 1e-6
    free = at == NOAXIS
    Q[free, 1:] = 0.0
    pol[free] = 0.0
    U[free] = 0.0
    thole[pol == 0] = 0.0
    return Q, pol, thole, U


def _finish(name, rng, pos, box, at, ai, pol_blocks=None, phi=None):
    n = len(at)
    Q, pol, thole, U = draw_parameters(rng, at)
    if pol_blocks is not None:      # per workgroup of k_prepare_sites: 'none', 'all' or 'mix'
        for b, what in enumerate(pol_blocks):
            s = slice(b * ATOM_BLOCK, min(n, (b + 1) * ATOM_BLOCK))
            if what == 'none':
                pol[s], U[s], thole[s] = 0.0, 0.0, 0.0
            elif what == 'all':
                pol[s] = rng.uniform(0.3, 1.5, s.stop - s.start)
                U[s] = rng.normal(size=(s.stop - s.start, 3)) * 0.1
                thole[s] = rng.uniform(0.2, 9.0, s.stop - s.start)
    c = dict(name=name, n=n, pos=pos, box=np.array(box), axis_type=at, axis_indices=ai, Q_local=Q, pol=pol, thole=thole, U=U,
             pot_in=rng.normal(size=(n, 9)) * POT_SCALE, kappa=KAPPA, K=K_MESH, lpol=True, phi=phi,
             pairs=np.zeros((0, 2), dtype=np.int32))
    c['cond'] = check_conditioning(pos, box, at, ai)
    c['mono'] = mono_mask(Q, pol, U)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _sizes_mixed(n):
    """the repeating pattern 3, 4, 1, 2, 4, 3 cut to n atoms"""
    out, k = [], 0
    while sum(out) < n:
        out.append(min((3, 4, 1, 2, 4, 3)[k % 6], n - sum(out)))
        k += 1
    return out


def _case_rules(tric):
    def build(rng):
        box = BOX_TRIC if tric else BOX_ORTHO
        sizes = [4, 4, 1, 4, 4, 1, 4, 4, 1, 4, 1, 4]      # 36 atoms: every rule, four axis-free sites; 2 runs of the gather
        pos, at, ai = build_groups(rng, sizes, box)
        return _finish('rules_tric' if tric else 'rules_ortho', rng, pos, box, at, ai)
    return build


def _case_mixed(n, tric=False, pol_blocks=None, straddle=True, name=None):
    def build(rng):
        box = BOX_TRIC if tric else BOX_ORTHO
        pos, at, ai = build_groups(rng, _sizes_mixed(n), box, straddle)
        return _finish(name or 'mixed_n%d' % n, rng, pos, box, at, ai, pol_blocks)
    return build


def _case_uniform(size, n):
    def build(rng):
        pos, at, ai = build_groups(rng, [size] * (n // size), BOX_ORTHO)
        return _finish('groups%d_n%d' % (size, n), rng, pos, BOX_ORTHO, at, ai)
    return build


def _case_hub(rng):
    """Not made of groups: four groups of 3, of which site 3 takes its x atom 5 places away (atom 8: the whole group of 8 is
    moved next to site 3), and six Z-only sites (12 .. 17) placed around atom 1, their common z atom: with its own frame and
    its mates' atom 1 has more than 4 frames in its inverse map, so that lane 0 of k_finish_pull<4> walks its loop twice."""
    box = BOX_ORTHO
    pos, at, ai = build_groups(rng, [3] * 6, box, straddle=False)
    hub = 1
    z3 = int(ai[3, 0])
    at[3] = ZTHENX
    ai[3] = [z3, 8, -1]
    for i in range(12, 18):
        at[i] = ZONLY
        ai[i] = [hub, -1, -1]
    for _ in range(5000):
        for i in range(12, 18):
            pos[i] = pos[hub] + _unit(rng.normal(size=3)) * rng.uniform(0.85, 1.25)
        pos[6:9] += pos[3] + _unit(rng.normal(size=3)) * rng.uniform(0.85, 1.25) - pos[8]
        frac = pos @ np.linalg.inv(box)
        p2 = (frac - np.floor(frac)) @ box
        try:
            check_conditioning(p2, box, at, ai)
            break
        except AssertionError:
            continue
    else:
        raise RuntimeError('no well-conditioned hub found')
    assert group_layout(at, ai)['groups'] is None and max(len(v) for v in group_layout(at, ai)['inv']) > 4
    return _finish('hub_n18', rng, p2, box, at, ai)


def _case_noise(rng):
    """the rules case again on white-noise phi: the gather's own pot and grad (mesh_ref.GatherRef) add to the closing work"""
    from tests.mesh_ref import noise
    pos, at, ai = build_groups(rng, [4, 4, 1, 4, 4, 1, 4, 4, 1, 4, 3, 4], BOX_TRIC)
    return _finish('rules_noise', rng, pos, BOX_TRIC, at, ai, phi=noise(K_MESH, 77, 8).astype(np.float64))


def with_unused_slots(c):
    """the case with every index slot its axis rule does not use pointing at an atom far outside the site's group and run: in
    another run of k_finish_rows where there is more than one (40 atoms or more from its ends, so in another run of the gather
    too), else in another run of the gather"""
    at, ai = c['axis_type'], np.array(c['axis_indices'])
    lay = group_layout(at, ai)
    rows = lay['rows_blk'] if len(lay['rows_blk']) > 2 else lay['gath_blk']
    assert len(rows) > 2
    margin = 40 if rows is lay['rows_blk'] else 0
    use = used_slots(at)
    for i in range(c['n']):
        r = int(np.searchsorted(rows, i, side='right')) - 1
        for k in range(3):
            if not use[i, k] and at[i] != NOAXIS:
                r2 = (r + 1 + k) % (len(rows) - 1)
                r2 = r2 if r2 != r else (r + 1) % (len(rows) - 1)
                lo, hi = rows[r2] + margin, rows[r2 + 1] - margin
                ai[i, k] = lo + (7 * i + k) % (hi - lo)
    out = dict(c, name=c['name'] + '_unused', axis_indices=ai)
    ai.setflags(write=False)
    return out


_BUILDERS = {
    'rules_ortho': _case_rules(False), 'rules_tric': _case_rules(True),
    'n1': _case_mixed(1), 'n4': _case_mixed(4), 'n31': _case_mixed(31), 'n32': _case_mixed(32), 'n33': _case_mixed(33),
    'n255': _case_mixed(255), 'n256': _case_mixed(256, tric=True), 'n257': _case_mixed(257),
    # 3 runs of k_finish_rows, 4 workgroups of k_prepare_sites: without a polarizable site, all 256, and two mixed
    'mixed_n760': _case_mixed(760, pol_blocks=('none', 'all', 'mix', 'mix')),
    'groups3_n258': _case_uniform(3, 258),         # 85 groups = 255 atoms: run 0 ends one short of 256
    'groups4_n260': _case_uniform(4, 260),         # exactly 256 a run, 32 a run of the gather
    'inside_n33': _case_mixed(33, straddle=False, name='inside_n33'),      # no group across a face: the frame virial is exactly zero
    'hub_n18': _case_hub,
    'rules_noise': _case_noise,
}
CASES = tuple(_BUILDERS) + ('rules_ortho_unused', 'mixed_n760_unused')
UNUSED_OF = {'rules_ortho_unused': 'rules_ortho', 'mixed_n760_unused': 'mixed_n760'}
GRID_CASE = 'mixed_n760'


@functools.lru_cache(maxsize=None)
def case(name):
    if name.endswith('_unused'):
        return with_unused_slots(case(name[:-len('_unused')]))
    c = _BUILDERS[name](np.random.default_rng(4100 + list(_BUILDERS).index(name)))
    if name == 'inside_n33':
        assert not straddling(c).any()
    return c


def straddling(c):
    """per site: whether a used axis vector crosses a cell face (a non-zero lattice translation in its minimum image)"""
    at, ai, pos, box = c['axis_type'], c['axis_indices'], c['pos'], c['box']
    use = used_slots(at)
    out = np.zeros(c['n'], dtype=bool)
    for k in range(3):
        idx = np.where(use[:, k], ai[:, k], np.arange(c['n']))
        _, nshift = _min_image(pos[idx] - pos, box)
        out |= use[:, k] & (np.abs(nshift).max(1) > 0)
    return out


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def self_factor_rows(kappa):
    l_list = np.array([0] + [1] * 3 + [2] * 5)
    l_fac2 = np.array([1] + [3] * 3 + [15] * 5)
    return kappa / np.sqrt(np.pi) * (2 * kappa ** 2) ** l_list / l_fac2


def u_harm(U):
    return np.asarray(U)[:, [2, 0, 1]]


_DUMMY = np.array([[0.31, 0.17, 0.23], [0.41, -0.19, 0.27], [-0.29, 0.37, 0.13], [0.111, 0.222, 0.333]])


def _extended(c):
    """Frames on the extended system: five rows per site -- the site, private copies of its z, x and y atoms, and a spacer --
    with the site rows and the three sets of copies as four autograd leaves.  (The oracle points the slots a rule does not use
    at the next row and discards the value; a copy of an unused slot and the spacer sit at offsets from the site that no atom
    shares, so that no two neighbouring rows coincide and no 0/0 enters the graph.)"""
    n = c['n']
    at, ai = np.asarray(c['axis_type']), np.asarray(c['axis_indices'])
    use = used_slots(at)
    p = T(c['pos'])
    leaves = [p.clone().requires_grad_(True)]
    for k in range(3):
        src = np.where(use[:, k, None], np.asarray(c['pos'])[np.where(use[:, k], ai[:, k], 0)], np.asarray(c['pos']) + _DUMMY[k])
        leaves.append(T(src).requires_grad_(True))
    spacer = T(np.asarray(c['pos']) + _DUMMY[3])
    ext = torch.stack(leaves + [spacer], dim=1).reshape(5 * n, 3)
    at_ext = np.full(5 * n, NOAXIS)
    at_ext[0::5] = at
    ai_ext = -np.ones((5 * n, 3), dtype=np.int64)
    for k in range(3):
        ai_ext[0::5, k] = np.where(use[:, k], 5 * np.arange(n) + k + 1, -1)
    R = O.construct_local_frames(ext, T(c['box']), at_ext, ai_ext)[0::5]
    return R, leaves


def site_table_ref(c):
    """the rows k_prepare_sites writes: r, Q global, U harmonic, p6, thole, the charge-only mark"""
    R = O.construct_local_frames(T(c['pos']), T(c['box']), c['axis_type'], c['axis_indices'])
    Qg = O.rot_local2global(T(c['Q_local']), R, 2).numpy()
    return dict(r=np.array(c['pos']), Q=Qg, U=u_harm(c['U']), p6=np.asarray(c['pol']) ** (1.0 / 6.0), thole=np.array(c['thole']),
                mono=mono_mask(c['Q_local'], c['pol'], c['U']), frames=R.numpy(), act=np.nonzero(c['pol'] > 0)[0])


def scatter(c, Gp, Gz, Gx, Gy):
    """the gradient from the four contributions of every frame"""
    at, ai = np.asarray(c['axis_type']), np.asarray(c['axis_indices'])
    use = used_slots(at)
    g = np.array(Gp)
    for k, G in enumerate((Gz, Gx, Gy)):
        rows = np.nonzero(use[:, k])[0]
        np.add.at(g, ai[rows, k], G[rows])
    return g


def closing_ref(c, pot_in=None, self_from_total=True):
    """P, grad (frame adjoint), dQ_local, E_self, E_pen, the four contributions per frame and the frame virial.  pot_in: in
    place of the case's (the gather case hands pot_in + the reciprocal part).  self_from_total=False: the self term taken from Q
    in place of Q + U (a perturbed reference)."""
    n = c['n']
    pot = np.asarray(c['pot_in'] if pot_in is None else pot_in)
    R, leaves = _extended(c)
    Qg = O.rot_local2global(T(c['Q_local']), R, 2)
    Qt = Qg.detach().clone()
    Qt_true = Qt.clone()
    Qt_true[:, 1:4] += T(u_harm(c['U']))
    if self_from_total:
        Qt = Qt_true
    P = T(pot) - 2.0 * O.DIELECTRIC * T(self_factor_rows(c['kappa']))[None, :] * Qt
    L = torch.sum(P * Qg)
    Gp, Gz, Gx, Gy = [g.numpy() for g in torch.autograd.grad(L, leaves)]
    dQ = O.rot_global2local(P, R.detach(), 2).numpy()
    E_self = float(O.pme_self(Qt, c['kappa'], 2))
    E_pen = float(O.pol_penalty(T(c['U']), T(c['pol'])))
    at, ai, pos, box = np.asarray(c['axis_type']), np.asarray(c['axis_indices']), c['pos'], c['box']
    use = used_slots(at)
    vir = np.zeros((3, 3))
    for k, G in enumerate((Gz, Gx, Gy)):
        rows = np.nonzero(use[:, k])[0]
        _, nshift = _min_image(pos[ai[rows, k]] - pos[rows], box)
        vir += (nshift @ box).T @ G[rows]
    return dict(P=P.numpy(), Qg=Qg.detach().numpy(), grad=scatter(c, Gp, Gz, Gx, Gy), dQ=dQ, E_self=E_self, E_pen=E_pen,
                parts=(Gp, Gz, Gx, Gy), vir=vir, L=float(L.detach()))


def frame_energy(c, P, pos=None, box=None):
    """L = sum_i P_i . Qg_i at the positions and cell given, P held fixed (for the finite differences of the CPU test)"""
    R = O.construct_local_frames(T(c['pos'] if pos is None else pos), T(c['box'] if box is None else box), c['axis_type'],
                                 c['axis_indices'])
    return float(torch.sum(T(P) * O.rot_local2global(T(c['Q_local']), R, 2)))


def direct_grad(c, P):
    """d/dpos of frame_energy by autograd on the system as it is (the CPU test holds `scatter` of the extended system to it)"""
    p = T(c['pos']).requires_grad_(True)
    R = O.construct_local_frames(p, T(c['box']), c['axis_type'], c['axis_indices'])
    L = torch.sum(T(P) * O.rot_local2global(T(c['Q_local']), R, 2))
    return torch.autograd.grad(L, [p])[0].numpy()


@functools.lru_cache(maxsize=None)
def gather_part(name, prec):
    """reciprocal pot, grad and their bars of the white-noise case: mesh_ref.GatherRef on the reference's global moments"""
    from tests import mesh_ref as M
    c = case(name)
    Qg = site_table_ref(c)['Q']
    mc = dict(K=c['K'], box=c['box'], pos=c['pos'], Q=Qg, U=c['U'], lpol=True, n=c['n'])
    g = M.GatherRef(M.SpreadRef(mc, prec), np.asarray(c['phi'], dtype=M.RT[prec]).astype(np.float64))
    return dict(pot=g.pot, grad=g.grad, bars=g.bars())


@functools.lru_cache(maxsize=None)
def reference(name, prec='double'):
    """closing_ref of the case; the white-noise case: gather + closing on pot_in + pot_recip (in the type's own phi)"""
    c = case(name)
    if c['phi'] is None:
        return closing_ref(c)
    g = gather_part(name, prec)
    r = closing_ref(c, c['pot_in'] + g['pot'])
    r['grad_frames'] = r['grad']
    r['grad'] = r['grad'] + g['grad']
    r['gather'] = g
    return r


# ---- host floors: the kernels' own frame_math.h compiled for the host, in float32 -----------------------------------------------
def shim_frames(c, prec, P, extended=False):
    """tests/hostshim shim_frames: frames, Q global, frame adjoint and dQ_local at P, atom by atom in the type.  extended: on the
    system with private copies of the axis atoms: returns the four contributions per frame in place of the gradient."""
    n = c['n']
    at, ai, pos = np.asarray(c['axis_type']), np.asarray(c['axis_indices']), np.asarray(c['pos'])
    Ql, Pp = np.asarray(c['Q_local']), np.asarray(P)
    if extended:
        use = used_slots(at)
        pos = np.concatenate([pos] + [pos[np.where(use[:, k], ai[:, k], 0)] for k in range(3)])
        ai = np.concatenate([np.stack([np.where(use[:, k], (k + 1) * n + np.arange(n), -1) for k in range(3)], axis=1),
                             -np.ones((3 * n, 3), dtype=np.int64)])
        at = np.concatenate([at, np.full(3 * n, NOAXIS)])
        Ql = np.concatenate([Ql, np.zeros((3 * n, 9))])
        Pp = np.concatenate([Pp, np.zeros((3 * n, 9))])
    m = len(at)
    frames, Qg, grad, dQ = np.zeros((m, 9)), np.zeros((m, 9)), np.zeros((m, 3)), np.zeros((m, 9))
    lib().shim_frames(prec, m, dp(c64(pos)), dp(c64(c['box'])), dp(i32(at)), dp(i32(ai)), dp(c64(Ql)), dp(c64(Pp)), dp(frames),
                      dp(Qg), dp(grad), dp(dQ))
    out = dict(frames=frames[:n].reshape(n, 3, 3), Qg=Qg[:n], dQ=dQ[:n])
    if extended:
        out['parts'] = tuple(grad[k * n:(k + 1) * n] for k in range(4))
    else:
        out['grad'] = grad
    return out


def potential_f32(c, Qg32, pot_in):
    """P = pot - 2 D f_l (Qg + U) and the per-site self and penalty energies as the closing kernels form them in float32
    (total_potential of atom_kernels.hip, self_factors of frame_math.h): products of rounded operands, summed in double"""
    f = np.float32
    k = f(c['kappa'])
    k2 = f(2) * k * k
    f0 = k * f(0.5 * 1.1283791670955126)
    fl = np.array([f0] + [f0 * k2 / f(3)] * 3 + [f0 * k2 * k2 / f(15)] * 5, dtype=f)
    q = np.asarray(Qg32, dtype=f).copy()
    q[:, 1:4] += u_harm(c['U']).astype(f)
    P = np.asarray(pot_in, dtype=f) - f(2.0 * O.DIELECTRIC) * fl[None, :] * q
    e_self = -O.DIELECTRIC * (fl[None, :] * q * q).astype(np.float64).sum(1)
    al = np.maximum(np.asarray(c['pol'], dtype=f), f(1e-8)).astype(np.float64)
    e_pen = O.DIELECTRIC * 0.5 * (np.asarray(c['U'], dtype=f).astype(np.float64) ** 2).sum(1) / al
    return P.astype(np.float64), e_self, e_pen


def rel_err(got, ref):
    """max |got - ref| / max |ref|; an all-zero reference wants exact zeros (inf otherwise)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max() if ref.size else 0.0
    d = np.abs(got - ref).max() if ref.size else 0.0
    if scale == 0.0:
        return 0.0 if d == 0.0 else np.inf
    return d / scale


def site_energies(c):
    """per-site self and penalty energies of the reference"""
    r = site_table_ref(c)
    Qt = r['Q'].copy()
    Qt[:, 1:4] += r['U']
    e_self = -O.DIELECTRIC * (self_factor_rows(c['kappa'])[None, :] * Qt ** 2).sum(1)
    e_pen = O.DIELECTRIC * 0.5 * (np.asarray(c['U']) ** 2).sum(1) / np.maximum(c['pol'], 1e-8)
    return e_self, e_pen


@functools.lru_cache(maxsize=None)
def floors(name):
    """What float32 storage and arithmetic cost on the host with the kernels' own frame_math.h (shim_frames at prec 4 on the
    potential of potential_f32), against the float64 reference: grad, dQ, Qg, vir relative to the array's largest entry.
    Energies (absolute): the per-site float32 errors summed WITHOUT cancellation -- the device adds the same per-site terms in
    double in another order, so their signed sum on the host would be an accident of that order -- and not below half a unit
    2^-24 of the summed magnitudes, what rounding the inputs alone costs."""
    c = case(name)
    ref = reference(name, 'single')
    pot_in = c['pot_in'] if c['phi'] is None else c['pot_in'] + ref['gather']['pot']
    first = shim_frames(c, 4, np.zeros((c['n'], 9)))
    P32, es32, ep32 = potential_f32(c, first['Qg'], pot_in)
    plain, ext = shim_frames(c, 4, P32), shim_frames(c, 4, P32, extended=True)
    es, ep = site_energies(c)
    at, ai, pos = np.asarray(c['axis_type']), np.asarray(c['axis_indices']), c['pos']
    box32 = np.asarray(c['box'], dtype=np.float32).astype(np.float64)
    use = used_slots(at)
    vir = np.zeros((3, 3))
    for k in range(3):
        rows = np.nonzero(use[:, k])[0]
        _, nshift = _min_image(pos[ai[rows, k]] - pos[rows], c['box'])
        vir += (nshift @ box32).T @ ext['parts'][k + 1][rows]
    u = 2.0 ** -24
    return dict(grad=rel_err(plain['grad'], ref.get('grad_frames', ref['grad'])), dQ=rel_err(plain['dQ'], ref['dQ']),
                Qg=rel_err(plain['Qg'], ref['Qg']), vir=rel_err(vir, ref['vir']),
                E_self=max(np.abs(es32 - es).sum(), u * np.abs(es).sum()), E_pen=max(np.abs(ep32 - ep).sum(), u * np.abs(ep).sum()))


def single_bars(name):
    """float32: FLOOR_FACTOR x the host floor (pair_ref.FLOOR_FACTOR: the project's allowance for FMA contraction and ordering
    on the device over the host's float32 arithmetic)"""
    return {k: FLOOR_FACTOR * v for k, v in floors(name).items()}


def double_excess(got, ref, key, atol_factor):
    """largest |got - ref| / (atol_factor max|ref| + 1e-9 |ref|): <= 1 passes (pair_ref.double_bars)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = atol_factor * np.abs(ref).max() + 1e-9 * np.abs(ref)
    if not ref.size:
        return 0.0
    if (tol > 0).all():
        return float((np.abs(got - ref) / tol).max())
    return 0.0 if np.array_equal(got, ref) else np.inf


DOUBLE_ATOL = dict(grad=1e-8, dQ=1e-9, Qg=1e-9)


# ---- what a subtly wrong kernel would give ----------------------------------------------------------------------------------------
def contribution(c, parts, i, a):
    """what the frame of site i adds to atom a"""
    at, ai = c['axis_type'], c['axis_indices']
    use = used_slots(at)
    out = np.zeros(3)
    if i == a:
        out += parts[0][i]
    for k in range(3):
        if use[i, k] and ai[i, k] == a:
            out += parts[k + 1][i]
    return out


def perturbed(name, what):
    """(grad, dQ, E_self) of a reference with one term wrong; see tests/test_site_ref_cpu.py for which case catches which"""
    c = case(name)
    ref = closing_ref(c)
    Gp, Gz, Gx, Gy = ref['parts']
    at, ai = np.asarray(c['axis_type']), np.asarray(c['axis_indices'])
    lay = group_layout(at, ai)
    grad, dQ, E = ref['grad'].copy(), ref['dQ'], ref['E_self']
    if what == 'drop_y':                  # the y-atom term of ThreeFold and ZBisect
        grad = scatter(c, Gp, Gz, Gx, np.zeros_like(Gy))
    elif what == 'drop_mate_at_run_boundary':      # the last atom of run 0 loses what one group mate's frame adds to it
        a = int(lay['rows_blk'][1]) - 1
        mates = [i for i in lay['inv'][a] if i != a]
        grad[a] -= contribution(c, ref['parts'], mates[0], a)
    elif what == 'swap_xy':               # x and y axis atoms swapped on one site
        i = int(np.argmax(np.where(used_slots(at)[:, 2], np.abs(Gx - Gy).max(1), -1.0)))      # (a site that has a torque)
        grad[ai[i, 1]] += Gy[i] - Gx[i]
        grad[ai[i, 2]] += Gx[i] - Gy[i]
    elif what == 'self_from_Q':           # the self term taken from Q in place of Q + U
        r = closing_ref(c, self_from_total=False)
        grad, dQ, E = r['grad'], r['dQ'], r['E_self']
    elif what == 'run_shifted':           # the rows of run 1 taken one group further on
        a0, a1 = int(lay['rows_blk'][1]), int(lay['rows_blk'][2])
        g0 = int(np.searchsorted(lay['groups'], a0))
        size = int(lay['groups'][g0 + 1] - lay['groups'][g0])
        grad[a0:a1] = np.roll(ref['grad'][a0:a1], -size, axis=0)
    elif what == 'lane3_dropped':         # the partial of lane 3 of the 4-lane fold: frames 3, 7, .. of an atom's inverse map
        for a in range(c['n']):
            for i in lay['inv'][a][3::4]:
                grad[a] -= contribution(c, ref['parts'], i, a)
    else:
        raise KeyError(what)
    return dict(grad=grad, dQ=dQ, E_self=E)


PERTURBATIONS = ('drop_y', 'drop_mate_at_run_boundary', 'swap_xy', 'self_from_Q', 'run_shifted', 'lane3_dropped')
