"""Molecular (centre-of-mass) cell scaling on the GPU (admp_amd.md.MolecularCRescaleBarostat, groups_of; admp_md_mol_plan /
_sums / _scale / _info, mol_kernels.hip) against the float64 numpy restatement of tests/test_mol_plan_cpu.py, under that
module's bars: the sums, one application, determinism over the tile capacity, the reduction to the atomic barostat for
singleton groups, the vanishing strain derivative of bonded terms under molecular scaling, the pressure convention against
finite differences of the total energy under the molecular map, an ideal gas of rigid dimers that must sit at N_mol kB T / P0,
the refusals, and the driver examples/md/npt_water.py --rigid / --molecular end to end.  Both precisions wherever a handle is
involved, unless stated."""
import ctypes
import functools
import re

import numpy as np
import pytest

from tests.test_con_plan_cpu import CROSSINGS, Con, constraint_errors, rigid_system
from tests.test_gpu_md_barostat import (BAND, BAR, LOG_LINE, NPT_ARGS, POL_CONV_FD, bonded_case, sums_case, water_setup)
from tests.test_gpu_md_langevin import ACC, E_ARG, KB, MASS, dev, eps_of, host, owner, ref_normals, run_driver      # noqa: F401
from tests.test_md_random_cpu import normals
from tests.test_mol_plan_cpu import (E64, _ext, group_vectors, labels_of, mol_restated, plan_restated, scale_restated, sums_bars,
                                     sums_restated)
from tests.test_mts_plan_cpu import BOX

pytestmark = pytest.mark.gpu


def tol_of(o):
    return 1e-12 if eps_of(o) < 1e-10 else 1e-6


def np_ty(o):
    return np.float64 if eps_of(o) < 1e-10 else np.float32


@functools.lru_cache(maxsize=None)
def system():
    """rigid_system of tests/test_con_plan_cpu.py: 64 waters, 5 free atoms, two 5-atom stars, a 6-atom chain, shuffled,
    triclinic, seven groups across faces or a corner; a random gradient"""
    r, v, mass, con, wrapped = rigid_system(64, 5, 7)
    assert len(r) == 213 and len(con.comps) == 64 + 5 + 3
    for m, want in enumerate(CROSSINGS):
        assert all(axis in wrapped[m] for axis, _ in want), m
    labels = labels_of(len(r), con.pairs)
    q = mol_restated(r, v, 1.0 / mass, labels, BOX)
    assert (np.abs(q['s']).sum(1) > 0).sum() >= 7 and np.abs(q['d']).max() < 6.0
    g = np.random.default_rng(17).normal(size=r.shape) * 50.0
    return r, v, g, mass, con, labels


def make(o, cap=None, **kw):
    """a Constraints of the handle's precision (the fixture holds settings.PRECISION), the groups from it, the barostat on
    the fixture's handle, and the device arrays"""
    from admp_amd.md import Constraints, MolecularCRescaleBarostat, groups_of
    r, v, g, mass, con, labels = system()
    c = Constraints(len(r), con.pairs, con.lengths, mass)
    groups = groups_of(len(r), constraints=c)
    assert groups.dtype == np.int32 and np.array_equal(groups, labels)
    a = dict(dt_p_fs=5.0, temperature=300.0, pressure_bar=1.0, tau_p_fs=500.0, compressibility_per_bar=4.5e-5, seed=2 ** 40 + 3)
    a.update(kw)
    bs = MolecularCRescaleBarostat(o, mass, groups, tile_atoms=cap, **a)
    return bs, dev(o, r), dev(o, v), dev(o, g)


# ---- 1. sums ------------------------------------------------------------------------------------------------------------
def check_sums(bs, r, v, g, labels, box):
    """the restatement from the device tensors' own rounded values, under the bar of tests/test_mol_plan_cpu.py"""
    kin, rg, xi = bs.sums(r, v, g, box)
    ty = np_ty(bs._o)
    arrays = [host(t).astype(ty) for t in (r, v, g, bs.inv_mass)]
    kin_ref, rg_ref, kin_bar, rg_bar = sums_bars(*arrays, labels, box, ty == np.float64)
    dk, dg = np.abs(kin * ACC - kin_ref), np.abs(rg - rg_ref)
    print('n %d: kin %.2e of %.2e, rg %.2e of %.2e' % (len(labels), dk.max(), kin_bar.min(), dg.max(), rg_bar.min()))
    assert kin.shape == (3, 3) and rg.shape == (3, 3)
    assert (dk <= kin_bar).all() and (dg <= rg_bar).all()
    return kin, rg, xi


def test_sums_against_numpy(owner):
    """213 atoms in 72 groups (no multiple of a tile); xi is the first normal of (seed, step, stream 2, atom 0), to 1e-12;
    another step another xi, the step set back the same bit for bit; the atomic sums are far outside the bar"""
    from admp_amd.md import CRescaleBarostat
    r, v, g, mass, con, labels = system()
    bs, rd, vd, gd = make(owner)
    seed = bs.seed
    bs.step = 7
    kin, rg, xi7 = check_sums(bs, rd, vd, gd, labels, BOX)
    assert bs.step == 7                                              # only apply() counts
    assert abs(xi7 - ref_normals(1, seed, 7, 2)[0, 0]) <= 1e-12
    bs.step = 2 ** 33
    xi_hi = bs.sums(rd, vd, gd, BOX)[2]
    assert abs(xi_hi - ref_normals(1, seed, 2 ** 33, 2)[0, 0]) <= 1e-12 and xi_hi != xi7
    bs.step = 7
    again = bs.sums(rd, vd, gd, BOX)
    assert again[2] == xi7
    atomic = CRescaleBarostat(owner, mass, 5.0, 300.0, 1.0, 500.0, 4.5e-5, seed)
    atomic.step = 7
    kin_a, rg_a, xi_a = atomic.sums(rd, vd, gd)
    assert xi_a == xi7                                                # the normal of the atomic barostat
    assert np.abs(rg_a - rg).max() > 1.0 and np.trace(kin) < 0.75 * np.trace(kin_a)
    info = bs.plan_info()
    assert info['atoms'] == 213 and info['groups'] == 72 and info['largest_group'] == 6 and info['tile_atoms'] == 256
    assert info['tiles'] == 1 and info['lanes'] == 256 and info['launches'] >= 3
    assert info['lds_bytes'] == 56 * 72 + 7 * 213 * (8 if eps_of(owner) < 1e-10 else 4)


@pytest.mark.parametrize('cap', [6, 7, 64, 256])
def test_sums_at_every_capacity(owner, cap):
    """the 213 atoms in 1, 4 and more than 30 tiles, a tile's lanes partly idle: each under the bar of the restatement"""
    r, v, g, mass, con, labels = system()
    bs, rd, vd, gd = make(owner, cap=cap)
    bs.step = 7
    kin, rg, xi = check_sums(bs, rd, vd, gd, labels, BOX)
    info = bs.plan_info()
    assert info['tiles'] == plan_restated(labels, cap)['n_tiles'] and info['tile_atoms'] == cap
    assert abs(xi - ref_normals(1, bs.seed, 7, 2)[0, 0]) <= 1e-12


@functools.lru_cache(maxsize=None)
def many_tiles_case():
    """333 groups of three atoms within 3 A of their anchor, scattered over BOX and wrapped atom by atom, shuffled: at
    capacity 3 a tile per group, at 4 likewise, at 6 two groups per tile"""
    rng = np.random.default_rng(41)
    n_grp = 333
    base = rng.uniform(0.0, 1.0, size=(n_grp, 3)) @ BOX
    r = (base[:, None, :] + np.concatenate([np.zeros((n_grp, 1, 3)), rng.uniform(-0.85, 0.85, size=(n_grp, 2, 3))], axis=1)).reshape(-1, 3)
    frac = r @ np.linalg.inv(BOX)
    r = (frac - np.floor(frac)) @ BOX
    n = len(r)
    mass = np.tile(MASS, n_grp)
    labels = np.repeat(np.arange(n_grp), 3)
    perm = rng.permutation(n)
    out = [np.empty_like(x) for x in (r, mass, labels)]
    for o, x in zip(out, (r, mass, labels)):
        o[perm] = x
    r, mass, labels = out
    v = rng.normal(size=(n, 3)) * np.sqrt(ACC * KB * 300.0 / mass)[:, None]
    g = rng.normal(size=(n, 3)) * 50.0
    q = mol_restated(r, v, 1.0 / mass, labels, BOX)
    assert (np.abs(q['s']).sum(1) > 0).sum() >= 20 and np.abs(q['d']).max() < 3.0
    return r, v, g, mass, labels.astype(np.int32)


@pytest.mark.parametrize('cap,tiles', [(3, 333), (4, 333), (6, 167), (256, 4)])
def test_sums_with_more_tiles_than_workgroups(owner, cap, tiles):
    """the launch of k_md_mol_sums is capped at 256 workgroups: with 333 tiles the first 77 workgroups take a second tile and
    use their LDS again.  999 atoms in 333 shuffled groups with atoms across every face, under the bar of the restatement at
    every capacity; a skipped tile, a tile taken twice or words left over from the tile before would miss it by whole terms"""
    from admp_amd.md import MolecularCRescaleBarostat
    r, v, g, mass, labels = many_tiles_case()
    bs = MolecularCRescaleBarostat(owner, mass, labels, 5.0, 300.0, 1.0, 500.0, 4.5e-5, 3, tile_atoms=cap)
    assert bs.plan_info()['tiles'] == tiles == plan_restated(labels, cap)['n_tiles']
    rd, vd, gd = dev(owner, r), dev(owner, v), dev(owner, g)
    kin, rg, xi = check_sums(bs, rd, vd, gd, labels, BOX)
    # one group's terms are far above the bar: a missed or doubled tile cannot hide
    ty = np_ty(owner)
    _, _, kin_bar, rg_bar = sums_bars(*[host(t).astype(ty) for t in (rd, vd, gd, bs.inv_mass)], labels, BOX, ty == np.float64)
    q = mol_restated(host(rd), host(vd), host(bs.inv_mass), labels, BOX)
    one = np.abs(q['Rc'][:, :, None] * host(gd)[:, None, :]).reshape(-1, 9).max(axis=0).reshape(3, 3)
    assert (one > 100 * rg_bar).all()
    assert abs(xi - ref_normals(1, 3, 0, 2)[0, 0]) <= 1e-12


def test_singletons_in_more_tiles_than_workgroups(owner):
    """1000 free atoms at capacity 3: 334 tiles on 256 workgroups, against CRescaleBarostat.sums under the sums bar"""
    from admp_amd.md import CRescaleBarostat, MolecularCRescaleBarostat
    n = 1000
    mass, r, v, g = sums_case(owner, n, 5)
    box = np.eye(3) * 20.8
    par = (5.0, 300.0, 1.0, 500.0, 4.5e-5, 9)
    mol = MolecularCRescaleBarostat(owner, mass, np.arange(n), *par, tile_atoms=3)
    assert mol.plan_info()['tiles'] == 334
    kin_m, rg_m, xi_m = check_sums(mol, r, v, g, np.arange(n), box)
    kin_a, rg_a, xi_a = CRescaleBarostat(owner, mass, *par).sums(r, v, g)
    m = 1.0 / host(mol.inv_mass)
    vh, rh, gh = host(v), host(r), host(g)
    kin_abs = _ext(np.abs((vh[:, :, None] * vh[:, None, :]) * m[:, None, None]).reshape(-1, 9)) / ACC
    rg_abs = _ext(np.abs(rh[:, :, None] * gh[:, None, :]).reshape(-1, 9))
    assert xi_m == xi_a
    assert (np.abs(kin_m - kin_a) <= 64 * E64 * kin_abs).all() and (np.abs(rg_m - rg_a) <= 64 * E64 * rg_abs).all()


# ---- 2. one application -------------------------------------------------------------------------------------------------
def test_one_application_against_the_formulas(owner):
    """d eps and mu restated in numpy, mu - 1 and 1/mu - 1 by expm1; r and v to 4 eps max|.| of r + (mu - 1) R_c(i) and v +
    (1/mu - 1) V_c; every vector from a group's anchor to its atoms unchanged to 2 ulp of the coordinates in the scaled cell,
    so the constraints hold without a re-projection; the groups' centres scaled by mu and their velocities by 1/mu; the box
    scaled in place, the step counted; with zero compressibility the application is the identity, bit for bit"""
    import torch
    r, v, g, mass, con, labels = system()
    eps = eps_of(owner)
    bs, rd, vd, gd = make(owner, seed=11)
    bs.step = 3
    box = BOX.copy()
    box_id = id(box)
    vol = abs(np.linalg.det(BOX))
    p_inst, xi = 5.0e4, float(ref_normals(1, 11, 3, 2)[0, 0])
    d_eps = bs.beta_T / bs.tau_p * (p_inst - bs.P0) * bs.dt_p + np.sqrt(2.0 * KB * bs.T * BAR * bs.beta_T * bs.dt_p / (vol * bs.tau_p)) * xi
    mu_ref = np.exp(d_eps / 3.0)
    r0, v0, im = host(rd), host(vd), host(bs.inv_mass)
    r_ref, v_ref, q0 = scale_restated(r0, v0, im, labels, BOX, np.expm1(d_eps / 3.0), np.expm1(-d_eps / 3.0))
    mu = bs.apply(rd, vd, box, p_inst, xi)
    r1, v1 = host(rd), host(vd)
    assert abs(mu - mu_ref) <= 4 * E64 and mu != 1.0 and bs.step == 4
    assert id(box) == box_id and np.abs(box - mu_ref * BOX).max() <= 1e-15 * np.abs(BOX).max()
    rmax, vmax = np.abs(r0).max(), np.abs(v0).max()
    dr, dv = np.abs(r1 - r_ref).max(), np.abs(v1 - v_ref).max()
    print('mu - 1 %.6e; |dr| %.2e of %.2e, |dv| %.2e of %.2e' % (mu - 1.0, dr, 4 * eps * rmax, dv, 4 * eps * vmax))
    assert dr <= 4 * eps * rmax and dv <= 4 * eps * vmax
    assert np.abs(r1 - r0).max() > 100 * eps * rmax
    dd = np.abs(group_vectors(r1, labels, box) - group_vectors(r0, labels, BOX)).max()
    ce = constraint_errors(con, r1, box).max()
    print('intra-group vectors moved by %.2e of %.2e; constraint error %.2e' % (dd, 2 * eps * rmax, ce))
    assert dd <= 2 * eps * rmax
    assert ce <= constraint_errors(con, r0, BOX).max() + 4 * eps * rmax / con.lengths.min()
    # the atomic scaling would have stretched every constraint by mu - 1
    assert abs(mu - 1.0) > 100 * (4 * eps * rmax / con.lengths.min())
    q1 = mol_restated(r1, v1, im, labels, box)
    # (R_c(i) of the atoms, images included, against mu R_c(i))
    assert np.abs(q1['Rc'] - mu_ref * q0['Rc']).max() <= 4 * eps * rmax
    assert np.abs(q1['Vc'] - q0['Vc'] / mu_ref).max() <= 4 * eps * vmax
    # relative velocities inside a group: unchanged but for the one rounding of v + dv
    rel0, rel1 = v0 - v0[q0['anchor']], v1 - v1[q0['anchor']]
    assert np.abs(rel1 - rel0).max() <= 2 * eps * vmax
    ident, rd, vd, gd = make(owner, seed=11, compressibility_per_bar=0.0)
    ra, va, b1 = rd.clone(), vd.clone(), box.copy()
    assert ident.apply(rd, vd, box, p_inst, xi) == 1.0
    assert torch.equal(rd, ra) and torch.equal(vd, va) and np.array_equal(box, b1) and ident.step == 1


# ---- 3. determinism -----------------------------------------------------------------------------------------------------
def test_results_are_bit_identical_for_every_capacity_and_run(owner):
    import torch
    outs = []
    for cap in (6, 7, 64, 100, 256, 256):
        bs, rd, vd, gd = make(owner, cap=cap)
        box = BOX.copy()
        bs.apply(rd, vd, box, 5000.0, 0.7)
        info = bs.plan_info()
        assert info['tile_atoms'] == cap and info['lanes'] == (64 if cap <= 64 else 128 if cap <= 128 else 256)
        outs.append((rd, vd, info['tiles']))
    labels = system()[5]
    assert [o[2] for o in outs] == [plan_restated(labels, cap)['n_tiles'] for cap in (6, 7, 64, 100, 256, 256)]
    assert outs[0][2] >= 30 and outs[2][2] >= 4 and outs[3][2] >= 3 and outs[4][2] == 1
    for rd, vd, _ in outs[1:]:
        assert torch.equal(rd, outs[0][0]) and torch.equal(vd, outs[0][1])
    assert not torch.equal(outs[0][0], make(owner)[1])


# ---- 4. singleton groups ------------------------------------------------------------------------------------------------
def test_singleton_groups_are_the_atomic_barostat(owner):
    """1000 free atoms (no multiple of 256, four tiles): the sums are those of CRescaleBarostat under the sums bar, one
    application is admp_md_scale to 4 eps"""
    from admp_amd.md import CRescaleBarostat, MolecularCRescaleBarostat
    n, seed = 1000, 9
    eps = eps_of(owner)
    mass, r, v, g = sums_case(owner, n, 5)
    box = np.eye(3) * 20.8
    par = (5.0, 300.0, 1.0, 500.0, 4.5e-5, seed)
    mol = MolecularCRescaleBarostat(owner, mass, np.arange(n)[::-1].copy(), *par)
    atomic = CRescaleBarostat(owner, mass, *par)
    assert mol.plan_info()['tiles'] == 4 and mol.plan_info()['groups'] == n
    kin_m, rg_m, xi_m = mol.sums(r, v, g, box)
    kin_a, rg_a, xi_a = atomic.sums(r, v, g)
    m = 1.0 / host(mol.inv_mass)
    vh, rh, gh = host(v), host(r), host(g)
    kin_abs = _ext(np.abs((vh[:, :, None] * vh[:, None, :]) * m[:, None, None]).reshape(-1, 9)) / ACC
    rg_abs = _ext(np.abs(rh[:, :, None] * gh[:, None, :]).reshape(-1, 9))
    print('kin %.2e of %.2e, rg %.2e of %.2e' % (np.abs(kin_m - kin_a).max(), 64 * E64 * kin_abs.min(), np.abs(rg_m - rg_a).max(),
                                                 64 * E64 * rg_abs.min()))
    assert xi_m == xi_a
    assert (np.abs(kin_m - kin_a) <= 64 * E64 * kin_abs).all() and (np.abs(rg_m - rg_a) <= 64 * E64 * rg_abs).all()
    r2, v2, box2 = r.clone(), v.clone(), box.copy()
    mu_m = mol.apply(r, v, box, 900.0, xi_m)
    mu_a = atomic.apply(r2, v2, box2, 900.0, xi_a)
    assert mu_m == mu_a and np.array_equal(box, box2) and mu_m != 1.0
    assert np.abs(host(r) - host(r2)).max() <= 4 * eps * np.abs(rh).max()
    assert np.abs(host(v) - host(v2)).max() <= 4 * eps * np.abs(vh).max()


# ---- 5. bonded terms under molecular scaling ----------------------------------------------------------------------------
@pytest.mark.parametrize('cell', ['cubic', 'triclinic'])
def test_bonded_strain_derivative_vanishes(owner, cell):
    """HarmonicBonded alone on 64 wrapped, perturbed waters with molecules across faces: molecular scaling moves molecules
    rigidly, so sum box . dE/dbox + sum R_c(i) . g_i = 0 -- to the project's bars for box gradients (1e-8 f64, 5e-4 f32) times
    sum |R_c(i)| |g_i|.  The atomic sum r_i . g_i does not cancel it, and a wrong image of a centre breaks it"""
    import torch
    from admp_amd.md import HarmonicBonded, MolecularCRescaleBarostat, groups_of
    pos, box, unwrapped, lists, n_cross, e_ref, ref = bonded_case(cell)
    f64 = eps_of(owner) < 1e-10
    f = HarmonicBonded(len(pos), *lists)
    groups = groups_of(len(pos), bonded=f)
    assert np.array_equal(groups, 3 * (np.arange(len(pos)) // 3))
    p = dev(f, pos)
    g = torch.zeros_like(p)
    f.add_forces(p, box, g)
    dbox = f.get_box_gradient(pos, box)
    bs = MolecularCRescaleBarostat(f, np.tile(MASS, len(pos) // 3), groups, 5.0, 300.0, 1.0, 500.0, 4.5e-5, 1)
    kin, rg, _ = bs.sums(p, torch.zeros_like(p), g, box)
    q = mol_restated(host(p), np.zeros_like(pos), host(bs.inv_mass), groups, box)
    scale = float((np.linalg.norm(q['Rc'], axis=1) * np.linalg.norm(host(g), axis=1)).sum())
    total = float((box * dbox).sum() + np.trace(rg))
    atomic = float((box * dbox).sum() + (host(p) * host(g)).sum())
    print('%s: sum box.dE/dbox %.6f + sum R_c(i).g_i %.6f = %.3e of %.3e; with r_i.g_i instead %.3e'
          % (cell, (box * dbox).sum(), np.trace(rg), total, (1e-8 if f64 else 5e-4) * scale, atomic))
    assert not kin.any() and n_cross >= 1 and (np.abs(q['s']).sum(1) > 0).any()
    assert abs((box * dbox).sum()) > 1.0
    assert abs(total) <= (1e-8 if f64 else 5e-4) * scale
    # without the images s_i the sum misses by the box-gradient term
    wrong = float((box * dbox).sum() + ((q['Rc'] - q['s']) * host(g)).sum())
    print('without the images: %.3e' % wrong)
    assert abs(wrong) > 1.0 and abs(wrong) > 100 * abs(total)
    if f64:
        assert abs(wrong) > 1e-8 * scale


# ---- 6. the pressure convention against finite differences --------------------------------------------------------------
def molecular_strain_derivative(pol, thresh, delta=6e-4):
    """(molecular dE/d eps, atomic dE/d eps, central difference at delta, at 2 delta) of the four calculators of water_md on 64
    wrapped waters with the set-up of tests/test_gpu_md_barostat.py strain_derivative; the scaled positions r_i + (mu - 1)
    R_c(i) are formed here in numpy float64, not by the kernel"""
    import torch
    from admp_amd import settings
    from admp_amd.md import CRescaleBarostat, MolecularCRescaleBarostat, groups_of
    old = (settings.PRECISION, settings.POL_CONV, settings.MAX_N_POL)
    try:
        w = water_setup(pol, thresh)
        box = w.box
        box0 = box.copy()
        pos0 = torch.remainder(w.pos + 0.125 * float(box[0, 0]) + 0.05 * torch.as_tensor(np.random.default_rng(9).normal(size=tuple(w.pos.shape)),
                                                              dtype=w.pos.dtype, device=w.pos.device), float(box[0, 0])).contiguous()
        d = host(pos0)
        assert (np.linalg.norm(d[1::3] - d[0::3], axis=1) > 2.0).any()          # molecules straddle the faces
        masses = np.tile(MASS, w.n_mol)
        groups = groups_of(3 * w.n_mol, bonded=w.bond)
        centres = mol_restated(d, np.zeros_like(d), 1.0 / masses, groups, box0)['Rc']
        w.nbl.allocate(pos0)

        def energy(mu):
            box[:] = box0 * mu
            p = torch.as_tensor(d + (mu - 1.0) * centres, dtype=pos0.dtype, device=pos0.device).contiguous()
            e123, _ = w.forces(p, None)
            e = w.epot_now(e123)
            box[:] = box0
            return e
        e123, grad = w.forces(pos0, None)
        dbox = w.box_gradient(pos0, None)
        zero = torch.zeros_like(pos0)
        mol = MolecularCRescaleBarostat(w.pme, masses, groups, 5.0, 300.0, 1.0, 1000.0, 4.5e-5, 1)
        kin, rg, _ = mol.sums(pos0, zero, grad.contiguous(), box0)
        assert not kin.any()
        vol = abs(np.linalg.det(box0))
        dE = -mol.pressure(box0, dbox, kin, rg) * vol / BAR
        atomic = CRescaleBarostat(w.pme, masses, 5.0, 300.0, 1.0, 1000.0, 4.5e-5, 1)
        _, rg_a, _ = atomic.sums(pos0, zero, grad.contiguous())
        dE_atomic = -atomic.pressure(box0, dbox, kin, rg_a) * vol / BAR
        fd = [(energy(np.exp(k * delta / 3.0)) - energy(np.exp(-k * delta / 3.0))) / (2.0 * k * delta) for k in (1, 2)]
        return dE, dE_atomic, fd[0], fd[1]
    finally:
        settings.PRECISION, settings.POL_CONV, settings.MAX_N_POL = old


@pytest.mark.parametrize('pol', [False, True])
def test_pressure_against_finite_differences_under_the_molecular_map(pol):
    """f64, fixed multipoles and polarizable (POL_CONV 1e-6, as the atomic test): dE/d eps = (sum box . dE/dbox + sum R_c(i) .
    g_i) / 3 against the central difference of the total energy, bonded terms included, with whole molecules translated, at mu
    = exp(+-delta / 3), delta = 6e-4, to 2e-4 of |dE/d eps| (the bar of the existing finite-difference tests).  The atomic and
    the molecular derivative differ by more than that bar (the bonded terms' share), or the case would show nothing"""
    dE, dE_atomic, fd1, fd2 = molecular_strain_derivative(pol, POL_CONV_FD if pol else 1e-2)
    print('molecular dE/d eps %.8f (atomic %.8f), central differences %.8f (delta) %.8f (2 delta): rel %.2e, delta against 2 delta '
          '%.2e, atomic against molecular %.2e' % (dE, dE_atomic, fd1, fd2, abs(fd1 - dE) / abs(dE), abs(fd1 - fd2) / abs(dE),
                                                  abs(dE_atomic - dE) / abs(dE)))
    assert abs(dE_atomic - dE) > 2e-4 * abs(dE)
    assert abs(fd1 - fd2) < 2e-4 * abs(dE)
    assert abs(fd1 - dE) <= 2e-4 * abs(dE)


# ---- 7. ideal gas of rigid dimers ---------------------------------------------------------------------------------------
GAS = dict(n_mol=4096, T=300.0, dt=1.0, gamma=0.05, P0=1.0, steps=3000, seed=5, m=(15.999, 1.008), d=1.0)
LNV_MOMENTUM = 4.0e-15      # what the rounding of the constraint updates may add (derived in the test's doc string)


def lnv_bar():
    """10 x the largest |ln V| difference between the restatement's two summation orders, computed here (3.553e-15 when this
    was written), plus LNV_MOMENTUM"""
    spread = float(np.abs(gas_restatement(0) - gas_restatement(1)).max())
    assert 0.0 < spread < 1e-13, spread
    return 10.0 * spread + LNV_MOMENTUM, spread


def gas_start():
    g = GAS
    mass = np.tile(g['m'], g['n_mol'])
    v0 = normals(2 * g['n_mol'], g['seed'], 0, 1) * np.sqrt(ACC * KB * g['T'] / mass)[:, None]
    v_eq = g['n_mol'] * KB * g['T'] * BAR / g['P0']
    return mass, v0, (1.3 * v_eq) ** (1.0 / 3.0), v_eq


@functools.lru_cache(maxsize=None)
def gas_restatement(order):
    """float64 numpy restatement: the gas of the dimers' centres.  Constraint impulses act along the bond with opposite
    momenta, so the group velocity V_c = sum m v / M follows BAOAB with zero gradients and the mass-weighted noise of the
    same generator, V_c <- c1 V_c + sqrt((1 - c1^2) kB T 1e-4) sum_i sqrt(m_i) xi_i / M; 2 K_com = sum M V_c^2 in one of two
    summation orders; the barostat's formulas with beta_T = 1 / P0, tau_p = 20 dt, every step.  Returns ln V after every step."""
    g = GAS
    mass, v0, L, _ = gas_start()
    n, M = g['n_mol'], float(sum(g['m']))
    vc = (mass[:, None] * v0).reshape(n, 2, 3).sum(1) / M
    c1 = np.exp(-g['gamma'] * g['dt'])
    amp = np.sqrt((1.0 - c1 * c1) * KB * g['T'] * ACC) * np.sqrt(mass)[:, None] / M
    beta, tau, dt = 1.0 / g['P0'], 20.0 * g['dt'], g['dt']
    box = np.eye(3) * L
    lnv = np.empty(g['steps'])
    for s in range(g['steps']):
        vc = c1 * vc + (amp * normals(2 * n, g['seed'], s, 0)).reshape(n, 2, 3).sum(1)
        terms = M * vc * vc
        two_k = (terms.sum() if order == 0 else terms[::-1].sum(axis=1).sum()) / ACC
        vol = abs(np.linalg.det(box))
        p = two_k / 3.0 / vol * BAR
        xi = normals(1, g['seed'], s, 2)[0, 0]
        d_eps = beta / tau * (p - g['P0']) * dt + np.sqrt(2.0 * KB * g['T'] * BAR * beta * dt / (vol * tau)) * xi
        mu = np.exp(d_eps / 3.0)
        vc, box = vc / mu, box * mu
        lnv[s] = np.log(abs(np.linalg.det(box)))
    return lnv


def test_gas_of_rigid_dimers_follows_the_restatement_and_sits_at_the_volume(owner):
    """4096 rigid dimers (d = 1 A, masses 15.999 and 1.008), zero gradients, cubic cell, ConstrainedLangevin (friction dt =
    0.05) and the molecular barostat every step with beta_T = 1/P0, tau_p = 20 dt, 3000 steps from V0 = 1.3 N_mol kB T / P0 (P0
    = 1 bar, 300 K: N_mol kB T / P0 = 1.696541e8 A^3).  A dimer has five degrees of freedom, of which the pressure may count the
    three of its centre: the volume of an ideal gas of N_mol rigid molecules is N_mol kB T / P0.  The atomic estimator (2 K over
    all atoms, no constraint virial) would sit at 5/3 of that and counting 3 N = 6 N_mol degrees of freedom at twice that:
    both leave the band by far.

    The restatement (gas_restatement, float64 numpy, deterministic, seed 5): V / (N_mol kB T / P0) = 1.2825, 1.0162, 0.9726,
    0.9812 after steps 0, 100, 300, 1000; over the last 2000 steps std V / mean V = 1.352e-2 (1 / sqrt N_mol = 1.5625e-2) and
    mean V sits -3.98e-4 below N_mol kB T / P0, 0.18 of sigma = 1 / sqrt(50 N_mol) = 2.21e-3 (n_eff = 2000 dt / 2 tau_p = 50):
    inside 2.5 sigma, so the analytic centre stands (seeds 1, 2, 3: +1.05, +0.54, -0.01 sigma).  Both handles: mean V of the
    last 2000 steps within 5 / sqrt(50 N_mol) = 1.105e-2 of N_mol kB T / P0.

    ln V on the f64 handle.  Summing M V_c^2 in two orders moves the restatement's ln V by at most 3.553e-15 over the 3000
    steps (the dynamics of the centres are linear: rounding is not amplified).  The constraints add nothing in exact
    arithmetic, whatever the tolerance: every SHAKE / RATTLE update gives the two atoms -+(g / m_i) s, opposite momenta.  In
    floating point each product g / m_i rounds, so an update may change a dimer's momentum by eps m_H |dv| with |dv| <= 2e-2
    A/fs (the thermal speed of the hydrogen), against M |V_c| = 17 x 6.6e-3: 0.18 eps; at most ten updates per step (two
    half steps, up to five sweeps at tolerance 1e-12) and a memory of 1 / (friction dt) = 20 steps give 10 x 0.18 x sqrt(20) = 8
    eps per dimer if the signs are random and every dimer errs the same way (no cancellation over the 4096), 16 eps on K_com
    and, with beta_T = 1 / P0, on ln V: 4e-15.  The bar is 10 x that spread (lnv_bar computes it) + 4e-15 = 3.95e-14 at every step; the device's share
    is printed (measured: 3.553e-15 on the f64 handle, 4.9e-7 on the f32 one, which is not held to the bar).  No constraint failures; the largest constraint error at the end within
    the stop rule, tolerance + 4 eps |r| / d."""
    import torch
    from admp_amd.md import ConstrainedLangevin, Constraints, MolecularCRescaleBarostat, groups_of
    g = GAS
    n = g['n_mol']
    mass, v0, L, v_eq = gas_start()
    ref = gas_restatement(0)
    bar, spread = lnv_bar()
    pairs = np.stack([2 * np.arange(n), 2 * np.arange(n) + 1], axis=1)
    tol = tol_of(owner)
    c = Constraints(2 * n, pairs, np.full(n, g['d']), mass, tolerance=tol)
    rng = np.random.default_rng(3)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    grid = (np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing='ij'), axis=-1).reshape(-1, 3) + 0.5) * (L / 16.0)
    r0 = np.stack([grid, grid + g['d'] * u], axis=1).reshape(-1, 3)
    r, v = dev(c, r0), dev(c, v0)
    grad = torch.zeros_like(r)
    box = np.eye(3) * L
    c.project_velocities(r, v, box, g['dt'])
    c.reset_failures()
    integ = ConstrainedLangevin(c, g['dt'], g['T'], g['gamma'], g['seed'])
    groups = groups_of(2 * n, constraints=c)
    assert np.array_equal(groups, 2 * (np.arange(2 * n) // 2))
    bs = MolecularCRescaleBarostat(c, mass, groups, g['dt'], g['T'], g['P0'], 20.0 * g['dt'], 1.0 / g['P0'], g['seed'])
    zero = np.zeros((3, 3))
    lnv = np.empty(g['steps'])
    for s in range(g['steps']):
        integ.kick_drift(r, v, grad, box)
        integ.kick(r, v, grad, box)
        kin, rg, xi = bs.sums(r, v, grad, box)
        bs.apply(r, v, box, bs.pressure(box, zero, kin, rg), xi)
        lnv[s] = np.log(abs(np.linalg.det(box)))
    assert bs.step == g['steps'] and integ.step == g['steps']
    dev_max = np.abs(lnv - ref).max()
    mean_v = np.exp(lnv[-2000:]).mean()
    band = 5.0 / np.sqrt(50.0 * n)
    ce = constraint_errors(Con(2 * n, pairs, np.full(n, g['d'])), host(r), box).max()
    ce_bar = tol + 4 * eps_of(owner) * np.abs(host(r)).max() / g['d']
    print('max |ln V - restatement| %.3e (bar %.2e on the f64 handle); mean V / centre - 1 = %+.4e (band %.4e); constraint error '
          '%.3e of %.3e, failures %d, most sweeps %d' % (dev_max, bar, mean_v / v_eq - 1.0, band, ce, ce_bar, c.failures(),
                                                         c.max_sweeps_seen()))
    if eps_of(owner) < 1e-10:
        assert dev_max <= bar
    assert abs(mean_v / v_eq - 1.0) <= band
    assert c.failures() == 0 and ce <= ce_bar


# ---- 8. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(owner):
    """bad tensors, a wrong number of labels, a negative label and a group above the capacity are refused in Python before any
    launch; a call without a plan, another n_atoms, n < 0 and a factor that is zero or no number are the library's argument
    error, with nothing launched"""
    import torch
    from admp_amd.md import HarmonicBonded, MolecularCRescaleBarostat
    n = 12
    mass = np.tile(MASS, n // 3)
    groups = np.repeat(np.arange(4), 3)
    par = (5.0, 300.0, 1.0, 1000.0, 4.5e-5, 1)
    bs = MolecularCRescaleBarostat(owner, mass, groups, *par)
    good = lambda: torch.ones((n, 3), dtype=owner._dtype, device=owner._device)      # noqa: E731
    other = torch.float32 if owner._dtype == torch.float64 else torch.float64
    bad = [torch.zeros((n, 3), dtype=other, device=owner._device),                       # wrong precision
           torch.zeros((n, 6), dtype=owner._dtype, device=owner._device)[:, :3],         # non-contiguous view
           torch.zeros((n + 3, 3), dtype=owner._dtype, device=owner._device),            # wrong length
           torch.zeros((n, 3), dtype=owner._dtype)]                                      # host tensor
    box = np.eye(3) * 10.0
    for b in bad:
        for slot in range(3):
            args = [good(), good(), good()]
            args[slot] = b
            with pytest.raises(ValueError):
                bs.sums(*args, box)
            if slot < 2:
                with pytest.raises(ValueError):
                    bs.apply(args[0], args[1], box, 1.0, 0.0)
    with pytest.raises(ValueError):
        bs.apply(good(), good(), np.eye(3, dtype=np.float32) * 10.0, 1.0, 0.0)          # cannot be scaled in place as double
    for p_inst in (float('inf'), float('nan')):
        with pytest.raises(ValueError):
            bs.apply(good(), good(), box, p_inst, 0.0)
    assert bs.step == 0 and np.array_equal(box, np.eye(3) * 10.0)
    for labels, words in ((groups[:-1], 'group labels for 12 atoms'), (np.arange(n + 1), 'group labels for 12 atoms'),
                          (np.where(np.arange(n) == 5, -3, groups), 'atom 5 has the negative group label -3'),
                          (groups.astype(np.float64), '32-bit integers'), (groups.reshape(4, 3), 'group labels for 12 atoms')):
        with pytest.raises(ValueError, match=words):
            MolecularCRescaleBarostat(owner, mass, labels, *par)
    with pytest.raises(ValueError, match=r'a group of 3 atoms \(smallest atom 0\) exceeds tile_atoms 2'):
        MolecularCRescaleBarostat(owner, mass, groups, *par, tile_atoms=2)
    with pytest.raises(ValueError, match=r'a group of 5 atoms \(smallest atom 1\) exceeds tile_atoms 4'):
        MolecularCRescaleBarostat(owner, mass, [0, 7, 7, 7, 1, 1, 7, 2, 2, 2, 7, 3], *par, tile_atoms=4)
    for cap in (0, -1, 257, 2.5):
        with pytest.raises(ValueError, match='tile_atoms'):
            MolecularCRescaleBarostat(owner, mass, groups, *par, tile_atoms=cap)
    for kw in (dict(temperature=-1.0), dict(tau_p_fs=0.0), dict(compressibility_per_bar=-1e-5)):
        a = dict(dt_p_fs=5.0, temperature=300.0, pressure_bar=1.0, tau_p_fs=1000.0, compressibility_per_bar=4.5e-5, seed=1)
        a.update(kw)
        with pytest.raises(ValueError):
            MolecularCRescaleBarostat(owner, mass, groups, **a)
    # the library's own checks
    bs = MolecularCRescaleBarostat(owner, mass, groups, *par)      # (the refused plans above left the last valid one in place)
    L, h, P = owner._L, owner._h, owner._ptr
    r, v, gr = good(), good(), good()
    out = torch.zeros(21, dtype=torch.float64, device=owner._device)
    cell = (ctypes.c_double * 9)(*(np.eye(3) * 10.0).ravel())
    flat = (ctypes.c_double * 9)(10.0, 0, 0, 0, 10.0, 0, 10.0, 10.0, 0)                 # singular
    nan_cell = (ctypes.c_double * 9)(10.0, 0, 0, 0, float('nan'), 0, 0, 0, 10.0)
    launches = bs.plan_info()['launches']
    a, b = float(np.expm1(1e-3)), float(np.expm1(-1e-3))
    for m1, m2 in ((-1.0, 1.0), (float('nan'), b), (a, float('nan')), (float('inf'), -1.0), (a, float('inf')), (-2.0, -2.0), (a, a)):
        assert L.admp_md_mol_scale(h, n, P(r), P(v), P(bs.inv_mass), cell, m1, m2) == E_ARG, (m1, m2)
    for n_bad in (-1, 0, n - 3, n + 3):
        assert L.admp_md_mol_scale(h, n_bad, P(r), P(v), P(bs.inv_mass), cell, a, b) == E_ARG
        assert L.admp_md_mol_sums(h, n_bad, P(r), P(v), P(gr), P(bs.inv_mass), cell, 1, 0, P(out)) == E_ARG
        assert b"n_atoms differs from the plan's" in L.admp_last_error(h)
    for bad_cell in (flat, nan_cell, None):
        assert L.admp_md_mol_scale(h, n, P(r), P(v), P(bs.inv_mass), bad_cell, a, b) == E_ARG
        assert L.admp_md_mol_sums(h, n, P(r), P(v), P(gr), P(bs.inv_mass), bad_cell, 1, 0, P(out)) == E_ARG
    assert L.admp_md_mol_scale(h, n, None, P(v), P(bs.inv_mass), cell, a, b) == E_ARG
    assert L.admp_md_mol_sums(h, n, P(r), P(v), None, P(bs.inv_mass), cell, 1, 0, P(out)) == E_ARG
    assert L.admp_md_mol_sums(h, n, P(r), P(v), P(gr), P(bs.inv_mass), cell, 1, 0, None) == E_ARG
    lab = np.ascontiguousarray(groups, dtype=np.int32)
    assert L.admp_md_mol_plan(h, 0, lab.ctypes.data, 0) == E_ARG and L.admp_md_mol_plan(h, n, None, 0) == E_ARG
    assert L.admp_md_mol_plan(h, n, lab.ctypes.data, 257) == E_ARG and b'tile_atoms 257 outside 1..256' in L.admp_last_error(h)
    assert L.admp_md_mol_info(h, None) == E_ARG
    # a handle without a plan
    fresh = HarmonicBonded(3, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 2)))
    assert fresh._L.admp_md_mol_scale(fresh._h, n, P(r), P(v), P(bs.inv_mass), cell, a, b) == E_ARG
    assert b'admp_md_mol_plan must precede admp_md_mol_scale' in fresh._L.admp_last_error(fresh._h)
    assert fresh._L.admp_md_mol_sums(fresh._h, n, P(r), P(v), P(gr), P(bs.inv_mass), cell, 1, 0, P(out)) == E_ARG
    assert b'admp_md_mol_plan must precede admp_md_mol_sums' in fresh._L.admp_last_error(fresh._h)
    info = (ctypes.c_int64 * 8)()
    assert fresh._L.admp_md_mol_info(fresh._h, info) == 0 and not any(info)
    torch.cuda.synchronize()
    assert torch.equal(r, good()) and torch.equal(v, good()) and not out.any()          # nothing was launched
    assert bs.plan_info()['launches'] == launches
    # and the plan still serves
    kin, rg, xi = bs.sums(r, v, gr, box)
    assert np.isfinite(kin).all() and np.isfinite(rg).all() and bs.plan_info()['launches'] == launches + 1


def test_two_barostats_share_a_handle(owner):
    """the handle keeps one plan: a barostat whose plan another one has replaced plans again before its next launch; a
    Constraints can hold the constraint plan and the molecular plan at once"""
    import torch
    from admp_amd.md import Constraints, MolecularCRescaleBarostat, groups_of
    r, v, g, mass, con, labels = system()
    a, rd, vd, gd = make(owner)
    first = a.sums(rd, vd, gd, BOX)
    b = MolecularCRescaleBarostat(owner, mass, np.arange(len(r)), 5.0, 300.0, 1.0, 500.0, 4.5e-5, a.seed)
    assert b.plan_info()['groups'] == len(r)
    second = a.sums(rd, vd, gd, BOX)
    assert a.plan_info()['groups'] == 72
    # the same plan on the same inputs, made twice: each under the module's sums bar, and so is their difference
    ty = np_ty(owner)
    kin_ref, rg_ref, kin_abs, rg_abs = sums_restated(*[host(t).astype(ty) for t in (rd, vd, gd, a.inv_mass)], labels, BOX, ty)
    assert (np.abs(first[0] - second[0]) * ACC <= 64 * E64 * kin_abs).all() and (np.abs(first[1] - second[1]) <= 64 * E64 * rg_abs).all()
    assert first[2] == second[2]
    c = Constraints(len(r), con.pairs, con.lengths, mass)
    on_c = MolecularCRescaleBarostat(c, mass, groups_of(len(r), constraints=c), 5.0, 300.0, 1.0, 500.0, 4.5e-5, a.seed)
    rc, vc = dev(c, r), dev(c, v)
    box = BOX.copy()
    on_c.apply(rc, vc, box, 5000.0, 0.7)
    c.project_velocities(rc, vc, box)                                   # the constraint plan is still there
    assert c.plan_info()['clusters'] == 72 and on_c.plan_info()['groups'] == 72 and c.failures() == 0
    assert torch.isfinite(rc).all() and torch.isfinite(vc).all()


# ---- 9. the driver ------------------------------------------------------------------------------------------------------
RIGID_ARGS = ['--waters', '216', '--steps', '100', '--minimize', '60', '--nbaro', '5', '--log', '5', '--friction', '0.05', '--rigid']
RIGID_LINE = re.compile(LOG_LINE.pattern + r' +constraints +(\S+)')


@functools.lru_cache(maxsize=None)
def rigid_run(pol, pressure):
    out = run_driver('npt_water.py', *RIGID_ARGS, '--pressure', repr(pressure), *(['--pol'] if pol else []))
    rows = np.array([[float(x) for x in m.groups()] for m in RIGID_LINE.finditer(out)])
    m = re.search(r'V_final ([-+0-9.e]+) A\^3', out)
    f = re.search(r'tolerance ([-+0-9.e]+), no re-projection in the loop\); most sweeps of a cluster (\d+); failures (\d+)', out)
    assert m and f and len(rows) == 20, out[-1500:]
    print(out.splitlines()[-1])
    return rows, float(m.group(1)), float(f.group(1)), int(f.group(3)), out


@pytest.mark.parametrize('pol', [False, True])
def test_npt_rigid_water_runs_holds_the_temperature_and_the_constraints(pol):
    """216 rigid waters, f64, 100 steps of 2 fs after the short minimisation, the molecular barostat every 5: every logged
    figure finite, the mean kinetic temperature of the second half (over the constrained degrees of freedom) within the band
    of test_npt_water_runs_and_holds_the_temperature, the largest constraint error right after every logged application
    within the stop rule of the tolerance (tolerance + 4 eps |r| / d) with no re-projection in the loop, no failures"""
    rows, v_final, tol, failures, out = rigid_run(pol, 1.0)
    assert np.isfinite(rows).all() and np.isfinite(v_final) and 'ns/day' in out and 'dt 2.00 fs' in out
    assert (rows[:, 4] > 0).all() and (rows[:, 5] > 0.5).all() and (rows[:, 5] < 1.5).all()
    tk = rows[rows[:, 0] >= 50, 2]
    assert abs(tk.mean() / 300.0 - 1.0) <= BAND, out[-1500:]
    assert tol == 1e-8 and failures == 0
    assert (rows[:, 6] <= tol + 4 * 2.0 ** -52 * 30.0 / 0.9572).all(), rows[:, 6]


def test_npt_rigid_water_higher_pressure_smaller_volume():
    """the same seed at 1 and 10 001 bar: both runs draw the same noise; the drift alone gives ln(V_low / V_high) = beta_T dP
    t / tau_p = 4.5e-5 * 1e4 * 200 / 1000 = 0.09"""
    _, v_low, _, _, _ = rigid_run(False, 1.0)
    _, v_high, _, _, _ = rigid_run(False, 10001.0)
    print('V %.4f at 1 bar, %.4f at 10001 bar: ln ratio %.5f (drift alone 0.09)' % (v_low, v_high, np.log(v_low / v_high)))
    assert v_high < v_low


def test_npt_flexible_water_with_molecular_scaling():
    """the flexible driver's arguments with --molecular: runs, every figure finite, the temperature in the band"""
    out = run_driver('npt_water.py', *NPT_ARGS, '--molecular')
    rows = np.array([[float(x) for x in m.groups()] for m in LOG_LINE.finditer(out)])
    assert len(rows) >= 4 and np.isfinite(rows).all() and 'molecular scaling: 216 groups' in out, out[-1500:]
    tk = rows[rows[:, 0] >= 50, 2]
    assert abs(tk.mean() / 300.0 - 1.0) <= BAND, out[-1500:]
