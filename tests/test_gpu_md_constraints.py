"""Distance constraints on the GPU (admp_amd.md.Constraints / ConstrainedLangevin; admp_md_con_plan / _step / _kick / _project,
con_kernels.hip) against the float64 numpy restatement of the scheme in tests/test_con_plan_cpu.py, under that module's bar
rule (16 x the float32 restatement's deviation from the float64 one, x 2^-29 in double, plus the stop-rule allowance 4 tol d_max
on positions and 4 tol d_max / dt on velocities; the float32 restatement, being only the yardstick, runs at tol 1e-6); both
precisions, double with tol 1e-12 and single with tol 1e-6.

Standard system: the 64 waters and 5 free atoms of tests/test_gpu_md_mts.py with the waters made rigid, two 5-atom stars and a
6-atom chain on top (213 atoms, 207 constraints, 72 clusters), triclinic cell, atom order shuffled, six molecules wrapped across
the six faces and one across a corner; 300 K, friction 0.05 / fs, seed 11, starting at step 3.  The slow force is the harmonic
tether to the start positions (k = 20 kJ/mol/A^2), computed with torch between the two halves of a step."""
import functools

import numpy as np
import pytest

from tests.test_con_plan_cpu import (CROSSINGS, Con, con_bars, constraint_errors, kick_restated, plan_restated, project_restated,
                                     rigid_system, step_restated, vectors)
from tests.test_gpu_md_mts import GAMMA, K_TETHER, NVE_SEED, SEED, START, T0, dev, eps_of, host, prec, run_driver      # noqa: F401
from tests.test_mts_plan_cpu import ACC, BOX, KB, bars

pytestmark = pytest.mark.gpu

DT = 2.0


def tol_of(o):
    return 1e-12 if eps_of(o) < 1e-10 else 1e-6


@functools.lru_cache(maxsize=None)
def system():
    s = rigid_system(64, 5, 7)
    r, v, mass, con, wrapped = s
    assert len(r) == 213 and len(con.pairs) == 192 + 8 + 5 and len(con.comps) == 64 + 5 + 3
    for m, want in enumerate(CROSSINGS):      # a cluster across each face, and one across a corner
        assert all(axis in wrapped[m] for axis, _ in want), m
    assert any(len(w) == 3 for w in wrapped)
    raw = r[con.pairs[:, 1]] - r[con.pairs[:, 0]]
    assert (np.abs(raw - vectors(con, r, BOX)).max(axis=1) > 1.0).sum() >= 7      # those constraints span the cell
    assert np.abs(con.pairs[:, 0] - con.pairs[:, 1]).max() > 2                   # shuffled: clusters are not contiguous
    assert constraint_errors(con, r, BOX).max() < 1e-14
    return s


def make(s, **kw):
    """the Constraints of a system at the tolerance of its precision (known only once the handle exists)"""
    from admp_amd.md import Constraints
    r, v, mass, con, _ = s
    c = Constraints(len(r), con.pairs, con.lengths, mass, **kw)
    c.tolerance = tol_of(c)
    return c


@functools.lru_cache(maxsize=None)
def perturbed():
    r = system()[0]
    return r + np.random.default_rng(21).uniform(-0.05, 0.05, size=r.shape)


def cast(single, *arrays):
    return [a.astype(np.float32) if single else a for a in arrays]


def check(what, name, got, ref, single, is_double, tol, d_max, per_dt=None):
    bar, dev32 = con_bars(single, ref, is_double, tol, d_max, per_dt)
    d = np.abs(got - ref).max()
    print('%s: max|d%s| %.3e, bar %.3e (float32 restatement %.3e): share %.4f' % (what, name, d, bar, dev32, d / bar))
    assert d <= bar, (what, name)


def holds(con, o, r, tol):
    """every constraint within tol (+ 4 eps |r| / d: the rounding of r0 + delta, in double far below tol)"""
    err = constraint_errors(con, host(r), BOX).max()
    bar = tol + 4 * eps_of(o) * np.abs(host(r)).max() / con.lengths.min()
    print('largest constraint error %.3e of %.3e' % (err, bar))
    assert err <= bar


def per_cluster(con, q):
    """sum of q over the atoms of each cluster"""
    return np.array([q[c].sum(axis=0) for c in con.comps])


def test_project_positions(prec):
    """a configuration perturbed by 0.05 A per coordinate, projected along its own directions and along those of the start"""
    import torch
    s = system()
    r, v, mass, con, _ = s
    c = make(s)
    tol, im, dm = c.tolerance, 1.0 / mass, con.lengths.max()
    free = np.array([len(x) == 1 for x in con.comps])
    free_atoms = np.concatenate([x for x, f in zip(con.comps, free) if f])
    assert len(free_atoms) == 5 and constraint_errors(con, perturbed(), BOX).max() > 1e-2
    for name, along in (('itself', None), ('the start', r)):
        ref = project_restated(con, perturbed(), perturbed() if along is None else along, im, BOX, tol, 500)
        single = project_restated(con, *cast(True, perturbed(), perturbed() if along is None else along, im), BOX, max(tol, 1e-6), 500)
        p = dev(c, perturbed())
        p0 = p.clone()
        c.project_positions(p, BOX, ref=None if along is None else dev(c, along))
        holds(con, c, p, tol)
        check('projection along ' + name, 'r', host(p), ref[0], single[0], eps_of(c) < 1e-10, tol, dm)
        assert torch.equal(p[free_atoms], p0[free_atoms]) and not torch.equal(p, p0)
        # the centre of mass of a cluster: sum m delta = 0 but for the rounding of every update (eps |delta| each, at most
        # sweeps x constraints of them) and of r0 + delta (eps |r| / 2 per atom)
        moved = np.abs(per_cluster(con, mass[:, None] * (host(p) - host(p0)))).max(axis=1) / per_cluster(con, mass)
        bar = eps_of(c) * (np.abs(host(p)).max() + c.max_sweeps_seen() * con.sweep.shape[1] * 0.2)
        print('centre of mass moved by %.3e of %.3e; most sweeps %d' % (moved.max(), bar, c.max_sweeps_seen()))
        assert moved.max() <= bar and c.failures() == 0


def test_project_velocities(prec):
    import torch
    s = system()
    r, v, mass, con, _ = s
    c = make(s)
    tol, im, dm = c.tolerance, 1.0 / mass, con.lengths.max()
    v0 = v + np.random.default_rng(22).normal(size=v.shape) * np.sqrt(ACC * KB * T0 / mass)[:, None]
    ref = kick_restated(con, r, v0, None, im, BOX, DT, tol, 500)
    single = kick_restated(con, *cast(True, r, v0), None, im.astype(np.float32), BOX, DT, max(tol, 1e-6), 500)
    rd, vd = dev(c, r), dev(c, v0)
    c.project_velocities(rd, vd, BOX, dt_fs=DT)
    sv = vectors(con, host(rd), BOX)
    w = host(vd)[con.pairs[:, 1]] - host(vd)[con.pairs[:, 0]]
    share = np.abs((sv * w).sum(1)) * DT / (tol * con.d2)
    # evaluated here in double from the handle's numbers; printed next to it: what the rounding of s and of the differences in
    # the kernel's own dot product could amount to, 4 eps |s| |dv| (the assertion does not use it)
    slack = 4 * eps_of(c) * (np.sqrt((sv * sv).sum(1)) * np.sqrt((w * w).sum(1))) * DT / (tol * con.d2)
    print('|s.dv| dt / (tol d^2): largest %.4f (rounding of this evaluation: %.4f)' % (share.max(), slack.max()))
    assert np.all(share <= 1.0)
    check('velocity projection', 'v', host(vd), ref[0], single[0], eps_of(c) < 1e-10, tol, dm, DT)
    dp = np.abs(per_cluster(con, mass[:, None] * (host(vd) - host(dev(c, v0))))).max()
    bar = eps_of(c) * mass.max() * (np.abs(v0).max() + c.max_sweeps_seen() * con.sweep.shape[1] * np.abs(w).max())
    print('momentum of a cluster changed by %.3e of %.3e; most sweeps %d' % (dp, bar, c.max_sweeps_seen()))
    assert dp <= bar and c.failures() == 0 and not torch.equal(vd, dev(c, v0))


@functools.lru_cache(maxsize=None)
def restated(steps, single, gamma=GAMMA, constrained=True, tol=1e-12):
    """the scheme with the tether as the force, `steps` steps of 2 fs from START: (r, v) after the closing half"""
    r, v, mass, con, _ = system()
    if not constrained:
        con = Con(len(r), np.zeros((0, 2), dtype=int), np.zeros(0))
    r, v, im = cast(single, r, v, 1.0 / mass)
    ty = r.dtype.type
    rs, g = r.copy(), np.zeros_like(r)
    for k in range(steps):
        r, v, failed, _ = step_restated(con, r, v, g, im, BOX, DT, T0, gamma, SEED, START + k, tol, 500)
        g = ty(K_TETHER) * (r - rs)
        v, failed2, _, _ = kick_restated(con, r, v, g, im, BOX, DT, tol, 500)
        assert failed == 0 == failed2
    return r, v


def run_steps(c, integ, steps, each=None):
    s = system()
    r, v = dev(c, s[0]), dev(c, s[1])
    rs, g = r.clone(), dev(c, np.zeros_like(s[0]))
    for _ in range(steps):
        integ.kick_drift(r, v, g, BOX)
        g = (K_TETHER * (r - rs)).contiguous()
        integ.kick(r, v, g, BOX)
        if each:
            each(r, v)
    return r, v


@pytest.mark.parametrize('steps', [1, 3])
def test_steps_against_the_restatement(prec, steps):
    from admp_amd.md import ConstrainedLangevin
    s = system()
    con = s[3]
    c = make(s)
    tol, dm, is_double = c.tolerance, con.lengths.max(), eps_of(c) < 1e-10
    integ = ConstrainedLangevin(c, DT, T0, GAMMA, SEED)
    integ.step = START
    r, v = run_steps(c, integ, steps, each=lambda r, v: holds(con, c, r, tol))
    assert integ.step == START + steps and c.failures() == 0 and c.plan_info()['launches'] == 2 * steps
    ref, single = restated(steps, False, tol=tol), restated(steps, True, tol=max(tol, 1e-6))
    check('%d steps' % steps, 'r', host(r), ref[0], single[0], is_double, tol, dm)
    check('%d steps' % steps, 'v', host(v), ref[1], single[1], is_double, tol, dm, DT)
    assert np.abs(host(r) - s[0]).max() > 1e-3


def test_every_capacity_bit_identical(prec):
    """capacities 6 (the largest cluster), 7, 64 (one wavefront), 100 (two), 256 (four) and a second run: r and v bit-identical"""
    import torch
    from admp_amd.md import ConstrainedLangevin
    s = system()
    con = s[3]
    out = []
    for cap, lanes in ((6, 64), (7, 64), (64, 64), (100, 128), (256, 256), (None, 256), (64, 64)):
        c = make(s, tile_atoms=cap)
        info = c.plan_info()
        want = plan_restated(213, con.pairs, cap or 256)
        assert info['tiles'] == want['n_tiles'] and info['lanes'] == lanes and info['tile_atoms'] == (cap or 256)
        assert info['largest_cluster'] == 6 and info['atoms'] == 213 and info['constraints'] == 205 and info['clusters'] == 72
        integ = ConstrainedLangevin(c, DT, T0, GAMMA, SEED)
        integ.step = START
        out.append(run_steps(c, integ, 3))
        assert c.failures() == 0
    assert plan_restated(213, con.pairs, 6)['n_tiles'] > 36 and plan_restated(213, con.pairs, 256)['n_tiles'] == 1
    for r, v in out[1:]:
        assert torch.equal(r, out[0][0]) and torch.equal(v, out[0][1])
    with pytest.raises(ValueError, match='a cluster of 6 atoms'):
        make(s, tile_atoms=5)


def test_no_constraints_is_the_langevin_chain(prec):
    """an empty list: three steps within the bar of the restatement, of the existing Langevin chain on the same gradient, and
    the two of each other (the displacement form adds (dt/2) v twice to zero, the chain to r: roundings differ)"""
    from admp_amd.md import Constraints, ConstrainedLangevin, Langevin
    s = system()
    c = Constraints(213, np.zeros((0, 2)), np.zeros(0), s[2], tolerance=1e-6)
    assert c.n_constraints == 0 and c.plan_info()['clusters'] == 213 and c.plan_info()['tiles'] == 1
    is_double = eps_of(c) < 1e-10
    integ = ConstrainedLangevin(c, DT, T0, GAMMA, SEED)
    integ.step = START
    r, v = run_steps(c, integ, 3)
    ref, single = restated(3, False, constrained=False), restated(3, True, constrained=False, tol=1e-6)
    lv = Langevin(c, s[2], DT, T0, GAMMA, SEED)
    lv.step = START
    rc, vc = dev(c, s[0]), dev(c, s[1])
    rs, g = rc.clone(), dev(c, np.zeros_like(s[0]))
    for _ in range(3):
        lv.kick_drift(rc, vc, g)
        g = (K_TETHER * (rc - rs)).contiguous()
        lv.kick(rc, vc, g)
    for what, a, b in (('no constraints', (r, v), ref), ('chain', (rc, vc), ref), ('no constraints against the chain', (r, v), (host(rc), host(vc)))):
        for name, q in (('r', 0), ('v', 1)):
            bar, dev32 = bars(single[q], ref[q], is_double)
            d = np.abs(host(a[q]) - b[q]).max()
            print('%s: max|d%s| %.3e, bar %.3e: share %.4f' % (what, name, d, bar, d / bar))
            assert d <= bar, (what, name)
    assert c.failures() == 0 and c.max_sweeps_seen() == 0


@functools.lru_cache(maxsize=None)
def nve_case():
    """64 rigid waters with the tether, 100 steps of 2 fs at friction 0: the start and std(E_kin + E_tether) of the float64
    restatement's own run"""
    r, v, mass, con, _ = rigid_system(64, 0, NVE_SEED, extras=False)
    im = 1.0 / mass

    def energy(x, w):
        return 0.5 * K_TETHER * ((x - r) ** 2).sum() + 0.5 * (w ** 2 / im[:, None]).sum() / ACC
    x, w, g, e = r.copy(), v.copy(), np.zeros_like(r), []
    for k in range(100):
        x, w, f1, _ = step_restated(con, x, w, g, im, BOX, DT, 0.0, 0.0, SEED, k, 1e-12, 500)
        g = K_TETHER * (x - r)
        w, f2, _, _ = kick_restated(con, x, w, g, im, BOX, DT, 1e-12, 500)
        assert f1 == 0 == f2
        e.append(energy(x, w))
    return r, v, mass, con, energy, float(np.std(e))


def test_nve_energy_fluctuation(prec):
    """friction 0 is RATTLE velocity Verlet: std(E_kin + E_tether) over 100 steps of 2 fs, formed on the host in float64 from
    the device's r and v, is at most 2 x that of the float64 restatement's own run of the same scheme (both printed)"""
    from admp_amd.md import Constraints, ConstrainedLangevin
    r0, v0, mass, con, energy, std_ref = nve_case()
    c = Constraints(len(r0), con.pairs, con.lengths, mass)
    c.tolerance = tol_of(c)
    integ = ConstrainedLangevin(c, DT)
    assert integ.c1 == 1.0 and integ.c2sq_kT_acc == 0.0
    r, v = dev(c, r0), dev(c, v0)
    rs, g, e = r.clone(), dev(c, np.zeros_like(r0)), []
    for _ in range(100):
        integ.kick_drift(r, v, g, BOX)
        g = (K_TETHER * (r - rs)).contiguous()
        integ.kick(r, v, g, BOX)
        e.append(energy(host(r), host(v)))
    print('std(E): restatement %.5f kJ/mol, device %.5f (ratio %.3f); mean E %.2f' % (std_ref, np.std(e), np.std(e) / std_ref, np.mean(e)))
    assert np.std(e) <= 2.0 * std_ref and c.failures() == 0
    holds(con, c, r, c.tolerance)


def test_thermostat_counts_the_constrained_degrees_of_freedom(prec):
    """1024 rigid waters, no forces, friction 0.05 / fs, 2 fs, 300 steps: the mean of temperature() over steps 100 to 300 within
    5 sigma of the target, sigma = sqrt(2 / 6144) = 1.8 % (the scheme alone stays within 0.7 % on the CPU; 3 N degrees of
    freedom would read 33 % low)"""
    import torch
    from admp_amd.md import Constraints, ConstrainedLangevin
    r0, v0, mass, con, _ = rigid_system(1024, 0, 4, crossings=[], extras=False)
    c = Constraints(3072, con.pairs, con.lengths, mass, tolerance=1e-6)
    if eps_of(c) < 1e-10:
        c.tolerance = 1e-8
    integ = ConstrainedLangevin(c, DT, T0, GAMMA, 2)
    r, v = dev(c, r0), dev(c, v0)
    g, temps = torch.zeros_like(r), []
    for _ in range(300):
        integ.kick_drift(r, v, g, BOX)
        integ.kick(r, v, g, BOX, want_ekin=True)
        temps.append(integ.temperature())
    mean, sigma = np.mean(temps[100:]), np.sqrt(2.0 / 6144)
    print('mean T over steps 100-300: %.2f K = %.4f of the target (5 sigma = %.3f); with 3 N degrees of freedom %.4f; most sweeps %d'
          % (mean, mean / T0, 5 * sigma, mean / T0 * 6144 / 9216, c.max_sweeps_seen()))
    assert abs(mean / T0 - 1.0) <= 5 * sigma and c.failures() == 0
    assert integ.temperature(n_dof=9216) == pytest.approx(integ.temperature() * 6144 / 9216)
    holds(con, c, r, c.tolerance)


def test_one_sweep_counts_failures(prec):
    """max_sweeps = 1 on the perturbed configuration: failures() is the number of clusters the restatement leaves unconverged
    after one sweep, the outputs are finite, reset_failures() zeroes the counter"""
    import torch
    s = system()
    r, v, mass, con, _ = s
    c = make(s, max_sweeps=1)
    single = eps_of(c) > 1e-10
    want = project_restated(con, *cast(single, perturbed(), perturbed(), 1.0 / mass), BOX, c.tolerance, 1)
    assert want[1] == 67                                     # every cluster with a constraint
    p = dev(c, perturbed())
    c.project_positions(p, BOX)
    assert c.failures() == want[1] and c.max_sweeps_seen() == 1 and bool(torch.isfinite(p).all())
    vd = dev(c, v + np.random.default_rng(23).normal(size=v.shape) * 0.01)
    c.project_velocities(p, vd, BOX)
    assert c.failures() > want[1] and bool(torch.isfinite(vd).all())
    c.reset_failures()
    assert c.failures() == 0 and c.max_sweeps_seen() == 0


def test_refusals(prec):
    """each raises before anything is launched: the tensors, `step` and the launch count are untouched"""
    import torch
    from admp_amd import _lib
    from admp_amd.md import Constraints, ConstrainedLangevin
    s = system()
    r, v, mass, con, _ = s
    n = 213
    for pairs, lengths, match in (([(0, n)], [1.0], 'out of range'), ([(-1, 2)], [1.0], 'out of range'), ([(4, 4)], [1.0], 'itself'),
                                  ([(0, 1)], [0.0], 'positive and finite'), ([(0, 1)], [-1.0], 'positive and finite'),
                                  ([(0, 1)], [np.nan], 'positive and finite'), ([(0, 1)], [np.inf], 'positive and finite'),
                                  ([(0, 1), (1, 2)], [1.0], 'pairs for'), ([(0, 2 ** 31)], [1.0], 'out of range')):
        with pytest.raises(ValueError, match=match):
            Constraints(n, pairs, lengths, mass)
    with pytest.raises(ValueError, match=r'a cluster of 4 atoms \(smallest atom 2\)'):
        Constraints(9, [(6, 7), (5, 2), (2, 8), (8, 4)], np.ones(4), np.ones(9), tile_atoms=3)
    for kw in (dict(tile_atoms=0), dict(tile_atoms=257), dict(tolerance=-1e-6), dict(tolerance=np.nan), dict(max_sweeps=0),
               dict(max_sweeps=2.5)):
        with pytest.raises(ValueError):
            Constraints(n, con.pairs, con.lengths, mass, **kw)
    for m in (mass[:-1], np.where(np.arange(n) == 3, 0.0, mass), -mass):
        with pytest.raises(ValueError):
            Constraints(n, con.pairs, con.lengths, m)
    c = make(s)
    for args in ((c, 0.0), (c, -1.0), (c, DT, -1.0), (c, DT, T0, -0.1), (c, DT, T0, GAMMA, -1), (object(), DT)):
        with pytest.raises(ValueError):
            ConstrainedLangevin(*args)
    integ = ConstrainedLangevin(c, DT, T0, GAMMA, SEED)
    good = lambda: torch.ones((n, 3), dtype=c._dtype, device=c._device)      # noqa: E731
    other = torch.float32 if c._dtype == torch.float64 else torch.float64
    bad = [torch.ones((n, 3), dtype=other, device=c._device),                        # wrong precision
           torch.ones((n + 1, 3), dtype=c._dtype, device=c._device),                 # wrong shape
           torch.ones((n, 6), dtype=c._dtype, device=c._device)[:, :3],              # non-contiguous
           torch.ones((n, 3), dtype=c._dtype)]                                       # on the host
    kept = [good(), good(), good()]
    for b in bad:
        for slot in range(3):
            args = list(kept)
            args[slot] = b
            with pytest.raises(ValueError):
                integ.kick_drift(args[0], args[1], args[2], BOX)
            with pytest.raises(ValueError):
                integ.kick(args[0], args[1], args[2], BOX)
            if slot < 2:
                with pytest.raises(ValueError):
                    c.project_velocities(args[0], args[1], BOX)
                with pytest.raises(ValueError):
                    c.project_positions(args[0], BOX, ref=args[1])
    with pytest.raises(ValueError):
        c.project_velocities(kept[0], kept[1], BOX, dt_fs=0.0)
    P, L = c._ptr, c._L
    boxa = c._harr('box', BOX, 9)[0]
    step = lambda n_atoms, tol, sweeps, dt=DT: L.admp_md_con_step(c._h, n_atoms, P(kept[0]), P(kept[1]), P(kept[2]), P(c.inv_mass),      # noqa: E731
                                                                  boxa, 1e-4, dt, 1.0, 0.0, 1, 0, tol, sweeps, P(c.counters))
    kick = lambda n_atoms, tol, sweeps, g=None, hda=0.0: L.admp_md_con_kick(c._h, n_atoms, P(kept[0]), P(kept[1]), g, P(c.inv_mass),      # noqa: E731
                                                                            boxa, hda, DT, tol, sweeps, None, P(c.counters))
    proj = lambda n_atoms, tol, sweeps: L.admp_md_con_project(c._h, n_atoms, P(kept[0]), P(kept[0]), P(c.inv_mass), boxa, tol, sweeps,      # noqa: E731
                                                              P(c.counters))
    for f in (step, kick, proj):
        assert f(n + 1, 1e-6, 10) == -1 and f(-1, 1e-6, 10) == -1 and f(n, -1e-6, 10) == -1 and f(n, 1e-6, 0) == -1      # ADMP_E_ARG
        assert b'max_sweeps' in L.admp_last_error(c._h)
    assert step(n, 1e-6, 10, dt=0.0) == -1 and kick(n, 1e-6, 10, g=None, hda=1e-4) == -1
    fresh = Constraints(3, [(0, 1)], [1.0], np.ones(3))
    fresh_t = torch.ones((3, 3), dtype=c._dtype, device=c._device)
    _lib.check(fresh._h, L.admp_slab_configure(fresh._h, 0, 2), 'admp_slab_configure')      # a slab-decomposed handle
    with pytest.raises(_lib.AdmpHipError, match='single-rank'):
        fresh.project_positions(fresh_t, BOX)
    with pytest.raises(_lib.AdmpHipError, match='single-rank'):
        fresh.project_velocities(fresh_t, fresh_t.clone(), BOX)
    with pytest.raises(_lib.AdmpHipError, match='single-rank'):
        ConstrainedLangevin(fresh, DT).kick_drift(fresh_t, fresh_t.clone(), fresh_t.clone(), BOX)
    assert L.admp_md_con_plan(fresh._h, 3, 0, None, None, 0) != 0 and b'single-rank' in L.admp_last_error(fresh._h)
    torch.cuda.synchronize()
    assert integ.step == 0 and c.plan_info()['launches'] == 0 and fresh.plan_info()['launches'] == 0 and c.failures() == 0
    assert all(bool((t == 1).all()) for t in kept + [fresh_t])


# ---- the driver ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', [(), ('--bonds-only', '--pol')])
def test_driver(flags):
    """216 waters, 200 fs after the same short minimisation: rigid_water.py at 2 fs against nve_water.py at 0.5 fs (with --pol
    where the constrained run has it).  No failures, the largest constraint error within the tolerance printed, and the
    relative energy drift inside the bar of 4 x the NVE driver's own drift over the same simulated time."""
    import re
    common = ['--waters', '216', '--minimize', '60']
    d_con, out = run_driver('rigid_water.py', *common, '--steps', '100', *flags)
    m = re.search(r'largest constraint error ([-+0-9.e]+) \(tolerance ([-+0-9.e]+)\); failures (\d+)', out)
    assert m, out[-800:]
    print(m.group(0))
    assert int(m.group(3)) == 0 and 'failures 0' in out and float(m.group(1)) <= float(m.group(2)) and 'ns/day' in out
    d_nve, _ = run_driver('nve_water.py', *common, '--steps', '400', '--dt', '0.5', *[f for f in flags if f == '--pol'])
    print('drift: constrained %.3e, NVE driver %.3e, ratio %.2f' % (d_con, d_nve, abs(d_con) / abs(d_nve)))
    assert abs(d_con) <= 4.0 * abs(d_nve)
