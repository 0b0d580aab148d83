"""The stochastic velocity-rescaling thermostat on the GPU (admp_amd.md.VRescale; admp_md_vrescale = k_md_vr_sums +
k_md_vr_scale): the closing kick bit for bit against admp_md_kick_drift, one application against the float64 restatement of
tests/vrescale_ref.py at every size at which the grid changes shape and in both state slots, bitwise repeatability, a chain of
2000 applications, c = 0, rigid water, the conserved quantity against the energy error of plain velocity Verlet, the frozen
state, the refusals, and the drivers.  Both precisions wherever a handle is involved."""
import ctypes
import re

import numpy as np
import pytest

from tests import vrescale_ref as R
from tests.test_gpu_md_fire import K_ANG, K_BOND, R0, TH0, double_precision, water_geometry      # noqa: F401
from tests.test_gpu_md_langevin import E_ARG, MASS, dev, eps_of, host, owner, run_driver         # noqa: F401

pytestmark = pytest.mark.gpu

E_STATE = -5                                   # include/admp_hip.h ADMP_E_STATE
SIZES = [1, 255, 256, 257, 1000, 70001]        # 70 001 > 256 x 256: the stride loop and all 256 partial rows are live
U64 = 2.0 ** -53
#        K_before K_after alpha heat  applications tries reserved flags
USED = (3.1e-3, 2.9e-3, 0.97, -4.0e-3, 17.0, 2.0, 0.0, 0.0)
SEED, T0, DT = 12345, 300.0, 0.5


def masses_of(n):
    return np.tile(MASS, n // 3 + 1)[:n]


def real_of(o):
    return np.float32 if eps_of(o) > 1e-10 else np.float64


def set_state(vr, state, call):
    """`state` into the slot that call number `call` reads, a poison value into the other"""
    import torch
    both = np.full((2, 8), -7.0)
    both[call & 1] = state
    vr.state.copy_(torch.as_tensor(both))
    vr.call = call


def state_of(vr, slot):
    return vr.state[slot].cpu().numpy()


def inputs(o, n, seed):
    """velocities of about 700 K and gradients whose half kick changes them by a tenth"""
    rng = np.random.default_rng(seed)
    return dev(o, rng.normal(size=(n, 3)) * 1e-2), dev(o, rng.normal(size=(n, 3)) * 300.0)


def close(got, want, bar=1e-12):
    return abs(got - want) <= bar * abs(want)


@pytest.mark.parametrize('n', SIZES)
def test_at_c_1_the_kick_is_that_of_kick_drift(owner, n):
    """tau = inf: the velocities are bitwise those of admp_md_kick_drift with dt = 0 on the same inputs, alpha is exactly 1 and
    K_after = K_before.  K_before against numpy's float64 sum of the same velocities (exact in double on both handles): a term
    0.5 v v / inv_mass carries 3 roundings, and a sum of 3 n terms of one sign in any order at most 3 n - 1 more per term, on the
    device and in numpy alike: |difference| <= 2 (3 n + 2) 2^-53 K."""
    import torch
    from admp_amd import _lib
    from admp_amd.md import VRescale
    mass = masses_of(n)
    v, g = inputs(owner, n, 200 + n)
    va = v.clone()
    vr = VRescale(owner, mass, DT, T0, float('inf'), SEED)
    assert vr.c == 1.0
    L, h, P = owner._L, owner._h, owner._ptr
    owner._use_current_stream()
    _lib.check(h, L.admp_md_kick_drift(h, n, None, P(va), P(g), P(vr.inv_mass), 0.5 * DT * R.ACC, 0.0, None), 'admp_md_kick_drift')
    vr.kick(v, g)
    assert torch.equal(v, va) and not torch.equal(v, inputs(owner, n, 200 + n)[0])
    info, K, got = vr.info(), R.kinetic(host(va), host(vr.inv_mass)), state_of(vr, 1)[R.K_BEFORE]
    bar = 2.0 * (3 * n + 2) * U64 * K
    print('n %6d: K %.6e kJ/mol, off by %.2e of %.2e' % (n, K / R.ACC, abs(got - K), bar))
    assert abs(got - K) <= bar
    assert info['alpha'] == 1.0 and info['k_after'] == info['k_before'] and info['heat'] == 0.0
    assert info['applications'] == 1 and info['tries'] == 0 and not info['failed']
    assert vr.step == 1 and vr.call == 1


@pytest.mark.parametrize('call', [4, 5])
@pytest.mark.parametrize('n', SIZES)
def test_one_application_against_the_restatement(owner, n, call):
    """grad NULL, c = 0.7, from a state out of the middle of a run: alpha, K_before, K_after and heat within 1e-12 relative of
    the restatement fed numpy's float64 K of the inputs, the tries equal; the velocities are T(alpha of the state) v bitwise; the
    slot that was read is left alone and the other (poisoned before) is written in full."""
    import torch
    from admp_amd.md import VRescale
    mass = masses_of(n)
    v, _ = inputs(owner, n, 300 + n)
    vin = v.clone()
    vr = VRescale(owner, mass, DT, T0, 100.0, SEED)
    vr.c, vr.step = 0.7, 2 ** 33 + 7
    set_state(vr, USED, call)
    want, alpha, ok = R.rule(USED, R.kinetic(host(v), host(vr.inv_mass)), 3 * n, vr.kT_acc, 0.7, SEED, 2 ** 33 + 7, real_of(owner))
    assert ok and alpha != 1.0
    vr.apply(v)
    assert vr.call == call + 1 and vr.step == 2 ** 33 + 8
    got = state_of(vr, (call + 1) & 1)
    assert np.array_equal(state_of(vr, call & 1), np.asarray(USED))
    print('n %6d call %d: alpha %.15f (restatement %.15f), tries %d, relative errors %s'
          % (n, call, got[R.ALPHA], alpha, got[R.TRIES], np.abs(got[:4] / want[:4] - 1.0)))
    for w in (R.K_BEFORE, R.K_AFTER, R.ALPHA, R.HEAT):
        assert close(got[w], want[w]), (w, got, want)
    assert got[R.TRIES] == want[R.TRIES] and got[R.APPLICATIONS] == 18 and got[R.RESERVED] == 0 and got[R.FLAGS] == 0
    a = torch.tensor(got[R.ALPHA], dtype=torch.float64, device=v.device).to(v.dtype)
    assert torch.equal(v, vin * a)


def test_repeatable_bit_for_bit(owner):
    """two runs of 50 kicks at 70 001 atoms: velocities and both state slots"""
    import torch
    from admp_amd.md import VRescale
    n = 70001
    mass = masses_of(n)

    def run():
        v, g = inputs(owner, n, 9)
        vr = VRescale(owner, mass, DT, T0, 20.0, SEED)
        for _ in range(50):
            vr.kick(v, g)
        return v, vr.state.clone(), vr.info()
    v1, s1, info = run()
    v2, s2, _ = run()
    assert torch.equal(v1, v2) and torch.equal(s1, s2)
    assert info['applications'] == 50 and not info['failed'] and info['alpha'] != 1.0


def test_a_chain_follows_the_restatement(owner):
    """2 atoms, Nf = 6, c = 0.9, no forces, 2000 applications with info() after each.  The restatement runs its own chain
    K_{k+1} = rule(K_k).  The device's differs in that its next K_before is the kinetic energy of velocities rounded once to T:
    each component (1 + e), |e| <= u = eps / 2, so K (1 + 2 u) at most.  A difference d in K goes through the rule as J d with
    J = dK'/dK = c + sqrt(c (1 - c) (kT / 2) / K) R1 (mean c: the contraction), so to first order
        bar_{k+1} = |J_k| (bar_k + 2 u K_k) + 32 2^-53 K_{k+1},   bar_0 = 0
    with J_k, K_k from the restatement's chain; the last term covers the rule's own dozen roundings in double on either side and
    the sum of six terms.  The terms of second order are bar / K <= 1e-5 of that: |J| carries a factor 1.001.  u is 2^-24 on the
    single handle and 2^-53 on the double one.  The heat is the sum of the differences K_after - K_before, so its bar is the sum
    of theirs.  The try counts are equal at every step."""
    import torch
    from admp_amd.md import VRescale
    n, nf, c = 2, 6, 0.9
    mass = masses_of(n)
    u = 0.5 * eps_of(owner)
    v = dev(owner, np.random.default_rng(5).normal(size=(n, 3)) * 3e-3)
    vr = VRescale(owner, mass, DT, T0, 100.0, SEED, n_dof=nf)
    vr.c = c
    g = (1.0 - c) * 0.5 * vr.kT_acc
    K = R.kinetic(host(v), host(vr.inv_mass))
    state, bar, worst, heat_bar = R.fresh_state(), 2.0 * 8 * U64 * K, 0.0, 0.0
    for step in range(2000):
        R1 = R.noise(SEED, step, nf)[0]
        J = abs(c + np.sqrt(c * g / K) * R1) * 1.001
        state, _, ok = R.rule(state, K, nf, vr.kT_acc, c, SEED, step, real_of(owner))
        assert ok
        heat_bar += bar + 2.0 * u * K
        bar = J * (bar + 2.0 * u * K) + 32.0 * U64 * state[R.K_AFTER]
        heat_bar += bar
        K = state[R.K_AFTER]
        vr.apply(v)
        info = vr.info()
        err = abs(info['k_after'] * R.ACC - K)
        worst = max(worst, err / bar)
        assert err <= bar, (step, err, bar)
        assert info['tries'] == state[R.TRIES] and info['applications'] == step + 1
    print('largest share of the bar %.3f; the bar ends at %.2e of K; heat %.6f kJ/mol' % (worst, bar / K, info['heat']))
    assert abs(info['heat'] * R.ACC - state[R.HEAT]) <= heat_bar
    assert torch.isfinite(v).all()


@pytest.mark.parametrize('scale', [1e-3, 1e-2, 1.0])
def test_at_c_0_the_kinetic_energy_is_drawn_afresh(owner, scale):
    """tau = 0: K_after = (kT / 2) (R1^2 + S) of the restatement whatever K_before, to 1e-12 relative, plus 2 eps on the single
    handle: K_after is the energy of the velocities as scaled, and alpha is rounded to single once (eps / 2, twice for the square)"""
    from admp_amd.md import VRescale
    n = 257
    vr = VRescale(owner, masses_of(n), DT, T0, 0.0, SEED, n_dof=3 * n - 3)
    assert vr.c == 0.0
    vr.step = 11
    v = dev(owner, np.random.default_rng(6).normal(size=(n, 3)) * scale)
    vr.apply(v)
    R1, S, tries = R.noise(SEED, 11, 3 * n - 3)
    want = 0.5 * vr.kT_acc * (R1 * R1 + S) / R.ACC
    info = vr.info()
    bar = 1e-12 + (2.0 * eps_of(owner) if eps_of(owner) > 1e-10 else 0.0)
    print('K_before %.4e, K_after %.6f, wanted %.6f kJ/mol: off by %.2e of %.2e' % (info['k_before'], info['k_after'], want,
                                                                                   abs(info['k_after'] / want - 1.0), bar))
    assert close(info['k_after'], want, bar) and info['tries'] == tries
    assert close(R.kinetic(host(v), host(vr.inv_mass)) / R.ACC, want, bar + 4.0 * eps_of(owner))      # and the velocities have it
    assert close(vr.temperature(), 2.0 * want / ((3 * n - 3) * R.KB), bar) and vr.kinetic_energy() == info['k_after']


@pytest.fixture(params=['double', 'single'])
def precision(request):
    from admp_amd import settings
    old = settings.PRECISION
    settings.PRECISION = request.param
    try:
        yield request.param
    finally:
        settings.PRECISION = old


def test_scaling_keeps_rigid_water_rigid(precision):
    """27 rigid waters tethered to targets 0.05 A away, ConstrainedLangevin at friction 0, 20 steps of 2 fs with apply after each
    kick: no cluster fails, and the velocity residual max |s.(v_j - v_i)| dt / d^2 after apply is within the constraint
    tolerance.  The residual is linear in the velocities, so one factor for all of them multiplies it by alpha exactly: measured
    before and after each application, after <= alpha before + 8 eps |s| |dv| dt / d^2 (the rounding of the products and of this
    evaluation).  What RATTLE leaves is anywhere up to the tolerance itself, so the residual stays within the tolerance for
    certain only while alpha <= 1: the run cools from 600 K towards 10 K with tau 20 fs (c = 0.905), where alpha^2 has the mean
    c + (1 - c) T_target / T <= 0.93 and the spread 2 sqrt(c (1 - c) (T_target / T) / Nf) <= 0.021 over all 20 steps (T falls
    from 470 K to 50 K, Nf = 162); that every alpha is below 1 is asserted first.  Every application's state is the restatement's for the K_before the
    device found (tries >= 1: the draw is a real one), and that K_before is the float64 sum over the velocities RATTLE left (bar
    as in test_at_c_1_the_kick_is_that_of_kick_drift)."""
    from admp_amd.md import Constraints, ConstrainedLangevin, VRescale, maxwell_boltzmann
    n_mol, L, k, dt = 27, 18.0, 100.0, 2.0
    tol = 1e-8 if precision == 'double' else 1e-6
    eps = 2.0 ** -52 if precision == 'double' else 2.0 ** -23
    box = np.eye(3) * L
    rng = np.random.default_rng(6)
    gr = np.arange(3) * 6.0 + 3.0
    centres = np.stack(np.meshgrid(gr, gr, gr, indexing='ij'), axis=-1).reshape(-1, 3)
    xs = water_geometry(n_mol, centres)
    o = 3 * np.arange(n_mol)
    pairs = np.stack([np.stack([o, o + 1], 1), np.stack([o, o + 2], 1), np.stack([o + 1, o + 2], 1)], axis=1).reshape(-1, 2)
    lengths = np.tile([R0, R0, 2.0 * R0 * np.sin(0.5 * TH0)], n_mol)
    masses = np.tile(MASS, n_mol)
    con = Constraints(3 * n_mol, pairs, lengths, masses, tolerance=tol)
    integ = ConstrainedLangevin(con, dt, T0, 0.0, SEED)
    n_dof = 9 * n_mol - len(pairs)
    vr = VRescale(con, masses, dt, 10.0, 20.0, SEED, n_dof=n_dof)
    x = dev(con, xs)
    t = dev(con, xs + 0.05 * rng.normal(size=xs.shape))
    vel = maxwell_boltzmann(con, masses, 600.0, SEED)
    con.project_velocities(x, vel, box, dt)

    def residual():
        s = host(x)[pairs[:, 1]] - host(x)[pairs[:, 0]]
        w = host(vel)[pairs[:, 1]] - host(vel)[pairs[:, 0]]
        scale = dt / (lengths * lengths)
        return np.abs((s * w).sum(1)) * scale, np.sqrt((s * s).sum(1) * (w * w).sum(1)) * scale
    state, worst, temps, alphas = R.fresh_state(), 0.0, [], []
    for step in range(20):
        integ.kick_drift(x, vel, k * (x - t), box)
        integ.kick(x, vel, k * (x - t), box)
        K = R.kinetic(host(vel), host(vr.inv_mass))
        before, _ = residual()
        vr.apply(vel)
        got = state_of(vr, vr.call & 1)
        assert abs(got[R.K_BEFORE] - K) <= 2.0 * (9 * n_mol + 2) * U64 * K
        state, alpha, ok = R.rule(state, got[R.K_BEFORE], n_dof, vr.kT_acc, vr.c, SEED, step, np.float32 if precision == 'single' else np.float64)
        assert ok and got[R.TRIES] == state[R.TRIES] >= 1
        for w in (R.K_AFTER, R.ALPHA, R.HEAT):
            assert close(got[w], state[w]), (step, w, got, state)
        state[:4] = got[:4]                                               # the next application starts from the device's words
        after, size = residual()
        assert np.all(after <= got[R.ALPHA] * before + 8.0 * eps * size), step
        worst = max(worst, after.max())
        alphas.append(got[R.ALPHA])
        temps.append(vr.temperature())
    print('%s: largest velocity residual %.3e (tolerance %.0e); alpha from %.4f to %.4f; T from %.1f to %.1f K; failures %d'
          % (precision, worst, tol, min(alphas), max(alphas), temps[0], temps[-1], con.failures()))
    assert max(alphas) < 1.0 and temps[-1] < temps[0]
    assert con.failures() == 0
    assert worst <= tol


def test_conserved_quantity(double_precision):
    """64 waters under HarmonicBonded alone in a periodic box, every atom wrapped on its own; the bonded minimum with
    Maxwell-Boltzmann velocities of 100 K; dt 0.25 fs, 2000 steps.  The yardstick is plain velocity Verlet on that start: the
    largest |E(t) - E(0)|, delta_NVE.  With VRescale.kick as the closing kick (target 300 K, tau 100 fs) H = E_pot + K_after -
    heat must stay within 3 delta_NVE of its start -- the thermostat adds no integration error of its own beyond the rounding of
    alpha, and the factor 3 allows for the run now being at a higher temperature than the start -- and |heat| at the end must be
    at least 100 delta_NVE, so that an idle thermostat cannot pass."""
    import torch
    from admp_amd.md import HarmonicBonded, VelocityVerlet, VRescale, maxwell_boltzmann
    n_mol, L, dt, steps = 64, 20.0, 0.25, 2000
    box = np.eye(3) * L
    gr = np.arange(4) * 5.0 + 4.6                                         # the last layer's hydrogens lie beyond the face
    centres = np.stack(np.meshgrid(gr, gr, gr, indexing='ij'), axis=-1).reshape(-1, 3)
    xs = water_geometry(n_mol, centres)
    xs -= L * np.floor(xs / L)
    o = 3 * np.arange(n_mol)
    bonds = np.stack([np.concatenate([o, o]), np.concatenate([o + 1, o + 2])], axis=1)
    angles = np.stack([o + 1, o, o + 2], axis=1)
    hb = HarmonicBonded(3 * n_mol, bonds, np.tile([K_BOND, R0], (2 * n_mol, 1)), angles, np.tile([K_ANG, TH0], (n_mol, 1)))
    masses = np.tile(MASS, n_mol)

    def run(thermostat):
        x = dev(hb, xs)
        vel = maxwell_boltzmann(hb, masses, 100.0, SEED)
        vv = VelocityVerlet(hb, masses, dt)
        vr = VRescale(hb, masses, dt, 300.0, 100.0, SEED, n_dof=9 * n_mol - 3)

        def forces():
            hb.reset_energy()
            return hb.add_forces(x, box, torch.zeros_like(x))
        g = forces()
        e0 = hb.energy() + 0.5 * float((torch.as_tensor(masses, device=x.device)[:, None] * vel * vel).sum()) / R.ACC
        dev_max, heat, temp = 0.0, 0.0, 0.0
        for _ in range(steps):
            vv.kick_drift(x, vel, g)
            g = forces()
            if thermostat:
                vr.kick(vel, g)
                i = vr.info()
                e, heat, temp = hb.energy() + i['k_after'] - i['heat'], i['heat'], vr.temperature()
            else:
                vv.kick(x, vel, g, want_ekin=True)
                e = hb.energy() + vv.kinetic_energy()
            dev_max = max(dev_max, abs(e - e0))
        return dev_max, heat, temp
    d_nve, _, _ = run(False)
    d_vr, heat, temp = run(True)
    print('delta_NVE %.6f kJ/mol; with the thermostat: largest |H(t) - H(0)| %.6f kJ/mol = %.2f delta_NVE, heat %.3f kJ/mol = '
          '%.0f delta_NVE, T at the end %.1f K' % (d_nve, d_vr, d_vr / d_nve, heat, abs(heat) / d_nve, temp))
    assert abs(heat) >= 100.0 * d_nve
    assert d_vr <= 3.0 * d_nve


def test_a_nan_velocity_freezes_the_thermostat(owner):
    import torch
    from admp_amd.md import VRescale
    n = 1000
    vr = VRescale(owner, masses_of(n), DT, T0, 100.0, SEED)
    v, _ = inputs(owner, n, 12)
    vr.apply(v)
    before = state_of(vr, 1)
    v[777, 1] = float('nan')
    kept = v.clone()
    vr.apply(v)
    info = vr.info()
    assert info['failed'] and info['applications'] == 1
    assert torch.equal(v.view(torch.int32 if v.dtype == torch.float32 else torch.int64),
                       kept.view(torch.int32 if v.dtype == torch.float32 else torch.int64))
    assert np.array_equal(state_of(vr, 0)[:7], before[:7])
    clean, _ = inputs(owner, n, 12)
    kept = clean.clone()
    vr.apply(clean)                                                       # a clean K now: still frozen, words carried over
    assert vr.info()['failed'] and torch.equal(clean, kept) and np.array_equal(state_of(vr, 1)[:7], before[:7])
    vr.reset()
    vr.apply(clean)
    info = vr.info()
    assert not info['failed'] and info['applications'] == 1 and not torch.equal(clean, kept)


def test_refusals(owner):
    """bad parameters and tensors the library would read or write out of bounds raise ValueError; each argument the library
    refuses is ADMP_E_ARG there and ValueError from Python; a slab-decomposed handle is ADMP_E_STATE with the text of the older
    entries, before any other argument; n = 0 launches nothing and copies the slot forward"""
    import torch
    from admp_amd import _lib
    from admp_amd.md import STREAM_VRESCALE, HarmonicBonded, VRescale
    assert STREAM_VRESCALE == R.STREAM == 3
    n = 12
    mass = masses_of(n)
    for args in ((mass, DT, -1.0, 100.0, 1), (mass, DT, float('nan'), 100.0, 1), (mass, DT, T0, -1.0, 1), (mass, DT, T0, float('nan'), 1),
                 (mass, -1.0, T0, 100.0, 1), (mass, float('inf'), T0, 100.0, 1), (mass, DT, T0, 100.0, -1), (mass, DT, T0, 100.0, 2 ** 64),
                 (-mass, DT, T0, 100.0, 1)):
        with pytest.raises(ValueError):
            VRescale(owner, *args)
    for n_dof in (0, -3, 2.5):
        with pytest.raises(ValueError):
            VRescale(owner, mass, DT, T0, 100.0, 1, n_dof=n_dof)
    vr = VRescale(owner, mass, DT, T0, 100.0, 1)
    assert vr.n_dof == 3 * n and close(vr.c, np.exp(-DT / 100.0), 1e-15)
    good = lambda: torch.ones((n, 3), dtype=owner._dtype, device=owner._device)      # noqa: E731
    other = torch.float32 if owner._dtype == torch.float64 else torch.float64
    bad = [torch.zeros((n, 3), dtype=other, device=owner._device),                       # wrong precision
           torch.zeros((n, 6), dtype=owner._dtype, device=owner._device)[:, :3],         # non-contiguous view
           torch.zeros((n + 3, 3), dtype=owner._dtype, device=owner._device),            # wrong length
           torch.zeros((n, 3), dtype=owner._dtype),                                      # host tensor
           np.zeros((n, 3))]                                                             # no tensor
    for b in bad:
        with pytest.raises(ValueError):
            vr.apply(b)
        for slot in range(2):
            args = [good(), good()]
            args[slot] = b
            with pytest.raises(ValueError):
                vr.kick(*args)
    # what the library itself refuses, through the object ...
    for name, value in (('n_dof', 0), ('c', -0.1), ('c', 1.5), ('c', float('nan')), ('kT_acc', -1.0), ('kT_acc', float('inf')),
                        ('kT_acc', float('nan')), ('dt', float('inf')), ('dt', float('nan'))):
        keep = getattr(vr, name)
        setattr(vr, name, value)
        with pytest.raises(ValueError, match='admp_md_vrescale'):
            vr.kick(good(), good())
        setattr(vr, name, keep)
    assert vr.call == 0 and vr.step == 0
    # ... and through the C entry
    L, h, P = owner._L, owner._h, owner._ptr
    v, g = good(), good()
    nul = ctypes.c_void_p(None)

    def call(h_=h, n_=n, vel=P(v), im=P(vr.inv_mass), half=1e-5, nf=3 * n, kT=vr.kT_acc, c=0.7, st=P(vr.state)):
        return L.admp_md_vrescale(h_, n_, vel, P(g), im, half, nf, kT, c, 1, 0, 0, st)
    for kw in (dict(vel=nul), dict(im=nul), dict(st=nul), dict(n_=-1), dict(nf=0), dict(nf=-5), dict(c=-1e-9), dict(c=1.0 + 1e-9),
               dict(c=float('nan')), dict(c=float('inf')), dict(kT=-1e-9), dict(kT=float('nan')), dict(kT=float('inf')),
               dict(half=float('nan')), dict(half=float('inf'))):
        assert call(**kw) == E_ARG, kw
    fresh = HarmonicBonded(3, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 2)))
    _lib.check(fresh._h, L.admp_slab_configure(fresh._h, 0, 2), 'admp_slab_configure')      # a slab-decomposed handle
    for kw in (dict(), dict(n_=-1), dict(vel=nul)):
        assert call(h_=fresh._h, **kw) == E_STATE
        assert L.admp_last_error(fresh._h) == b'the MD helpers serve single-rank handles only'
    torch.cuda.synchronize()
    assert torch.equal(v, good()) and np.array_equal(vr.state.cpu().numpy(), np.tile(R.fresh_state(), (2, 1)))      # nothing ran
    # n_atoms = 0 launches nothing and carries the state forward
    none = VRescale(owner, np.zeros(0), DT, T0, 100.0, 1, n_dof=1)
    set_state(none, USED, 3)
    none.apply(torch.zeros((0, 3), dtype=owner._dtype, device=owner._device))
    assert np.array_equal(state_of(none, 0), np.asarray(USED)) and np.array_equal(state_of(none, 1), np.asarray(USED))


def test_drivers_run_with_the_thermostat():
    """examples/md/nvt_water.py and rigid_water.py with --thermostat vrescale on 216 waters: exit status 0 and a final line that
    parses (no temperature is asserted)"""
    out = run_driver('nvt_water.py', '--thermostat', 'vrescale', '--waters', '216', '--steps', '100')
    line = out.strip().splitlines()[-1]
    print(line)
    m = re.search(r'velocity rescaling ([0-9.]+) K, tau ([0-9.]+) fs, seed \d+: T_kin over the second half mean ([-+0-9.e]+) K std '
                  r'([-+0-9.e]+) K \((\d+) records\); conserved quantity drift ([-+0-9.e]+) kJ/mol over (\d+) steps', line)
    assert m, out[-1500:]
    assert float(m.group(1)) == 300.0 and float(m.group(2)) == 100.0 and np.isfinite(float(m.group(3))) and int(m.group(7)) == 99
    assert re.search(r'step +90 +Epot +[-0-9.]+ +Ekin +[0-9.]+ +T_kin +[0-9.]+ +conserved +[-0-9.]+', out), out[-1500:]
    out = run_driver('rigid_water.py', '--thermostat', 'vrescale', '--waters', '216', '--steps', '50', '--dt', '2')
    line = out.strip().splitlines()[-1]
    print(line)
    m = re.search(r'relative energy drift ([-+0-9.e]+), T_final ([-+0-9.e]+) K; velocity rescaling 300.0 K, tau 100 fs: conserved '
                  r'quantity drift ([-+0-9.e]+) kJ/mol over (\d+) steps, heat ([-+0-9.e]+) kJ/mol', line)
    assert m, out[-1500:]
    assert all(np.isfinite(float(m.group(k))) for k in (1, 2, 3, 5)) and int(m.group(4)) == 49
    assert re.search(r'failures 0', out)
