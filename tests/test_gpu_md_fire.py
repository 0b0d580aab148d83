"""The FIRE minimiser on the GPU (admp_amd.md.FireMinimizer; admp_md_fire_step = k_md_fire_sums + k_md_fire_step): one step
against the float64 restatement of tests/fire_ref.py at every size at which the grid changes shape, the two state slots, bitwise
repeatability, the displacement cap, convergence on a harmonic well, the frozen states (done, failed), bonded water in a periodic
box, minimisation on constraints, the refusals, and the driver examples/md/minimize_water.py against the capped descent of the
other drivers.  Both precisions wherever a handle is involved.  Gradients are elementwise torch expressions, so repeatable."""
import re

import numpy as np
import pytest

from tests import fire_ref as R
from tests.test_gpu_md_langevin import E_ARG, MASS, dev, eps_of, host, owner, run_driver      # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1000, 70001]      # 70 001 > 256 x 256: the stride loop and all 256 partial rows are live
MID = (1.3, 0.21, 7.0, 0.9, 3.0, 41.0, 5.0, 0.0)          # a state from the middle of a run (dt, alpha, n_pos, dtv_last, ...)
K_V, K_X = 11, 13                                          # see test_one_step_against_the_restatement


@pytest.fixture
def double_precision():
    from admp_amd import settings
    old = settings.PRECISION
    settings.PRECISION = 'double'
    try:
        yield
    finally:
        settings.PRECISION = old


def masses_of(n):
    return np.tile(MASS, n // 3 + 1)[:n]


def set_state(fm, state, call):
    """`state` into the slot that call number `call` reads, a poison value into the other"""
    import torch
    both = np.full((2, 8), -7.0)
    both[call & 1] = state
    fm.state.copy_(torch.as_tensor(both))
    fm.call = call


def state_of(fm, slot):
    return fm.state[slot].cpu().numpy()


def step_inputs(o, n, downhill, seed):
    """x, v, g (device, the handle's precision) with |Fv| >= 0.1 sqrt(FF vv): F = +-5000 v + noise"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 20.0, size=(n, 3))
    v = rng.normal(size=(n, 3)) * 1e-2
    F = (1.0 if downhill else -1.0) * 5e3 * v + 25.0 * rng.normal(size=(n, 3))
    return dev(o, x), dev(o, v), dev(o, -F)


@pytest.mark.parametrize('downhill', [True, False])
@pytest.mark.parametrize('n', SIZES)
def test_one_step_against_the_restatement(owner, n, downhill):
    """State words: 1e-12 relative on both handles (the six words are summed in double from the same numbers; only the order of
    the sums differs from numpy's).  Positions and velocities: 1e-13 x magnitude on the double handle, k 2^-24 x magnitude on
    the single one, where `magnitude` is the largest sum of the absolute terms of the update and k counts its roundings, each
    at most 2^-24 relative (the restatement works in double from the same single-precision inputs):
      v' = (a v + b F) + dtw F, dtw = dtv (acc / m): a, b, dtv, acc rounded once each (1 each); a v: 1 + 1 = 2 |a v|; b F: 2
      |b F|; their sum: 1; dtw: dtv, acc, two products = 4, dtw F: 5 |dtw F|; the last sum: 1  ->  k_v = 2 + 2 + 1 + 5 + 1 = 11
      of |a v| + |b F| + |dtw F|.
      x' = (x - back v) + dtv v': back v: 2 |back v|; the difference: 1; dtv v': 2 |dtv v'| and dtv times the error of v';
      the last sum: 1  ->  k_x = 13 of |x| + |back v| + dtv (|a v| + |b F| + |dtw F|), the largest single share being dtv k_v + 2.
    The call is number 5, so slot 1 is read and slot 0 (poisoned before) must be written in full."""
    import torch
    from admp_amd.md import FireMinimizer
    mass = masses_of(n)
    fm = FireMinimizer(owner, n, mass)
    x, v, g = step_inputs(owner, n, downhill, 100 + n)
    state = MID[:2] + ((25.0,) if n == 1000 else (7.0,)) + MID[3:]          # n = 1000: past the delay, dt and alpha change too
    set_state(fm, state, 5)
    fm.vel.copy_(v)
    xh, vh, gh, im = host(x), host(v), host(g), host(fm.inv_mass)
    words = R.reduce_words(vh, gh, im)
    assert abs(words[0]) >= 0.1 * np.sqrt(words[1] * words[2])
    x1, v1, s1 = R.step(xh, vh, gh, im, state)
    _, (a, b, back, dtv), moves = R.control(state, words, R.DEFAULTS, 0.0)
    assert moves and (b > 0.0) == downhill and (back > 0.0) == (not downhill)
    fm.step(x, g)
    assert fm.call == 6
    got = state_of(fm, 0)
    s_err = np.abs(got - s1) / np.maximum(np.abs(s1), 1e-300)
    assert np.array_equal(state_of(fm, 1), np.asarray(state))                 # the slot that was read is left alone
    F = -gh
    mag_v = (np.abs(a * vh) + np.abs(b * F) + np.abs(dtv * R.ACC * im[:, None] * F)).max()
    mag_x = (np.abs(xh) + np.abs(back * vh)).max() + dtv * mag_v
    single = owner._dtype == torch.float32
    bar_v, bar_x = (K_V * 2.0 ** -24 * mag_v, K_X * 2.0 ** -24 * mag_x) if single else (1e-13 * mag_v, 1e-13 * mag_x)
    ev, ex = np.abs(host(fm.vel) - v1).max(), np.abs(host(x) - x1).max()
    print('n %6d %s %s: state %.2e of 1e-12, v err / bar %.3f, x err / bar %.3f'
          % (n, 'downhill' if downhill else 'uphill', 'f32' if single else 'f64', s_err.max(), ev / bar_v, ex / bar_x))
    assert s_err.max() <= 1e-12, (got, s1)
    assert ev <= bar_v and ex <= bar_x
    assert torch.equal(g, dev(owner, gh))                                     # the gradient is only read


def test_two_calls_use_the_two_slots(owner):
    """fresh state: call 0 reads slot 0 and writes slot 1, call 1 reads slot 1 and writes slot 0; the state after the second
    call is the restatement's after two steps.  A kernel that read or wrote the wrong parity would start the second step from
    the fresh state again (one iteration counted instead of two) or leave slot 0 fresh."""
    from admp_amd.md import FireMinimizer
    n = 257
    mass = masses_of(n)
    fm = FireMinimizer(owner, n, mass)
    x0, k, _, xs = R.harmonic_well(n)
    x, x0d, kd = dev(owner, xs), dev(owner, x0), dev(owner, k)
    im = host(fm.inv_mass)
    fresh = R.fresh_state()
    assert np.array_equal(state_of(fm, 0), fresh) and np.array_equal(state_of(fm, 1), fresh) and fm.call == 0
    xr, vr, sr = host(x), np.zeros((n, 3)), fresh
    after = []
    for call in range(2):
        g = kd * (x - x0d)
        xr, vr, sr = R.step(xr, vr, host(g), im, sr)
        after.append(sr)
        fm.step(x, g)
        assert fm.call == call + 1
        written, read = state_of(fm, (call + 1) & 1), state_of(fm, call & 1)
        assert np.abs(written - sr).max() <= 1e-12 * np.abs(sr).max(), (call, written, sr)
        assert np.array_equal(read, fresh if call == 0 else written_before)
        written_before = written
        xr, vr = host(x), host(fm.vel)                                        # the next reference step starts from the device's
    info = fm.info()
    assert info['iterations'] == 2 and not info['done'] and not info['failed']
    assert abs(info['dt'] - after[1][R.DT]) <= 1e-12 and info['n_pos'] == after[1][R.NPOS]
    assert info['uphill_steps'] == after[1][R.UPHILL] == 1               # the first call starts from rest: Fv = 0
    assert fm.fmax() == info['fmax'] and fm.converged() is False


def run_well(o, n, iterations, unit_masses=False):
    """`iterations` steps on the harmonic well from a fresh minimiser: (x, vel, both state slots) on the host, bit for bit"""
    import torch
    from admp_amd.md import FireMinimizer
    x0, k, masses, xs = R.harmonic_well(n, unit_masses)
    fm = FireMinimizer(o, n, masses)
    x, x0d, kd = dev(o, xs), dev(o, x0), dev(o, k)
    for _ in range(iterations):
        fm.step(x, kd * (x - x0d))
    torch.cuda.synchronize()
    return x.cpu().numpy(), fm.vel.cpu().numpy(), fm.state.cpu().numpy()


def test_two_runs_are_bitwise_equal(owner):
    """50 iterations at n = 70 001 (every partial row and the stride loop in use): positions, velocities and state"""
    a = run_well(owner, 70001, 50)
    b = run_well(owner, 70001, 50)
    for p, q in zip(a, b):
        assert np.array_equal(p.view(np.uint8), q.view(np.uint8))
    assert a[2][0][R.ITER] == 50 or a[2][1][R.ITER] == 50


def test_no_atom_moves_further_than_the_cap(owner):
    """from rest at the origin, |F_i| log-uniform up to 1e9 kJ/mol/A, one step: every |x_i'| <= max_step (1 + 8 eps_T) and the
    largest is within 1 % of max_step.  (vb = 0, so dtv^2 amax = max_step in double; the move of a component is dtv (dtw F)
    with dtv, acc, acc / m, dtw, dtw F and the last product rounded once each: at most 6 x 2^-24 = 3 eps_T relative, whatever
    the mass.  The positions start at zero so that the move itself, not a rounded sum with a coordinate, is what is measured.)"""
    import torch
    from admp_amd.md import FireMinimizer
    n = 1000
    rng = np.random.default_rng(8)
    mass = masses_of(n)
    F = rng.normal(size=(n, 3))
    F *= (10.0 ** rng.uniform(0.0, 9.0, size=n) / np.sqrt((F * F).sum(1)))[:, None]
    F[17] *= 1e9 / np.sqrt((F[17] ** 2).sum())
    for max_step in (0.1, 0.03):
        fm = FireMinimizer(owner, n, mass, max_step=max_step)
        x = torch.zeros((n, 3), dtype=owner._dtype, device=owner._device)
        fm.step(x, dev(owner, -F))
        move = np.sqrt((host(x) ** 2).sum(1))
        print('max_step %.2f: largest move %.9f' % (max_step, move.max()))
        assert move.max() <= max_step * (1.0 + 8.0 * eps_of(owner))
        assert move.max() >= 0.99 * max_step
        assert fm.info()['dtv_last'] < fm.info()['dt']


@pytest.mark.parametrize('unit_masses', [False, True])
def test_converges_on_the_harmonic_well(owner, unit_masses):
    """n = 1000, k in [500, 4000]: done within 1000 iterations at ftol = 1e-8 (double) or 64 x 2^-24 k_max max|x|, the rounding
    floor of the gradient (single); then every |x_i - x0_i| <= ftol / k_min"""
    import torch
    from admp_amd.md import FireMinimizer
    x0, k, masses, xs = R.harmonic_well(1000, unit_masses)
    fm = FireMinimizer(owner, 1000, masses)
    x, x0d, kd = dev(owner, xs), dev(owner, x0), dev(owner, k)
    single = owner._dtype == torch.float32
    ftol = 64.0 * 2.0 ** -24 * host(kd).max() * np.abs(xs).max() if single else 1e-8
    info = fm.minimize(x, lambda p: kd * (p - x0d), ftol, 1000)
    print('%s, %s masses: done %s after %d iterations (%d uphill), fmax %.3e, ftol %.3e'
          % ('f32' if single else 'f64', 'unit' if unit_masses else 'water', info['done'], info['iterations'], info['uphill_steps'],
             info['fmax'], ftol))
    assert info['done'] and not info['failed'] and info['iterations'] <= 1000 and info['fmax'] <= ftol
    assert fm.converged()
    assert np.sqrt(((host(x) - host(x0d)) ** 2).sum(1)).max() <= ftol / host(kd).min()


def test_done_and_failed_freeze_the_atoms(owner):
    """after `done` further calls change neither positions, velocities nor the iteration counter, bit for bit, and a larger
    force resumes; one NaN in the gradient sets `failed` and moves nothing, also in later calls with a clean gradient;
    minimize raises; reset() clears it"""
    import torch
    from admp_amd.md import FireMinimizer
    n = 300
    x0, k, masses, xs = R.harmonic_well(n)
    fm = FireMinimizer(owner, n, masses)
    x, x0d, kd = dev(owner, xs), dev(owner, x0), dev(owner, k)
    grad = lambda p: kd * (p - x0d)      # noqa: E731
    for _ in range(30):
        fm.step(x, grad(x))
    ftol = 2.0 * float(grad(x).double().norm(dim=1).max())
    fm.step(x, grad(x), ftol)
    info = fm.info()
    assert info['done'] and info['iterations'] == 30
    x_done, v_done = x.clone(), fm.vel.clone()
    assert bool(fm.vel.any())
    for _ in range(3):                                                   # an odd number: both slots carry the frozen state
        fm.step(x, grad(x), ftol)
    assert torch.equal(x, x_done) and torch.equal(fm.vel, v_done)
    assert fm.info() == info
    fm.step(x, grad(x), 0.0)                                             # the same force, a tighter tolerance: it resumes
    info = fm.info()
    assert not info['done'] and info['iterations'] == 31 and not torch.equal(x, x_done)

    x_before, v_before = x.clone(), fm.vel.clone()
    bad = grad(x)
    bad[n // 2, 1] = float('nan')
    fm.step(x, bad)
    info = fm.info()
    assert info['failed'] and not info['done'] and info['iterations'] == 31
    for _ in range(2):
        fm.step(x, grad(x))                                              # clean again: still frozen
    assert fm.info()['failed'] and torch.equal(x, x_before) and torch.equal(fm.vel, v_before)
    with pytest.raises(FloatingPointError):
        fm.minimize(x, grad, 0.0, 20)
    assert torch.equal(x, x_before)
    calls = iter(range(100))
    with pytest.raises(FloatingPointError):                              # a NaN that appears during minimize
        FireMinimizer(owner, n, masses).minimize(x.clone(), lambda p: bad if next(calls) == 12 else grad(p), 0.0, 50)
    fm.reset()
    assert fm.call == 0 and not bool(fm.vel.any())
    info = fm.info()
    assert not info['failed'] and info['iterations'] == 0 and info['dt'] == 0.5
    fm.step(x, grad(x))
    assert fm.info()['iterations'] == 1 and not torch.equal(x, x_before)


K_BOND, R0, K_ANG, TH0 = 3765.6, 0.9572, 460.24, 1.82421813418      # the water of examples/md/water_md.py


def water_geometry(n_mol, centres):
    mol = np.array([[0.0, 0.0, 0.0], [R0, 0.0, 0.0], [R0 * np.cos(TH0), R0 * np.sin(TH0), 0.0]])
    return (centres[:, None, :] + mol[None]).reshape(3 * n_mol, 3)


def test_bonded_water_in_a_periodic_box(double_precision):
    """64 perturbed waters under HarmonicBonded alone, every atom wrapped into the cell on its own so that molecules lie across
    faces: minimize brings every bond within 1e-4 A of r0 and every angle within 1e-4 rad of theta0.  ftol 1e-3 kJ/mol/A: a
    bond 1e-4 A off pulls with 0.38, an angle 1e-4 rad off with 0.05."""
    import torch
    from admp_amd.md import FireMinimizer, HarmonicBonded
    n_mol, L = 64, 20.0
    box = np.eye(3) * L
    rng = np.random.default_rng(4)
    g = np.arange(4) * 5.0 + 4.6                                          # the last layer's hydrogens lie beyond the face
    centres = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    xs = water_geometry(n_mol, centres) + 0.05 * rng.normal(size=(3 * n_mol, 3))
    xs -= L * np.floor(xs / L)
    mol = xs.reshape(n_mol, 3, 3)
    across = int((np.abs(mol[:, 1:] - mol[:, :1]).max(axis=(1, 2)) > 0.5 * L).sum())
    assert across >= 2
    o = 3 * np.arange(n_mol)
    bonds = np.stack([np.concatenate([o, o]), np.concatenate([o + 1, o + 2])], axis=1)
    angles = np.stack([o + 1, o, o + 2], axis=1)
    hb = HarmonicBonded(3 * n_mol, bonds, np.tile([K_BOND, R0], (2 * n_mol, 1)), angles, np.tile([K_ANG, TH0], (n_mol, 1)))
    fm = FireMinimizer(hb, 3 * n_mol, np.tile(MASS, n_mol))
    x = dev(hb, xs)

    def grad(p):
        return hb.add_forces(p, box, torch.zeros_like(p))
    info = fm.minimize(x, grad, 1e-3, 3000)
    m = host(x).reshape(n_mol, 3, 3)
    a, b = m[:, 1] - m[:, 0], m[:, 2] - m[:, 0]
    a -= L * np.round(a / L)
    b -= L * np.round(b / L)
    ra, rb = np.sqrt((a * a).sum(1)), np.sqrt((b * b).sum(1))
    th = np.arccos((a * b).sum(1) / (ra * rb))
    print('%d molecules across a face; done %s after %d iterations; bonds off by %.2e A, angles by %.2e rad'
          % (across, info['done'], info['iterations'], max(np.abs(ra - R0).max(), np.abs(rb - R0).max()), np.abs(th - TH0).max()))
    assert info['done']
    assert max(np.abs(ra - R0).max(), np.abs(rb - R0).max()) <= 1e-4 and np.abs(th - TH0).max() <= 1e-4


def test_minimises_on_the_constraints(double_precision):
    """27 rigid waters (three constraints each) drawn towards random targets by E = sum k |x - t|^2 / 2: after every one of 100
    steps the largest relative constraint error is <= 10 tolerance, no cluster fails, and the energy ends below the start"""
    from admp_amd.md import Constraints, FireMinimizer
    n_mol, L, tol, k = 27, 18.0, 1e-8, 100.0
    box = np.eye(3) * L
    rng = np.random.default_rng(6)
    g = np.arange(3) * 6.0 + 3.0
    centres = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    xs = water_geometry(n_mol, centres)
    o = 3 * np.arange(n_mol)
    pairs = np.stack([np.stack([o, o + 1], 1), np.stack([o, o + 2], 1), np.stack([o + 1, o + 2], 1)], axis=1).reshape(-1, 2)
    lengths = np.tile([R0, R0, 2.0 * R0 * np.sin(0.5 * TH0)], n_mol)
    masses = np.tile(MASS, n_mol)
    con = Constraints(3 * n_mol, pairs, lengths, masses, tolerance=tol)
    fm = FireMinimizer(con, 3 * n_mol, masses, constraints=con)
    x = dev(con, xs)
    t = dev(con, xs + 0.5 * rng.normal(size=xs.shape))

    def error(p):
        d = host(p)[pairs[:, 1]] - host(p)[pairs[:, 0]]
        return (np.abs(np.sqrt((d * d).sum(1)) - lengths) / lengths).max()

    def energy(p):
        return 0.5 * k * float(((p - t) ** 2).sum())
    assert error(x) <= tol
    with pytest.raises(ValueError):
        fm.step(x, k * (x - t))                                          # no box
    e0, worst = energy(x), 0.0
    for _ in range(100):
        fm.step(x, k * (x - t), 0.0, box)
        worst = max(worst, error(x))
    print('energy %.4f -> %.4f, worst constraint error %.2e (tolerance %.0e), most sweeps %d, %d iterations, %d uphill'
          % (e0, energy(x), worst, tol, con.max_sweeps_seen(), fm.info()['iterations'], fm.info()['uphill_steps']))
    assert worst <= 10.0 * tol
    assert con.failures() == 0
    assert energy(x) < e0


BAD_PARAMETERS = [dict(dt_min_fs=0.0), dict(dt_min_fs=float('nan')), dict(dt_max_fs=-1.0), dict(dt_max_fs=float('inf')),
                  dict(max_step=0.0), dict(max_step=float('nan')), dict(dt_min_fs=6.0), dict(f_inc=0.9), dict(f_dec=0.0),
                  dict(f_dec=1.5), dict(alpha_start=0.0), dict(alpha_start=1.1), dict(f_alpha=0.0), dict(f_alpha=2.0),
                  dict(n_delay=-1), dict(dt_start_fs=0.0)]
# the same through the C entry: index into params9 and the bad value
BAD_WORDS = [(2, 0.0), (2, float('nan')), (1, -1.0), (1, float('inf')), (3, 0.0), (3, float('nan')), (2, 6.0), (5, 0.9), (6, 0.0),
             (6, 1.5), (7, 0.0), (7, 1.1), (8, 0.0), (8, 2.0), (4, -1.0), (3, float('inf')), (5, float('nan')), (4, float('nan'))]


def test_refusals(owner):
    """bad parameters, tensors the library would read or write out of bounds and a slab-decomposed handle are refused with
    ValueError in Python and ADMP_E_ARG by the library, before anything is launched"""
    import torch
    from admp_amd import _lib
    from admp_amd.md import FireMinimizer, HarmonicBonded
    n = 12
    mass = masses_of(n)
    for kw in BAD_PARAMETERS:
        with pytest.raises(ValueError):
            FireMinimizer(owner, n, mass, **kw)
    for args in ((owner, n, mass[:-1]), (owner, n, -mass), (owner, -1, None), (owner, 2.5, None)):
        with pytest.raises(ValueError):
            FireMinimizer(*args)
    with pytest.raises(ValueError):
        FireMinimizer(owner, n, mass, constraints=owner)                 # not a Constraints
    fm = FireMinimizer(owner, n)                                         # unit masses
    assert np.array_equal(host(fm.inv_mass), np.ones(n))
    good = lambda: torch.ones((n, 3), dtype=owner._dtype, device=owner._device)      # noqa: E731
    other = torch.float32 if owner._dtype == torch.float64 else torch.float64
    bad = [torch.zeros((n, 3), dtype=other, device=owner._device),                       # wrong precision
           torch.zeros((n, 6), dtype=owner._dtype, device=owner._device)[:, :3],         # non-contiguous view
           torch.zeros((n + 3, 3), dtype=owner._dtype, device=owner._device),            # wrong length
           torch.zeros((n, 3), dtype=owner._dtype),                                      # host tensor
           np.zeros((n, 3))]                                                             # no tensor
    for b in bad:
        for slot in range(2):
            args = [good(), good()]
            args[slot] = b
            with pytest.raises(ValueError):
                fm.step(*args)
    for ftol in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            fm.step(good(), good(), ftol)
    with pytest.raises(ValueError):
        fm.minimize(good(), lambda p: good(), 0.0, 10, check_every=0)
    assert fm.call == 0

    L, h, P = owner._L, owner._h, owner._ptr
    x, g = good(), good()
    par = list(R.DEFAULTS)
    call = lambda p9, n_=n, ftol=0.0, xs=x, st=fm.state: L.admp_md_fire_step(      # noqa: E731
        h, n_, P(xs), P(fm.vel), P(g), P(fm.inv_mass), None if p9 is None else _lib.darr(p9), ftol, 0, P(st))
    for w, value in BAD_WORDS:
        p9 = list(par)
        p9[w] = value
        assert call(p9) == E_ARG, (w, value)
    for ftol in (-1.0, float('nan'), float('inf')):
        assert call(par, ftol=ftol) == E_ARG
    assert call(par, n_=-1) == E_ARG
    assert call(None) == E_ARG and call(par, xs=None) == E_ARG and call(par, st=None) == E_ARG
    fresh = HarmonicBonded(3, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 2)))
    _lib.check(fresh._h, L.admp_slab_configure(fresh._h, 0, 2), 'admp_slab_configure')      # a slab-decomposed handle
    assert L.admp_md_fire_step(fresh._h, n, P(x), P(fm.vel), P(g), P(fm.inv_mass), _lib.darr(par), 0.0, 0, P(fm.state)) == E_ARG
    assert b'single-rank' in L.admp_last_error(fresh._h)
    with pytest.raises(ValueError, match='single-rank'):
        FireMinimizer(fresh, n).step(good(), good())
    torch.cuda.synchronize()
    assert torch.equal(x, good()) and not bool(fm.vel.any())             # nothing was launched
    assert np.array_equal(fm.state.cpu().numpy(), np.tile(R.fresh_state(), (2, 1)))
    # n_atoms = 0 launches nothing and carries the state forward
    none = FireMinimizer(owner, 0)
    set_state(none, MID, 3)
    empty = torch.zeros((0, 3), dtype=owner._dtype, device=owner._device)
    none.step(empty, empty)
    assert np.array_equal(state_of(none, 0), np.asarray(MID)) and np.array_equal(state_of(none, 1), np.asarray(MID))


def test_driver_fire_ends_below_the_capped_descent():
    """examples/md/minimize_water.py on 216 waters, 100 evaluations, double precision, fixed multipoles: both minimisers in one
    process from the same start; FIRE must end below the capped steepest descent of water_md.minimize in the potential
    energy AND in the largest |g_i|"""
    out = run_driver('minimize_water.py', '--waters', '216', '--minimize', '100')
    line = out.strip().splitlines()[-1]
    m = re.search(r'after 100 evaluations: sd Epot ([-+0-9.e]+) gmax ([-+0-9.e]+); fire Epot ([-+0-9.e]+) gmax ([-+0-9.e]+)', line)
    assert m, out[-1500:]
    print(line)
    sd_e, sd_g, fire_e, fire_g = (float(x) for x in m.groups())
    assert fire_e < sd_e and fire_g < sd_g, line
