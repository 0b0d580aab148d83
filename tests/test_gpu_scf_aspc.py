"""Predictor-corrector dipoles (ADMPPmeForce.set_aspc; admp_scf_aspc, engine.hip scf_fixed): a step restated with the float64
oracle, the fixed form against the existing SCF taking the same Jacobi steps, the history's bookkeeping, stability along a
smooth path against a float64 restatement of the same run (tests/golden/aspc_track_64.npz, written by
tests/golden/make_aspc_track.py), the refusals, and a driver run."""
import os
import subprocess
import sys

import numpy as np
import pytest

from admp_amd import settings
from admp_amd import systems as S
from tests.test_gpu_parity import GOLD, precision, rel, water_system      # noqa: F401
from tests.test_scf_aspc_cpu import closed_B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def coefs(k):
    return [float(closed_B(k, j)) for j in range(1, k + 3)]


def kolafa(k):
    return (k + 2.0) / (2 * k + 3.0)


def predict(hist, k):
    """U_p in float64 from the returned dipoles, newest last in `hist`; summed from j = 1 upwards like the kernel"""
    acc = np.zeros_like(np.asarray(hist[-1], dtype=np.float64))
    for j, b in enumerate(coefs(k), start=1):
        acc = acc + b * np.asarray(hist[-j], dtype=np.float64)
    return acc


def moving_frames(pos, n):
    """pos + vel k, vel as in test_first_cycle_forms_agree_on_a_moving_sequence"""
    vel = np.random.default_rng(3).normal(size=pos.shape) * 0.012
    return [pos + vel * k for k in range(n)]


def pol_args(par):
    return (par['Q_local'], par['pol'], par['tholes'], par['mScales'], par['pScales'], par['dScales'])


def force(n_mol, prec, rc_list=4.0, mesh=None, cutoff=None, seed=5):
    from admp_amd.pme import ADMPPmeForce
    settings.PRECISION = prec
    pos, box, at, ai, cov, par, pairs = water_system(n_mol, seed, True, rc=rc_list)

    def make():
        f = ADMPPmeForce(box, at, ai, cov, 4.0, 1e-4, 2, lpol=True)
        if mesh:
            for k in ('K1', 'K2', 'K3'):
                f.update_env(k, mesh)
        if cutoff:
            f.set_cutoff(cutoff)
        return f
    return make, pos, box, par, pairs


def close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max()
    d = np.abs(a - b).max()
    return d <= tol * scale, (d, scale)


# ---- 1. one step against the float64 oracle -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def oracle_125():
    """the 125-water system and one oracle object per mesh; the oracle's answers to a step are cached by the bytes of its inputs"""
    import torch
    from oracle import admp_oracle as O
    pos, box, at, ai, cov, par, pairs = water_system(125, 5, True)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)      # noqa: E731
    Q, pol, thole, mS, pS = t(par['Q_local']), t(par['pol']), t(par['tholes']), t(par['mScales']), t(par['pScales'])

    def step(kappa, K, p, U_p, n_corr, omega):
        sysm = O.PmeSystem(at, ai, cov, kappa, K, 2, True)
        U, resid = t(U_p), None
        for _ in range(n_corr):
            Ug = U.clone().requires_grad_(True)
            e = O.energy_pme(sysm, t(p), t(box), pairs, Q, Ug, pol, thole, mS, pS)
            field, = torch.autograd.grad(e, Ug)
            if resid is None:
                resid = float(field[pol > 0.001].abs().max())
            U = (Ug - omega * field * pol[:, None] / O.DIELECTRIC).detach()
        pt = t(p).clone().requires_grad_(True)
        parts = O.energy_pme_parts(sysm, pt, t(box), pairs, Q, U, pol, thole, mS, pS)
        g, = torch.autograd.grad(sum(parts), pt)
        return U.numpy(), [float(x.detach()) for x in parts], g.numpy(), resid
    return pos, box, par, pairs, step


DOUBLE, SINGLE = ('double', 1e-9, 1e-8), ('single', 2e-4, 5e-4)      # the bars of test_polarizable_water_vs_oracle


@pytest.mark.parametrize('bars,order,n_corr,omega', [(DOUBLE, 0, 1, None), (DOUBLE, 2, 1, None), (DOUBLE, 4, 1, None), (SINGLE, 0, 1, None),
                                                     (SINGLE, 2, 1, None), (SINGLE, 4, 1, None), (DOUBLE, 2, 2, 0.8)])
def test_one_step_against_the_oracle(precision, oracle_125, bars, order, n_corr, omega):
    from admp_amd.pme import ADMPPmeForce
    prec, tolE, tolG = bars
    settings.PRECISION = prec
    pos, box, par, pairs, oracle_step = oracle_125
    at, ai, cov = S.water_topology(125)
    f = ADMPPmeForce(box, at, ai, cov, 4.0, 1e-4, 2, lpol=True)
    f.set_aspc(order, n_corr, omega)
    om = kolafa(order) if omega is None else omega
    info = f.aspc_info()
    assert (info['order'], info['n_corrector'], info['stored'], info['fixed'], info['warmup'], info['fallback']) == (order, n_corr, 0, 0, 0, 0)
    assert info['omega'] == om
    hist, U = [], None
    frames = moving_frames(pos, order + 2 + 3)
    for k, p in enumerate(frames):
        E, G = f.get_forces(p, box, pairs, *pol_args(par), U_init=U)
        U = np.asarray(f.U_ind, dtype=np.float64).copy()
        info = f.aspc_info()
        fixed = max(0, k + 1 - (order + 2))
        assert (info['stored'], info['fixed'], info['warmup'], info['fallback']) == (min(k + 1, order + 2), fixed, min(k + 1, order + 2), 0), (k, info)
        if k >= order + 2:
            U_ref, parts, g_ref, resid = oracle_step(f.kappa, (f.K1, f.K2, f.K3), p, predict(hist, order), n_corr, om)
            scale = max(abs(x) for x in parts)
            dE = max(abs(a - b) for a, b in zip(f.energy_parts, parts)) / scale
            print('%s order %d step %d: parts %.2e of the largest, U %.2e, grad %.2e, residual %.4e (oracle %.4e)'
                  % (prec, order, k, dE, rel(U, U_ref), rel(G, g_ref), info['residual'], resid))
            assert f.n_cycle == n_corr and f.lconverg is True
            assert dE <= tolE
            assert rel(U, U_ref) < tolG and rel(G, g_ref) < tolG
            assert abs(E - sum(parts)) <= 4 * tolE * scale
            assert abs(info['residual'] - resid) <= tolG * resid
        hist.append(U)


# ---- 2. equivalence with the existing SCF ---------------------------------------------------------------------------------
CASES = {'216-double': (216, 'double', {}), '216-single': (216, 'single', {}), '216-double-mesh32': (216, 'double', dict(mesh=32)),
         '216-double-cutoff': (216, 'double', dict(rc_list=5.0, cutoff=4.0)), '1536-single': (1536, 'single', {})}


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('case', sorted(CASES))
def test_fixed_form_equals_n_jacobi_steps_of_the_existing_scf(precision, case, n):
    """omega = 1, n correctors: the same dipoles, energies and gradient as the plain loop started from U_p with maxiter = n
    and a threshold nothing passes"""
    n_mol, prec, kw = CASES[case]
    order = 2
    make, pos, box, par, pairs = force(n_mol, prec, **kw)
    f, g = make(), make()
    f.set_aspc(order, n, 1.0)
    tol = 1e-10 if prec == 'double' else 2e-4
    hist, U = [], None
    for k, p in enumerate(moving_frames(pos, order + 2 + 2)):
        if k == order + 2:
            stats0, riders0 = f.scf_stats(), f.pair_rider_stats()
        E, G = f.get_forces(p, box, pairs, *pol_args(par), U_init=U)
        U = np.asarray(f.U_ind, dtype=np.float64).copy()
        if k >= order + 2:
            Q, pol, th, mS, pS, dS = pol_args(par)
            r = g._evaluate(p, box, pairs, Q, mS, pol, th, pS, dS, U_init=predict(hist, order), maxiter=n, thresh=0.0)
            assert f.n_cycle == n and f.lconverg is True
            for name, a, b in (('parts', f.energy_parts, g.energy_parts), ('grad', G, r['grad'].cpu().numpy()), ('U', U, r['U'].cpu().numpy())):
                ok, fig = close(a, b, tol)
                print('%s n=%d step %d %s: %.3e of %.3e' % (case, n, k, name, fig[0], fig[1]))
                assert ok, (name, fig)
        hist.append(U)
    stats, riders = f.scf_stats(), f.pair_rider_stats()
    assert f.aspc_info()['fixed'] == 2 and f.aspc_info()['fallback'] == 0
    for key in ('plain', 'speculative', 'chained'):
        assert stats[key] == stats0[key], (key, stats, stats0)      # the fixed-form steps are none of the three
    assert stats['jacobi_steps'] == stats0['jacobi_steps'] + 2 * n
    if case == '216-double':          # a direct-DFT mesh on one stream: the closing pair kernel rode in the last x pass
        assert riders['rode'] == riders0['rode'] + 2 and riders['own_launch'] == riders0['own_launch'], (riders, riders0)
    else:
        assert riders['rode'] + riders['own_launch'] == riders0['rode'] + riders0['own_launch'] + 2


# ---- 3. the history -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['double', 'single'])
def test_history_bookkeeping(precision, prec):
    order = 1
    make, pos, box, par, pairs = force(216, prec)
    tol = 1e-10 if prec == 'double' else 2e-4
    args = pol_args(par)
    frames = moving_frames(pos, 8)

    def run(f, k, U):
        E, G = f.get_forces(frames[k], box, pairs, *args, U_init=U)
        return np.asarray(f.energy_parts), np.asarray(G), np.asarray(f.U_ind, dtype=np.float64).copy()

    def same(x, y):
        for a, b in zip(x, y):
            ok, fig = close(a, b, tol)
            assert ok, fig

    f, plain, undisturbed = make(), make(), make()
    f.set_aspc(order)
    undisturbed.set_aspc(order)
    U = Up = Uu = None
    for k in range(order + 2):          # warm-up calls return what a handle without the mode returns
        a, b = run(f, k, U), run(plain, k, Up)
        run(undisturbed, k, Uu)
        same(a, b)
        assert f.n_cycle == plain.n_cycle and f.lconverg == plain.lconverg
        U, Up, Uu = a[2], b[2], np.asarray(undisturbed.U_ind, dtype=np.float64).copy()
    assert f.aspc_info()['stored'] == order + 2 and f.aspc_info()['warmup'] == order + 2
    k = order + 2
    a = run(f, k, U)
    same(a, run(undisturbed, k, Uu))
    assert f.aspc_info()['fixed'] == 1
    # calls that are not time steps leave the history alone ...
    Q, pol, th, mS, pS, dS = args
    f.get_energy_and_box_gradient(frames[k], box, pairs, *args)
    f.energy_fn(frames[k], box, pairs, Q, a[2], pol, th, mS, pS, dS)
    f.get_pscale_gradient(frames[k], box, pairs, *args)
    info = f.aspc_info()
    assert (info['stored'], info['fixed'], info['warmup'], info['fallback']) == (order + 2, 1, order + 2, 0)
    # ... so the next step is the one of the undisturbed run
    same(run(f, k + 1, None), run(undisturbed, k + 1, None))
    assert f.aspc_info()['fixed'] == 2 and f.n_cycle == 1
    # a call that raises leaves the count unchanged, and the step after it is still the undisturbed one
    old = settings.MAX_N_POL
    settings.MAX_N_POL = 0
    try:
        with pytest.raises(RuntimeError):
            f.get_forces(frames[k + 2], box, pairs, *args)
    finally:
        settings.MAX_N_POL = old
    assert f.aspc_info()['stored'] == order + 2 and f.aspc_info()['fixed'] == 2
    same(run(f, k + 2, None), run(undisturbed, k + 2, None))
    # polarizabilities the host has not seen: the ordinary SCF from U_p, counted as a fallback, and stored
    hist_U = np.asarray(f.U_ind, dtype=np.float64)
    par2 = dict(par, pol=par['pol'] * (1.0 + 1e-13))
    f.get_forces(frames[k + 3], box, pairs, *pol_args(par2))
    info = f.aspc_info()
    assert (info['fallback'], info['fixed'], info['stored']) == (1, 3, order + 2) and f.lconverg is True
    assert not np.array_equal(np.asarray(f.U_ind, dtype=np.float64), hist_U)
    # reset, switching off and a new mesh empty it
    f.reset_aspc()
    assert f.aspc_info()['stored'] == 0 and f.aspc_info()['order'] == order
    run(f, 0, None)
    assert f.aspc_info()['stored'] == 1
    f.update_env('K1', f.K1)             # (admp_set_ewald)
    assert f.aspc_info()['stored'] == 0 and f.aspc_info()['order'] == order
    run(f, 0, None)
    f.set_aspc(None)
    info = f.aspc_info()
    assert (info['order'], info['stored'], info['n_corrector']) == (-1, 0, 0)
    same(run(f, 3, None), run(plain, 3, None))      # off: as a handle that never had the mode
    assert f.aspc_info()['stored'] == 0


def test_a_new_topology_empties_the_history(precision):
    from admp_amd import _lib
    make, pos, box, par, pairs = force(125, 'double')
    f = make()
    f.set_aspc(0)
    f.get_forces(pos, box, pairs, *pol_args(par))
    assert f.aspc_info()['stored'] == 1
    at, ai, cov = S.water_topology(125)
    _lib.check(f._h, f._L.admp_set_topology(f._h, 375, None, None, None, None, None), 'admp_set_topology')
    assert f.aspc_info()['stored'] == 0 and f.aspc_info()['order'] == 0


# ---- 4. stability ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['double', 'single'])
def test_stability_along_a_smooth_path(precision, prec):
    """40 fixed-form steps (order 2, one corrector) on pos + vel k + acc k^2 / 2: at every step the deviation from the converged
    dipoles is at most 1.5 x the float64 restatement's (tests/golden/make_aspc_track.py), plus the dipole tolerance 5e-4 in
    single precision, and it does not grow: the last 10 steps stay within a factor 2 of steps 5 - 15."""
    from admp_amd.pme import ADMPPmeForce
    from tests.golden.make_aspc_track import path_frames
    gold = np.load(os.path.join(GOLD, 'aspc_track_64.npz'))
    n_mol, order, steps = int(gold['n_mol']), int(gold['order']), int(gold['steps'])
    settings.PRECISION = prec
    pos, box = S.synthetic_water_box(n_mol, seed=int(gold['seed']))
    at, ai, cov = S.water_topology(n_mol)
    par = S.water_parameters(n_mol, polarizable=True)
    pairs = S.build_pairs(pos, box, float(gold['rc']))
    f, conv = (ADMPPmeForce(box, at, ai, cov, float(gold['rc']), float(gold['ethresh']), 2, lpol=True) for _ in range(2))
    assert (f.K1, f.K2, f.K3) == tuple(int(x) for x in gold['K']) and abs(f.kappa - float(gold['kappa'])) < 1e-12
    tight = float(gold['tight']) if prec == 'double' else 1e-2
    Q, pol, th, mS, pS, dS = pol_args(par)
    f.set_aspc(order, 1)
    dev, Uc = [], None
    for k, p in enumerate(path_frames(pos, order + 2 + steps, int(gold['path_seed']), float(gold['vel']), float(gold['acc']))):
        r = conv._evaluate(p, box, pairs, Q, mS, pol, th, pS, dS, U_init=Uc, want_grad=False, maxiter=200, thresh=tight)
        assert r['flag']
        Uc = r['U']
        if k < order + 2:      # the warm-up dipoles are the converged ones, as in the restatement
            r = f._evaluate(p, box, pairs, Q, mS, pol, th, pS, dS, U_init=Uc, want_grad=False, maxiter=200, thresh=tight)
            continue
        r = f._evaluate(p, box, pairs, Q, mS, pol, th, pS, dS, want_grad=False)
        assert r['i'] == 1
        dev.append(float((r['U'].double() - Uc.double()).abs().max() / Uc.double().abs().max()))
    dev = np.array(dev)
    assert f.aspc_info()['fixed'] == steps and f.aspc_info()['fallback'] == 0
    bar = 1.5 * gold['dev'] + (5e-4 if prec == 'single' else 0.0)
    print(prec, 'deviation / bar, worst step:', float((dev / bar).max()), 'deviations', dev.min(), dev.max())
    assert (dev <= bar).all(), (dev / bar).max()
    assert dev[-10:].max() <= 2.0 * dev[5:16].max()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(precision):
    from admp_amd import _lib
    from admp_amd.pme import ADMPPmeForce
    make, pos, box, par, pairs = force(125, 'double')
    f = make()
    f.set_aspc(3, 2, 0.9)
    before = f.aspc_info()
    for bad in (dict(order=-2), dict(order=5), dict(order=2, n_corrector=0), dict(order=2, n_corrector=7), dict(order=2, omega=1.5),
                dict(order=2, omega=float('nan')), dict(order=2, omega=0.0), dict(order=1.5)):
        with pytest.raises(ValueError):
            f.set_aspc(**bad)
        assert f.aspc_info() == before
    L = f._L
    for order, nc, om in ((-2, 1, 0.0), (5, 1, 0.0), (2, 0, 0.0), (2, 7, 0.0), (2, 1, 1.5), (2, 1, float('nan'))):
        assert L.admp_scf_aspc(f._h, order, nc, om) == _lib.E_ARG
        assert f.aspc_info() == before
    assert L.admp_scf_aspc_info(f._h, None, None) == _lib.E_ARG
    # a non-polarizable handle
    at, ai, cov = S.water_topology(125)
    fixed = ADMPPmeForce(box, at, ai, cov, 4.0, 1e-4, 2, lpol=False)
    with pytest.raises(RuntimeError):
        fixed.set_aspc(2)
    assert L.admp_scf_aspc(fixed._h, 2, 1, 0.0) == _lib.E_STATE
    assert L.admp_scf_aspc(fixed._h, -1, 1, 0.0) == 0          # switching off what is off is no error
    # a slab-configured handle refuses; configuring a handle as a slab afterwards turns the mode off
    slab = make()
    _lib.check(slab._h, L.admp_slab_configure(slab._h, 0, 2), 'admp_slab_configure')
    assert L.admp_scf_aspc(slab._h, 2, 1, 0.0) == _lib.E_STATE
    with pytest.raises(RuntimeError):
        slab.set_aspc(2)
    _lib.check(f._h, L.admp_slab_configure(f._h, 0, 2), 'admp_slab_configure')
    assert f.aspc_info()['order'] == -1


# ---- 6. a driver run --------------------------------------------------------------------------------------------------------------
def test_nve_driver_with_aspc():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'md', 'nve_water.py'), '--waters', '64', '--pol', '--aspc', '2',
                        '--steps', '40', '--minimize', '20'], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith('# ASPC order 2')]
    assert len(line) == 1 and ' 2.00 field evaluations per step after the warm-up' in line[0], r.stdout[-2000:]
    assert '(36 fixed-form, 4 warm-up, 0 fallback calls' in line[0], line[0]
    drift = float(r.stdout.split('relative energy drift')[1].split(',')[0])
    assert np.isfinite(drift), r.stdout[-500:]
    both = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'md', 'nve_water.py'), '--aspc', '2', '--predict', '1'],
                          capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert both.returncode == 2 and 'not allowed with' in both.stderr
