"""The Langevin thermostat of the MD drivers on the GPU (admp_amd.md.Langevin / maxwell_boltzmann; admp_md_langevin,
admp_md_random): the device generator against the numpy restatement of tests/test_md_random_cpu.py (words exactly, normals to
rounding, moments within their sampling error), one BAOAB step against the formulas, the friction-free limit against velocity
Verlet, an ideal gas that must sit at the target temperature per species, the Maxwell-Boltzmann start, the refusals, and the
driver examples/md/nvt_water.py end to end.  Both precisions wherever a handle is involved."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_md_random_cpu import TRIPLES, normals, words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB = 0.0083144626          # kJ/mol/K
ACC = 1e-4                 # 1 kJ/mol/amu = 1e-4 A^2/fs^2
MASS = (15.999, 1.008, 1.008)
E_ARG = -1                 # include/admp_hip.h ADMP_E_ARG

ref_words = functools.lru_cache(maxsize=None)(words)
ref_normals = functools.lru_cache(maxsize=None)(normals)


@pytest.fixture(params=['double', 'single'])
def owner(request):
    """a calculator whose handle and stream the MD helpers borrow (no bonds: only its precision and device matter)"""
    from admp_amd import settings
    from admp_amd.md import HarmonicBonded
    old = settings.PRECISION
    settings.PRECISION = request.param
    try:
        yield HarmonicBonded(3, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 2)))
    finally:
        settings.PRECISION = old


def eps_of(o):
    import torch
    return float(np.finfo(np.float32 if o._dtype == torch.float32 else np.float64).eps)


def host(t):
    return t.double().cpu().numpy()


def dev(o, a):
    import torch
    return torch.as_tensor(np.asarray(a), dtype=o._dtype, device=o._device).contiguous()


def baoab_first_half(r, v, g, im, dt, T, gamma, seed, step):
    """float64 restatement of k_md_langevin: B, A, O, A"""
    c1 = np.exp(-gamma * dt)
    v = v - 0.5 * dt * ACC * g * im[:, None]
    r = r + 0.5 * dt * v
    v = c1 * v + np.sqrt((1.0 - c1 * c1) * KB * T * ACC * im)[:, None] * ref_normals(len(im), seed, step, 0)
    r = r + 0.5 * dt * v
    return r, v


@pytest.mark.parametrize('seed,step,stream', TRIPLES)
def test_words_equal_the_restatement(owner, seed, step, stream):
    """n = 1000 is no multiple of the 256 lanes of a workgroup; the third triple fails if a high half of seed or step is
    dropped on the way to the kernel"""
    from admp_amd.md import random_fill
    w = random_fill(owner, 0, 1000, seed, step, stream).cpu().numpy().view(np.uint32)
    assert w.shape == (1000, 4)
    assert np.array_equal(w, ref_words(1000, seed, step, stream))


@pytest.mark.parametrize('seed,step,stream', TRIPLES)
def test_normals_equal_the_restatement(owner, seed, step, stream):
    """evaluated in double on both handles and rounded last: 1e-12 on a double handle (two libm's), 1e-6 on a single one
    (6.77 * 2^-24 for the final rounding, with a factor 2 to spare)"""
    from admp_amd.md import random_fill
    z = host(random_fill(owner, 1, 1000, seed, step, stream))
    d = np.abs(z - ref_normals(1000, seed, step, stream)).max()
    print('max |difference| %.3e' % d)
    assert d <= (1e-12 if eps_of(owner) < 1e-10 else 1e-6)


def test_normal_moments_within_sampling_error(owner):
    """n = 65536 atoms at seed 1: every moment within 4 sigma of its sampling error (the draw is deterministic; the restatement
    sits inside 2 sigma on each)"""
    from admp_amd.md import random_fill
    n = 65536
    a, b = host(random_fill(owner, 1, n, 1, 0, 0)), host(random_fill(owner, 1, n, 1, 1, 0))
    figures = {
        'mean': (a.mean(), 1.0 / np.sqrt(3 * n)),
        'variance': (a.var() - 1.0, np.sqrt(2.0 / (3 * n))),
        'fourth moment': ((a ** 4).mean() - 3.0, np.sqrt(96.0 / (3 * n))),
        'xy': ((a[:, 0] * a[:, 1]).mean(), 1.0 / np.sqrt(n)),
        'atom i, i+1': ((a[:-1, 0] * a[1:, 0]).mean(), 1.0 / np.sqrt(n)),
        'step 0, 1': ((a * b).mean(), 1.0 / np.sqrt(3 * n)),
    }
    for name, (value, sigma) in figures.items():
        print('%-14s %+.2f sigma' % (name, value / sigma))
    assert np.abs(a).max() <= 6.77
    for name, (value, sigma) in figures.items():
        assert abs(value) <= 4.0 * sigma, name


def test_one_step_against_the_formulas(owner):
    """300 waters' worth of atoms, dt 0.5, 300 K, friction 0.05, seed 11, step 3: r and v after kick_drift to 16 eps max|.|
    (the longest rounding chain, positions, is about six operations on numbers up to the box length), the kinetic energy after
    kick to 64 eps relative; the second call draws step 4; step set back to 3 on a fresh copy repeats the first result bit
    for bit."""
    import torch
    from admp_amd.md import Langevin
    eps = eps_of(owner)
    n, dt, T, gamma, seed = 900, 0.5, 300.0, 0.05, 11
    mass = np.tile(MASS, n // 3)
    rng = np.random.default_rng(1)
    r = dev(owner, rng.uniform(0.0, 20.8, size=(n, 3)))
    v = dev(owner, rng.normal(size=(n, 3)) * 1e-2)
    g = dev(owner, rng.normal(size=(n, 3)) * 50.0)
    r_in, v_in = r.clone(), v.clone()
    lv = Langevin(owner, mass, dt, T, gamma, seed)
    lv.step = 3
    im = host(lv.inv_mass)
    r1, v1 = baoab_first_half(host(r), host(v), host(g), im, dt, T, gamma, seed, 3)
    lv.kick_drift(r, v, g)
    assert lv.step == 4
    dr, dv = np.abs(host(r) - r1).max(), np.abs(host(v) - v1).max()
    print('step 3: |dr| %.2e of %.2e, |dv| %.2e of %.2e' % (dr, 16 * eps * np.abs(r1).max(), dv, 16 * eps * np.abs(v1).max()))
    assert dr <= 16 * eps * np.abs(r1).max() and dv <= 16 * eps * np.abs(v1).max()
    r_first, v_first = r.clone(), v.clone()

    v_before = host(v)
    lv.kick(r, v, g, want_ekin=True)
    v2 = v_before - 0.5 * dt * ACC * host(g) * im[:, None]
    ek = 0.5 * (v2 ** 2 / im[:, None]).sum() / ACC
    print('Ekin %.10e, restated %.10e' % (lv.kinetic_energy(), ek))
    assert abs(lv.kinetic_energy() - ek) <= 64 * eps * ek
    assert abs(lv.temperature() - 2.0 * ek / (3 * n * KB)) <= 64 * eps * 2.0 * ek / (3 * n * KB)
    assert torch.equal(r, r_first)                                       # the closing kick moves no atom

    r3, v3 = baoab_first_half(host(r), host(v), host(g), im, dt, T, gamma, seed, 4)
    _, v_old = baoab_first_half(host(r), host(v), host(g), im, dt, T, gamma, seed, 3)
    lv.kick_drift(r, v, g)
    assert lv.step == 5
    assert np.abs(host(r) - r3).max() <= 16 * eps * np.abs(r3).max() and np.abs(host(v) - v3).max() <= 16 * eps * np.abs(v3).max()
    assert np.abs(host(v) - v_old).max() > 1e3 * 16 * eps * np.abs(v3).max()      # not the noise of step 3 again

    again = Langevin(owner, mass, dt, T, gamma, seed)
    again.step = 3
    again.kick_drift(r_in, v_in, g)
    assert torch.equal(r_in, r_first) and torch.equal(v_in, v_first)


def test_without_friction_it_is_velocity_verlet(owner):
    """c1 = 1, c2sq_kT_acc = 0: one step equals VelocityVerlet.kick_drift to 4 eps max|.| (two half drifts round differently
    from one whole drift)"""
    from admp_amd.md import Langevin, VelocityVerlet
    eps = eps_of(owner)
    n = 900
    mass = np.tile(MASS, n // 3)
    rng = np.random.default_rng(2)
    r = dev(owner, rng.uniform(0.0, 20.8, size=(n, 3)))
    v = dev(owner, rng.normal(size=(n, 3)) * 1e-2)
    g = dev(owner, rng.normal(size=(n, 3)) * 50.0)
    ra, va = r.clone(), v.clone()
    lv = Langevin(owner, mass, 0.5, 300.0, 0.0, 11)
    assert lv.c1 == 1.0 and lv.c2sq_kT_acc == 0.0
    lv.kick_drift(r, v, g)
    VelocityVerlet(owner, mass, 0.5).kick_drift(ra, va, g)
    dr, dv = np.abs(host(r) - host(ra)).max(), np.abs(host(v) - host(va)).max()
    print('|dr| %.2e of %.2e, |dv| %.2e of %.2e' % (dr, 4 * eps * np.abs(host(ra)).max(), dv, 4 * eps * np.abs(host(va)).max()))
    assert dr <= 4 * eps * np.abs(host(ra)).max() and dv <= 4 * eps * np.abs(host(va)).max()


def test_ideal_gas_sits_at_the_temperature(owner):
    """4096 free atoms from rest, friction * dt = 0.05, 300 steps: T_kin of each of the last 100 steps within 5 sigma of T,
    sigma = sqrt(2 / 3n) (the restatement: mean 0.9988 T, worst step 2.3 sigma); in the last step the oxygens and the hydrogens
    each within 5 sigma of their own counts -- a missing or misplaced inverse mass under the square root fails that."""
    import torch
    from admp_amd.md import Langevin
    n, T = 4096, 300.0
    mass = np.tile(MASS, n // 3 + 1)[:n]
    r, v, g = (torch.zeros((n, 3), dtype=owner._dtype, device=owner._device) for _ in range(3))
    lv = Langevin(owner, mass, 1.0, T, 0.05, 5)
    temps = []
    for s in range(300):
        lv.kick_drift(r, v, g)
        lv.kick(r, v, g, want_ekin=s >= 200)
        if s >= 200:
            temps.append(lv.temperature())
    temps = np.array(temps)
    sigma = np.sqrt(2.0 / (3 * n))
    print('mean %.4f T, worst step %.2f sigma' % (temps.mean() / T, np.abs(temps / T - 1.0).max() / sigma))
    assert np.abs(temps / T - 1.0).max() <= 5.0 * sigma
    vh = host(v)
    for name, sel in (('O', mass > 2.0), ('H', mass < 2.0)):
        k = int(sel.sum())
        t = (mass[sel, None] * vh[sel] ** 2).sum() / (ACC * KB * 3 * k)
        print('%s: %d atoms, %.4f T, %.2f sigma' % (name, k, t / T, abs(t / T - 1.0) / np.sqrt(2.0 / (3 * k))))
        assert abs(t / T - 1.0) <= 5.0 * np.sqrt(2.0 / (3 * k)), name


def test_maxwell_boltzmann(owner):
    import torch
    from admp_amd.md import maxwell_boltzmann
    eps = eps_of(owner)
    n, T = 4096, 300.0
    mass = np.tile(MASS, n // 3 + 1)[:n]
    v = maxwell_boltzmann(owner, mass, T, 7)
    assert v.shape == (n, 3) and v.dtype == owner._dtype and v.is_cuda and v.is_contiguous()
    vh = host(v)
    p = np.abs((mass[:, None] * vh).sum(0)).max()
    print('momentum %.2e of %.2e' % (p, 64 * eps * (mass[:, None] * np.abs(vh)).sum()))
    assert p <= 64 * eps * (mass[:, None] * np.abs(vh)).sum()
    dof = 3 * n - 3
    t = (mass[:, None] * vh ** 2).sum() / (ACC * KB * dof)
    print('T %.2f K, %.2f sigma' % (t, abs(t / T - 1.0) / np.sqrt(2.0 / dof)))
    assert abs(t / T - 1.0) <= 5.0 * np.sqrt(2.0 / dof)
    assert torch.equal(v, maxwell_boltzmann(owner, mass, T, 7))
    assert not torch.equal(v, maxwell_boltzmann(owner, mass, T, 8))
    # with the centre of mass left in: the normals of stream 1, step 0 times sqrt(1e-4 kB T / m)
    raw = host(maxwell_boltzmann(owner, mass, T, 7, remove_com=False))
    want = ref_normals(n, 7, 0, 1) * np.sqrt(ACC * KB * T / mass)[:, None]
    # (two rounded factors and their product: 4 eps; on a double handle the two libm's differ by a few ulp more)
    assert np.abs(raw - want).max() <= 4 * max(eps, 1e-13) * np.abs(want).max()


def test_refusals(owner):
    """what would make the library read or write out of bounds is refused in Python before any launch; a bad kind or
    coefficient is the library's argument error (every pointer handed over here is valid for the n it comes with)"""
    import torch
    from admp_amd.md import Langevin
    n = 12
    mass = np.tile(MASS, n // 3)
    lv = Langevin(owner, mass, 0.5, 300.0, 0.05, 1)
    good = lambda: torch.zeros((n, 3), dtype=owner._dtype, device=owner._device)      # noqa: E731
    other = torch.float32 if owner._dtype == torch.float64 else torch.float64
    bad = [torch.zeros((n, 3), dtype=other, device=owner._device),                       # wrong precision
           torch.zeros((n, 6), dtype=owner._dtype, device=owner._device)[:, :3],         # non-contiguous view
           torch.zeros((n + 3, 3), dtype=owner._dtype, device=owner._device),            # wrong length
           torch.zeros((n, 3), dtype=owner._dtype)]                                      # host tensor
    for b in bad:
        for slot in range(3):
            args = [good(), good(), good()]
            args[slot] = b
            with pytest.raises(ValueError):
                lv.kick_drift(*args)
            with pytest.raises(ValueError):
                lv.kick(*args)
    assert lv.step == 0
    with pytest.raises(ValueError):
        Langevin(owner, mass, 0.5, -1.0, 0.05, 1)
    L, h, P = owner._L, owner._h, owner._ptr
    out = torch.zeros((n, 4), dtype=torch.int32, device=owner._device)
    assert L.admp_md_random(h, 2, n, 1, 0, 0, P(out)) == E_ARG
    assert L.admp_md_random(h, 0, -1, 1, 0, 0, P(out)) == E_ARG
    r, v, g = good(), good(), good()
    for c1, c2sq in ((1.5, 0.0), (-0.1, 0.0), (0.5, -1.0)):
        assert L.admp_md_langevin(h, n, P(r), P(v), P(g), P(lv.inv_mass), 0.25e-4, 0.5, c1, c2sq, 1, 0, None) == E_ARG
    assert L.admp_md_langevin(h, -1, P(r), P(v), P(g), P(lv.inv_mass), 0.25e-4, 0.5, 1.0, 0.0, 1, 0, None) == E_ARG
    torch.cuda.synchronize()
    assert not r.any() and not v.any() and not out.any()                 # nothing was launched


# ---- the driver ---------------------------------------------------------------------------------------------------------
DRIVER_ARGS = ['--waters', '216', '--steps', '200', '--minimize', '60', '--dt', '0.5']
BAND = 5.0 * np.sqrt(2.0 / 1944.0)      # 5 sigma of the instantaneous temperature of 648 atoms: 16 %


def run_driver(name, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'md', name)] + list(args), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize('pol', [False, True])
def test_nvt_water_holds_the_temperature(pol):
    """200 BAOAB steps (friction * time = 5) after the short minimisation: the mean kinetic temperature of the second half
    within 16 % of --temp"""
    out = run_driver('nvt_water.py', *DRIVER_ARGS, '--friction', '0.05', *(['--pol'] if pol else []))
    m = re.search(r'T_kin over the second half mean ([-+0-9.e]+) K std ([-+0-9.e]+) K', out)
    assert m, out[-800:]
    print(out.splitlines()[-1])
    assert 'ns/day' in out and 'T_kin' in out
    assert abs(float(m.group(1)) / 300.0 - 1.0) <= BAND, out[-800:]


def test_nve_water_alone_does_not_hold_it():
    """what the thermostat is for: the constant-energy driver on the same box with the same arguments ends outside the band
    (measured: T_final 439 K for --temp 300 -- the minimised synthetic box goes on turning potential into kinetic energy)"""
    out = run_driver('nve_water.py', *DRIVER_ARGS)
    m = re.search(r'T_final ([-+0-9.e]+) K', out)
    assert m, out[-800:]
    print(out.splitlines()[-1])
    assert abs(float(m.group(1)) / 300.0 - 1.0) > BAND, out[-800:]
