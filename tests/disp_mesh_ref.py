"""Reference, inputs and bars for the spread and gather legs of dispersion PME (admp_amd/csrc/disp_kernels.hip:
k_spread_bricks_scalar, k_spread_bricks_typed, k_interleave, k_gather_scalar and its typed form, k_gather_value, k_scalar_self,
k_types_check, k_type_counts, k_onehot; and the batch forms of the electrostatics kernels the site-row paths use), used by
tests/test_disp_mesh_ref_cpu.py (no GPU: reference, cases and bars are proved sound there), tests/test_disp_scale_cpu.py (the
scale rule behind the quanta) and tests/test_gpu_disp_mesh_legs.py (the legs alone through admp_disp_mesh_spread /
admp_disp_mesh_gather).

Reference.  tests/mesh_ref.py's, unchanged: a scalar channel p is a case whose sites carry Q[:, 0] = c_p and nothing else, a
type mesh one with unit charge on the atoms of that type.  SpreadRef / GatherRef then give, in long double from the inputs
rounded to the handle's type, the mesh, the absolute-weight mesh W, the term count t, the brick entries and counts, the words no
stencil reaches, pot[:, 0] (the mesh potential at the atoms: the value gather's mesh part), grad and their absolute versions.

Bars (reference-side quantities only; the scale is never read back; C = DEVICE_FACTOR x C_HOST[prec] of mesh_ref).

    spread, brick paths    C u W(n) + 1/2 q_b t(n), q_b the quantum of the word's brick by the rule of disp_math.h restated:
                           f32 q_b <= 2^-29 0.17 1.0001 bmax_b cnt_b x 1.001 (quantum_f32); f64 max(2^-61 0.17 1.0001 bmax_b
                           cnt_b, 2^-49 bmax_b, 2^-60) x 1.001 (quantum_f64); typed: bmax = 1 and 2^-49 in f64 (quantum_typed).
                           bmax_b, cnt_b: largest |c_p| over and number of the brick's entries.  A channel that is zero on
                           every entry of a brick has q_b = 0: its words are exact zeros (the ex = 20 branch).
    spread, site-row paths SpreadRef.bar of the form info8 names ('scan', 'bricks', 'planes')
    unreached words        exactly zero, in every mesh
    gradient               sum_p bar_grad_p + (nch + 1) u sum_p grad_abs_p per component (the second term: folding the channels
                           with the coefficients); typed: p runs over the one mesh of the atom's type, unit coefficient
    value gather           bar_pot[:, 0] + 2 u (|v| + |2 kp c|)
    self word              reference sum_p kp_p sum_i c_p,i^2, on typed paths sum_p kp_p sum_t n_t c_p,t^2 (they must agree);
                           bar (na + 16) 2^-53 sum |terms|

C was not widened: the device's scalar chain (scale c) ((Mx My) Mz) stayed inside C u W on every case (largest err / bar in
tests/test_gpu_disp_mesh_legs.py's docstring), so no C_HOST_SCALAR exists.

Meshes.  (32, 33, 35) triclinic: fused-x, 2 x 3 x 3 bricks of uneven widths (the fast_div branch of the tile store);
(30, 20, 24) triclinic: rocFFT 3-D, 2 x 2 x 2 bricks; (32, 17, 18) orthorhombic: 2 x 2 x 2 bricks of 16 + 16, 8 + 9, 9 + 9 --
17 has a prime factor above 13, so mesh_path takes the direct DFT for it without any switch and it is the default child's
direct-DFT mesh, not a fused-x one; (19, 22, 17) under ADMP_DFT=1; (32, 16, 18): one brick along y, the site-row fallback of
the bricks child.  expected_path restates mesh_path.h + disp_plan.h for these meshes; info8 must agree with it.

Cases are named for what they put in play; test_disp_mesh_ref_cpu.py asserts that they do."""
import functools

import numpy as np

from tests import mesh_ref as R
from tests.mesh_ref import LD, U, RT, PREC_BYTES, DEVICE_FACTOR, C_HOST      # noqa: F401
from tests.test_gpu_mesh_convolve import make_box, noise, wave

KAPPA = 0.55                      # only the self term and the value gather's 2 kp c read it
MESH_A, MESH_B, MESH_C, MESH_D, MESH_E = (32, 33, 35), (30, 20, 24), (32, 17, 18), (19, 22, 17), (32, 16, 18)
TRIC = {MESH_A: True, MESH_B: True, MESH_C: False, MESH_D: True, MESH_E: False}
# children of the GPU test: environment and meshes (at most three each)
CHILDREN = {'default': ({}, (MESH_A, MESH_B, MESH_C)),
            'bricks': ({'ADMP_SPREAD_BRICK_MIN': '0'}, (MESH_A, MESH_B, MESH_E)),
            'dft': ({'ADMP_DFT': '1'}, (MESH_D,)),
            'dft_bricks': ({'ADMP_DFT': '1', 'ADMP_SPREAD_BRICK_MIN': '0'}, (MESH_D,))}
BRICK_PATHS = ('BricksTyped', 'BricksBatched', 'BricksPerPower')
TYPED_PATHS = ('BricksTyped', 'DftTyped')


def kp(kappa=KAPPA):
    return np.array([-kappa ** 6 / 12.0, -kappa ** 8 / 48.0, -kappa ** 10 / 240.0])


# ---- the scale rule of disp_math.h restated as the bars take it (test_disp_scale_cpu.py: never finer than the header's) ---------
def quantum_f32(bmax, cnt):
    return 2.0 ** -29 * 0.17 * 1.0001 * np.asarray(bmax, dtype=np.float64) * np.maximum(cnt, 1) * 1.001


def quantum_f64(bmax, cnt):
    b = np.asarray(bmax, dtype=np.float64)
    return np.maximum(np.maximum(2.0 ** -61 * 0.17 * 1.0001 * b * np.maximum(cnt, 1), 2.0 ** -49 * b), 2.0 ** -60 * (b > 0)) * 1.001


def quantum_typed(prec, cnt):
    cnt = np.asarray(cnt, dtype=np.float64)
    return 2.0 ** -29 * 0.17 * np.maximum(cnt, 1) * 1.001 if prec == 'single' else np.full(cnt.shape, 2.0 ** -49 * 1.001)


# ---- which path a (mesh, child, pmax, nt, precision) reaches: mesh_path.h and disp_plan.h restated for the meshes above ----------
def mesh_is_direct(K, env):
    def hard(n):
        for p in (2, 3, 5, 7, 11, 13):
            while n > 1 and n % p == 0:
                n //= p
        return n > 1
    small = all(2 <= k <= 160 for k in K)
    return small and (env.get('ADMP_DFT') == '1' or any(hard(k) for k in K))


def uses_bricks(K, n, env):
    nb = R.make_bricks(K)
    m = int(env.get('ADMP_SPREAD_BRICK_MIN', 20000))
    wants = n >= m or (m > 0 and n >= 4096 and n >= 24 * nb[0] * nb[1] * nb[2])
    return wants and min(nb) > 1


def expected_path(K, n, env, pmax, nt, prec):
    """(path, nmesh, per_type)"""
    nch = (pmax - 4) // 2
    dft, bricks = mesh_is_direct(K, env), uses_bricks(K, n, env)
    fx = K[0] >= 32 and K[0] <= 1024 and K[0] & (K[0] - 1) == 0
    if not dft and bricks:
        if fx and prec == 'single' and 1 <= nt <= nch:
            return 'BricksTyped', nt, True
        if fx and nch >= 2:
            return 'BricksBatched', nch, False
        return 'BricksPerPower', nch, False
    if dft and not bricks and 1 <= nt < nch:
        return 'DftTyped', nt, True
    if dft and nch > 1:
        return 'DftBatched', nch, False
    return 'PerPower', nch, False


def expected_form(K, n, env):
    """the site-row paths' spread form (launch_spread's rule, as tests/test_gpu_mesh_spread_gather.py restates it)"""
    if min(R.make_bricks(K)) == 1:
        return 'scan'
    return 'bricks' if uses_bricks(K, n, env) else 'scan'


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def _coef(rng, n, signed):
    c = rng.uniform(0.5, 1.0, (n, 3)) * np.array([1.0, 3.0, 9.0])
    return c * rng.choice([-1.0, 1.0], (n, 3)) if signed else c


def _finish(name, K, rm, c, rng, pmaxes, types=None, ctab=None, shift=True, precs=('double', 'single'), **extra):
    K = tuple(K)
    box = make_box(K, TRIC[K])
    n = len(rm)
    frac = rm / np.array(K, dtype=np.float64)
    if shift and n >= 8:                     # atoms outside the cell, two of them 50 cells away
        sel = rng.permutation(n)[:max(2, n // 8)]
        frac[sel] += rng.integers(-2, 3, (len(sel), 3))
        frac[sel[0]] += np.array([50, -50, 50])
        frac[sel[1]] -= np.array([50, 0, -50])
        extra['shifted'] = sel
    if types is not None:
        c = np.asarray(ctab)[types]
    d = dict(name=name, K=K, tric=TRIC[K], box=box, n=n, pos=frac @ box, c=np.array(c, dtype=np.float64), pmaxes=tuple(pmaxes),
             types=None if types is None else np.asarray(types, dtype=np.int32), ctab=None if ctab is None else np.asarray(ctab, dtype=np.float64),
             nt=0 if types is None else len(ctab), precs=tuple(precs), pairs=np.zeros((0, 2), dtype=np.int32), kappa=KAPPA)
    d.update(extra)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _uniform(rng, K, n):
    return rng.uniform(0, 1, (n, 3)) * np.array(K)


def _case_n1(rng):
    return _finish('n1', MESH_A, np.array([[7.6, 8.4, 10.7]]), _coef(rng, 1, True), rng, (10,))


def _case_n31(rng):            # one partial workgroup of the gather; negative coefficients; atoms exactly on mesh points
    K = MESH_B
    rm = np.concatenate([R._special(K, rng)[:12], _uniform(rng, K, 19)])
    return _finish('n31_negative_onpoints', K, rm, _coef(rng, 31, True), rng, (8,), on_points=np.arange(2))


def _case_n33(rng):            # the second workgroup of the gather; atoms with an all-zero row
    c = _coef(rng, 33, True)
    zero = np.array([0, 7, 32])
    c[zero] = 0.0
    return _finish('n33_zero_rows', MESH_A, _uniform(rng, MESH_A, 33), c, rng, (6, 8), zero_rows=zero)


def _case_n65(K, name):
    def build(rng):
        rm = np.concatenate([R._special(K, rng), _uniform(rng, K, 65 - len(R._special(K, rng)))])[:65]
        return _finish(name, K, rm, _coef(rng, 65, True), rng, (6, 8, 10))
    return build


TYPES3 = np.array([[1.0, 3.1, 8.7], [0.61, 2.2, 5.9], [0.0, 0.0, 0.0]])


def _case_n257_typed(rng):     # second workgroup of k_types_check / k_onehot; a minority of 3 atoms; a type whose row is all zero
    n = 257
    types = np.zeros(n, dtype=np.int32)
    types[[5, 130, 256]] = 1
    types[10:20] = 2
    return _finish('n257_nt3_minority', MESH_A, _uniform(rng, MESH_A, n), None, rng, (10,), types=types, ctab=TYPES3, minority=1)


def _case_typed_empty(K, name, pmaxes, n=65):
    def build(rng):            # nt = 2 with a type that no atom has
        return _finish(name, K, _uniform(rng, K, n), None, rng, pmaxes, types=np.zeros(n, dtype=np.int32), ctab=TYPES3[:2], empty_type=1)
    return build


def _case_typed_nt1(K, name, pmaxes):
    def build(rng):
        return _finish(name, K, _uniform(rng, K, 40), None, rng, pmaxes, types=np.zeros(40, dtype=np.int32), ctab=TYPES3[:1])
    return build


def _case_typed_dft(rng):      # nt = 2 < nch = 3 on the direct-DFT meshes: DftTyped; 257 atoms: two workgroups of k_onehot
    n = 257
    types = (rng.random(n) < 0.3).astype(np.int32)
    types[256] = 1
    return _finish('n257_nt2_dft', MESH_D, _uniform(rng, MESH_D, n), None, rng, (10,), types=types, ctab=TYPES3[:2])


CROWDED = (1, 1, 1)
ZERO_C8 = (0, 2, 0)


def _case_crowded(rng):        # ~600 entries in one brick beside sparse and empty ones; five atoms 1000 x the rest, C10 = 1e4 C6
    K = MESH_A
    rm = np.concatenate([R._inside(rng, K, CROWDED, 600), R._inside(rng, K, (0, 0, 0), 20), R._inside(rng, K, ZERO_C8, 12)])
    c = _coef(rng, len(rm), False)
    big = np.arange(5)
    c[big] *= 1000.0
    c[big, 2] = 1e4 * c[big, 0]
    z8 = np.arange(620, 632)
    c[z8, 1] = 0.0              # C8 is zero on every atom of one brick: its exponent takes the ex = 20 branch
    return _finish('crowded_range', K, rm, c, rng, (10,), shift=False, big=big, crowded=CROWDED, zero_c8=z8, zero_c8_brick=ZERO_C8)


def _case_xplane(rng):         # all atoms in one x plane
    K = MESH_B
    rm = _uniform(rng, K, 40)
    rm[:, 0] = 11.0 + rng.uniform(0.05, 0.95, 40)
    return _finish('xplane_n40', K, rm, _coef(rng, 40, True), rng, (10,), shift=False)


def _case_typed_2100(rng):     # two workgroups of k_type_counts, two chunks of a brick list (more than 2048 entries in one brick)
    K = MESH_A
    rm = np.concatenate([R._touching(rng, K, CROWDED, 2080), _uniform(rng, K, 20)])
    types = (rng.random(2100) < 0.4).astype(np.int32)
    return _finish('n2100_nt2_chunks', K, rm, None, rng, (8,), types=types, ctab=TYPES3[:2], shift=False, crowded=CROWDED)


_BUILDERS = {'n1': _case_n1, 'n31_negative_onpoints': _case_n31, 'n33_zero_rows': _case_n33,
             'n65_general': _case_n65(MESH_A, 'n65_general'), 'n65_rocfft': _case_n65(MESH_B, 'n65_rocfft'),
             'n65_dft17': _case_n65(MESH_C, 'n65_dft17'), 'n65_dft': _case_n65(MESH_D, 'n65_dft'),
             'n65_one_brick_y': _case_n65(MESH_E, 'n65_one_brick_y'), 'n257_nt3_minority': _case_n257_typed,
             'n65_nt2_empty_type': _case_typed_empty(MESH_A, 'n65_nt2_empty_type', (8, 10)), 'n40_nt1': _case_typed_nt1(MESH_C, 'n40_nt1', (8,)),
             'n40_nt1_fx': _case_typed_nt1(MESH_A, 'n40_nt1_fx', (6,)),
             'n257_nt2_dft': _case_typed_dft, 'crowded_range': _case_crowded, 'xplane_n40': _case_xplane,
             'n2100_nt2_chunks': _case_typed_2100}
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name](np.random.default_rng(2000 + CASES.index(name)))


def _site_case(c, q):
    """the mesh_ref case of one scalar channel: charge-only sites"""
    Q = np.zeros((c['n'], 9))
    Q[:, 0] = q
    return dict(name=c['name'], K=c['K'], box=c['box'], n=c['n'], pos=c['pos'], Q=Q, U=np.zeros((c['n'], 3)), lpol=False)


@functools.lru_cache(maxsize=None)
def channel_ref(name, prec, p):
    c = case(name)
    return R.SpreadRef(_site_case(c, c['c'][:, p]), prec)


@functools.lru_cache(maxsize=None)
def type_ref(name, prec, t):
    c = case(name)
    return R.SpreadRef(_site_case(c, (c['types'] == t).astype(np.float64)), prec)


def rounded_c(c, prec):
    return np.asarray(c['c'], dtype=RT[prec]).astype(np.float64)


def rounded_ctab(c, prec):
    return np.asarray(c['ctab'], dtype=RT[prec]).astype(np.float64)


def brick_quantum(r, q, prec, typed=False):
    """per-word quantum of the dispersion brick spreads for the SpreadRef r of a channel with coefficients q (rounded)"""
    K = r.K
    nb = R.make_bricks(K)
    ncell = nb[0] * nb[1] * nb[2]
    cnt = r.cnt                                   # every atom's entries, whatever its coefficient (the list is by position)
    if typed:
        qc = quantum_typed(prec, cnt.astype(np.float64))
    else:
        bmax = np.zeros(ncell)
        np.maximum.at(bmax, r.ent_cell, np.abs(q)[r.ent_atom])
        qc = (quantum_f32 if prec == 'single' else quantum_f64)(bmax, cnt)
    return qc[R.word_bricks(K)]


def spread_bar_bricks(r, q, prec, typed=False):
    u = U[prec]
    return DEVICE_FACTOR * C_HOST[prec] * u * r.W + 0.5 * brick_quantum(r, q, prec, typed) * r.t


def mesh_refs(name, prec, pmax, per_type):
    """the SpreadRefs of the meshes of a call: one per power, or one per type"""
    c = case(name)
    if per_type:
        return [type_ref(name, prec, t) for t in range(c['nt'])]
    return [channel_ref(name, prec, p) for p in range((pmax - 4) // 2)]


def phi_batch(c, prec, nmesh, kind='noise'):
    """a different mesh per member of the batch: a swapped channel or type shows"""
    K = c['K']
    if kind == 'noise':
        return np.stack([noise(K, 77 + 13 * b, PREC_BYTES[prec]).astype(np.float64) for b in range(nmesh)])
    ms = [(1, 2 % max(1, K[1] // 2), 1), (2, 1, 3 % max(1, K[2] // 2)), (3, 1, 2)]
    return np.stack([wave(K, ms[b], PREC_BYTES[prec]).astype(np.float64) for b in range(nmesh)])


def gather_reference(name, prec, pmax, per_type, phi):
    """grad (n, 3) and its bar for meshes phi (nmesh, K): per power phi_p, or per type psi_t"""
    c = case(name)
    nch = (pmax - 4) // 2
    refs = mesh_refs(name, prec, pmax, per_type)
    grad, bar, gabs = 0.0, 0.0, 0.0
    for b, r in enumerate(refs):
        g = R.GatherRef(r, phi[b])
        grad = grad + g.grad
        bar = bar + g.bars()['grad']
        gabs = gabs + g.grad_abs
    return grad, bar + (nch + 1) * U[prec] * gabs


def value_reference(name, prec, pmax, phi, kappa=KAPPA):
    """(n, 3) out of which = 1 and its bar: column p = phi_p(r_i) + 2 kp_p c_p,i; columns of unused powers stay zero"""
    c = case(name)
    nch = (pmax - 4) // 2
    cr = rounded_c(c, prec)
    out, bar = np.zeros((c['n'], 3)), np.zeros((c['n'], 3))
    for p in range(nch):
        g = R.GatherRef(channel_ref(name, prec, p), phi[p])
        v, extra = g.pot[:, 0], 2.0 * kp(kappa)[p] * cr[:, p]
        out[:, p] = v + extra
        bar[:, p] = g.bars()['pot'][:, 0] + 2.0 * U[prec] * (np.abs(v) + np.abs(extra))
    return out, bar


def self_reference(c, prec, pmax, kappa=KAPPA):
    """(E_self, bar, E_self by types or None)"""
    nch = (pmax - 4) // 2
    cr = rounded_c(c, prec)
    terms = kp(kappa)[None, :nch] * cr[:, :nch] ** 2
    e = float(terms.astype(LD).sum())
    bar = (c['n'] + 16) * 2.0 ** -53 * float(np.abs(terms).sum())
    et = None
    if c['types'] is not None:
        tab = rounded_ctab(c, prec)
        nt_ = np.bincount(c['types'], minlength=c['nt']).astype(np.float64)
        et = float((kp(kappa)[None, :nch] * nt_[:, None] * tab[:, :nch] ** 2).astype(LD).sum())
    return e, bar, et


# ---- composition: the legs' conventions against the oracle ---------------------------------------------------------------------
# two cases per brick path (bricks child): (case, pmax, with the type table, precision)
COMPOSITION = (('n257_nt3_minority', 10, True, 'single'), ('n65_nt2_empty_type', 8, True, 'single'),
               ('n65_general', 10, False, 'double'), ('n33_zero_rows', 8, False, 'single'),
               ('n65_rocfft', 10, False, 'double'), ('n33_zero_rows', 6, False, 'single'))


def composition(name, prec, pmax, per_type, kappa=KAPPA):
    """(phi (nmesh, K), oracle gradient (n, 3)): phi_p = N ifftn(G_p fftn(mesh_p)) in float64 from the REFERENCE mesh of every
    power, with the oracle's own k-point table (its default order; the handle's default too), or psi_t = sum_p c_p,t phi_p per
    type; and the gradient of oracle.admp_oracle.disp_energy_and_grad without pairs -- its reciprocal part alone (the self
    term does not depend on the positions) -- for the inputs rounded to the handle's type."""
    from oracle import admp_oracle as O
    from tests.test_gpu_mesh_convolve import g_table, half_spectrum_table
    c = case(name)
    K, nch = c['K'], (pmax - 4) // 2
    box = np.array(c['box'])
    phi = []
    for p in range(nch):
        G = half_spectrum_table(g_table(box, K, kappa, 6 + 2 * p, ref_order=True))
        m = np.asarray(channel_ref(name, prec, p).mesh, dtype=np.float64)
        phi.append(np.fft.ifftn(G * np.fft.fftn(m)).real * float(np.prod(K)))
    phi = np.stack(phi)
    if per_type:
        tab = rounded_ctab(c, prec)
        phi = np.stack([sum(tab[t, p] * phi[p] for p in range(nch)) for t in range(c['nt'])])
    cr = np.array(rounded_c(c, prec))
    cr[:, nch:] = 0.0
    pos = np.asarray(c['pos'], dtype=RT[prec]).astype(np.float64)
    o = O.disp_energy_and_grad(pos, box, np.zeros((0, 2), dtype=np.int32), cr, np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0]),
                               R.EmptyCov(c['n']), kappa, list(K), pmax)
    return phi, np.asarray(o['grad'], dtype=np.float64)


# ---- mutants: what a defect changes, over the bar of what it changes -----------------------------------------------------------------
def _ratio(change, bar):
    change, bar = np.abs(np.asarray(change, dtype=np.float64)), np.asarray(bar, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(bar > 0, change / bar, np.where(change > 0, np.inf, 0.0))


def mutant_entry_dropped(name, prec, p):
    """per atom with a non-zero c_p: an (atom, brick) entry lost from the brick spread of channel p"""
    c = case(name)
    r = channel_ref(name, prec, p)
    q = rounded_c(c, prec)[:, p]
    m = R.mutant_ratios(_BarView(r, spread_bar_bricks(r, q, prec)), 'bricks')
    show = q != 0
    if 'big' in c and prec == 'single':
        # the f32 quantum of the crowded brick is set by its five large atoms (that is the case's purpose): the other atoms of
        # that brick lie below it by construction, in every kernel that keeps the scale rule.  The mutant runs on the five and
        # on the atoms of the other bricks.
        nb = R.make_bricks(c['K'])
        cell = (c['crowded'][0] * nb[1] + c['crowded'][1]) * nb[2] + c['crowded'][2]
        inside = np.zeros(c['n'], dtype=bool)
        inside[r.ent_atom[r.ent_cell == cell]] = True
        inside[c['big']] = False
        show = show & ~inside
    return m['entry'][show], m['column'][show]


class _BarView:
    """a SpreadRef with this module's bar in place of its own (mesh_ref.mutant_ratios reads r.bar)"""

    def __init__(self, r, bar):
        self._r, self._bar = r, bar

    def __getattr__(self, k):
        return getattr(self._r, k)

    def bar(self, form, C=None):
        return self._bar


def mutant_wrong_tile(name, prec):
    """per atom: spread into another type's tile -- its words are missing from its own type's mesh"""
    c = case(name)
    out = []
    for t in range(c['nt']):
        sel = c['types'] == t
        if not sel.any():
            continue
        r = type_ref(name, prec, t)
        bar = spread_bar_bricks(r, None, prec, typed=True).reshape(-1)
        rt = _ratio(r.vals, bar[r.idx])
        out.append(rt.max(axis=(1, 2, 3))[sel])
    return np.concatenate(out)


def mutant_gather(name, prec, pmax, kind):
    """per atom, largest change / bar over the components of the gradient on the noise: 'swap' -- the coefficients of channels
    0 and 1 exchanged; 'stride' -- the row read one channel on (c_p+1 for c_p, the next atom's c_0 for the last); 'zcol' -- one
    z column of the stencil dropped (the column that shows most).  Atoms the mutant cannot touch are left out (mask returned)."""
    c = case(name)
    nch = (pmax - 4) // 2
    cr = rounded_c(c, prec)
    phi = phi_batch(c, prec, nch)
    _, bar = gather_reference(name, prec, pmax, False, phi)
    unit = []                                                   # gradient of a unit coefficient per channel: Jac . F1
    for p in range(nch):
        r = channel_ref(name, prec, p)
        F = R.f_sums(phi[p].reshape(-1)[r.idx].astype(LD), r.Wt)
        F1 = np.stack([F[:, R.FI[(1, 0, 0)]], F[:, R.FI[(0, 1, 0)]], F[:, R.FI[(0, 0, 1)]]], axis=1)
        unit.append(np.asarray(F1 @ r.g.Jac.T, dtype=np.float64))
    if kind in ('swap', 'stride'):
        flat = np.concatenate([cr.reshape(-1), [0.0]])
        cm = np.array(cr, copy=True)
        if kind == 'swap':
            cm[:, [0, 1]] = cr[:, [1, 0]]
        else:
            cm = flat[1:].reshape(-1, 3)
        touched = (cm[:, :nch] != cr[:, :nch]).any(axis=1)
        change = sum((cm[:, p:p + 1] - cr[:, p:p + 1]) * unit[p] for p in range(nch))
        return _ratio(change, bar).max(axis=1)[touched], touched
    best = np.zeros(c['n'])
    for lane in range(6):
        change = 0.0
        for p in range(nch):
            r = channel_ref(name, prec, p)
            Fm = R.f_sums(phi[p].reshape(-1)[r.idx].astype(LD), r.Wt, drop_z=np.full(c['n'], lane))
            _, gm = R.unfold(r.g.Aop, r.g.Jac, None, r.coef, Fm)
            change = change + (np.asarray(gm, dtype=np.float64) - R.GatherRef(r, phi[p]).grad)
        best = np.maximum(best, _ratio(change, bar).max(axis=1))
    touched = (cr[:, :nch] != 0).any(axis=1)
    return best[touched], touched


def mutant_self(c, prec, pmax, kappa=KAPPA):
    """|change| / bar of the self word when channel 0 takes the kp of the neighbouring power"""
    e, bar, _ = self_reference(c, prec, pmax, kappa)
    cr = rounded_c(c, prec)
    change = (kp(kappa)[1] - kp(kappa)[0]) * float((cr[:, 0] ** 2).sum())
    return abs(change) / bar if bar > 0 else (np.inf if change else 0.0)
