"""Reference, inputs and bars for the mesh spread and gather kernels (admp_amd/csrc/recip_kernels.hip: k_spread_scan,
k_spread_planes, k_bin + k_spread_bricks, k_gather_staged, k_gather_field_staged; dft_kernels.hip: zy_plane_spread), used by
tests/test_mesh_ref_cpu.py (no GPU: reference, cases and bars are proved sound there) and by
tests/test_gpu_mesh_spread_gather.py (the kernels alone through the C entries admp_mesh_spread / admp_mesh_gather).

Reference.  From the inputs rounded to the handle's type, in numpy's long double (64-bit mantissa on x86: u = 5.4e-20, three
decimal orders below float64), with the B-splines by the Cox-de Boor recursion (sums of non-negative terms).  The oracle's
spread_Q builds its splines from truncated powers, sum_k binom (u - k)^5 / 120 with terms up to 20 * 6^5 / 120: in float64 that
is accurate to ~1e-13 absolute, a thousand float64 roundings, so it cannot referee a float64 kernel word by word.  The CPU test
proves the recursion reference equal to oracle.spread_Q (mesh) and to autograd of sum phi * spread_Q (pot, grad) at that
accuracy; the GPU test compares with the recursion reference.  Sites carry no axis atoms (identity frame): Q_global = Q_local,
dipole slots + U in harmonic order (z, x, y).

Bars (first order in u = 2^-24 / 2^-53, reference-side quantities only).  Per mesh word n

    err(n) <= C u W(n) + Q(n)

    W(n) = W0(n) + Wc(n).  W0: the spread of the absolute folded multipoles (|q| + |U|, |d| |Aop|, |Aop|^T |Theta/3| |Aop| with
           |Theta| built from absolute harmonic components) with absolute weights.  Wc: the same with the weights of one axis
           replaced by the next derivative, times X_d = K_d sum_i |r_i| |box^-1[i][d]| >= |K frac|, summed over the axes: what
           a rounding error of the fractional coordinate (u X_d per operation) does to the weights; it also covers a stencil
           that starts one point earlier or later than the reference's (atoms on mesh points: the spline is continuous).
    Q(n):  the fixed-point quantum of the brick form, half a quantum per term that reaches the word (t(n), counted in the
           reference): f32 quantum <= 2^-29 bound, bound = (largest entry bound of the brick) x (entries of the brick) -- the
           entry-count contract; the stencil-window scale is never coarser -- with the entry bound 0.55^3 |q| + 0.46004 0.55^2
           amax |d|_1 + 0.55^2 2 amax^2 |Theta|_1 of the kernel's header comment; f64 quantum <= max(2^-58 bmax cnt, 2^-49
           bmax, 2^-60) with bmax = |q| + amax |d|_1 + 2 amax^2 |Theta|_1.  Both carry the kernel's safety factor 1.0001 and
           a float rounding: x 1.001.  The scale is never read back from the kernel.  The scan form sums 64-bit words under
           the f64 rule at both precisions (its brick's entries: the atoms whose stencil meets the brick) and gets that Q.
    C:     measured on the CPU as the largest err / (u W) of the HOST-compiled arithmetic (tests/hostshim: the same inline
           functions, atoms summed in double) over all cases, per type: C_HOST below.  The device gets DEVICE_FACTOR = 4 times
           that (contraction, another summation order, v_cvt rounding).  C_CAP bounds C_host from the operation chain, so that
           a defect in the shared headers cannot widen its own bar (count in test_mesh_ref_cpu.py).

The gather is bound likewise per output: C u times the sums of |w| |phi| (and their coordinate term) unfolded through |Aop|
and |Jac| with the absolute multipoles.  Energy word: |E - E_ref| <= 1/2 sum |Q| bar(pot) + Na 2^-53 |E_ref|.

Cases: general sites, three classes (general, dipole only, charge only), half of them on a triclinic cell, atoms outside the
cell and up to 50 cells away.  Each case is named for what it puts in play; test_mesh_ref_cpu.py asserts that it does."""
import functools
import math

import numpy as np

from tests.test_gpu_mesh_convolve import make_box, noise, wave, g_table, flat_kappa, half_spectrum_table      # noqa: F401

LD = np.longdouble
U = {'single': 2.0 ** -24, 'double': 2.0 ** -53}
RT = {'single': np.float32, 'double': np.float64}
PREC_BYTES = {'single': 4, 'double': 8}
DEVICE_FACTOR = 4.0
# largest err / (u W) of the host-compiled arithmetic over all cases: measured 4.25 and 2.74 (test_mesh_ref_cpu.py measures
# and asserts <= these), rounded up in the third digit only
C_HOST = {'single': 4.3, 'double': 2.75}
C_CAP = 120.0
SQRT3 = math.sqrt(3.0)
KIND_GENERAL, KIND_DIPOLE, KIND_CHARGE = 0, 1, 2
SCAN_ROUND = 3072        # kScanChunk of k_spread_scan, kZyScan * kZyBlock of zy_plane_spread
BRICK_CHUNK = 2048       # kBrickChunk of k_spread_bricks
# the ten terms of a site's mesh value: (order along x, y, z) of q, c1[0..2], c2[00, 11, 22, 01, 02, 12]
TERMS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1)]
T_CHARGE, T_DIPOLE, T_QUAD = [0], [1, 2, 3], [4, 5, 6, 7, 8, 9]


# ---- splines and geometry ---------------------------------------------------------------------------------------------------
def bspline6(f):
    """M6 and its first four derivatives at u = f + p, p = 0..5, by the Cox-de Boor recursion: list of five (n, 6) arrays"""
    f = np.asarray(f)
    n = f.shape[0]
    z = np.zeros(n, dtype=f.dtype)
    a = [None, None, [f, 1 - f, z, z, z, z]]
    for order in range(3, 7):
        src, dst = a[order - 1], []
        for p in range(6):
            lo = src[p - 1] if p > 0 else z
            hi = src[p] if p < order - 1 else z
            dst.append(((f + p) * hi + (order - f - p) * lo) / (order - 1) if p < order else z)
        a.append(dst)

    def diff(src, k):
        co = [1, -1], [1, -2, 1], [1, -3, 3, -1], [1, -4, 6, -4, 1]
        return [sum(c * src[p - j] for j, c in enumerate(co[k - 1]) if p - j >= 0) for p in range(6)]
    out = [a[6], diff(a[5], 1), diff(a[4], 2), diff(a[3], 3), diff(a[2], 4)]
    return [np.stack([np.asarray(x, dtype=f.dtype) + z for x in w], axis=1) for w in out]


class Geom:
    def __init__(self, box, K, dtype=LD):
        self.K = tuple(int(k) for k in K)
        self.inv = np.linalg.inv(np.asarray(box, dtype=np.float64)).astype(dtype)
        if dtype is LD:      # one Newton step: the inverse to long-double accuracy
            b = np.asarray(box, dtype=LD)
            self.inv = self.inv + self.inv @ (np.eye(3, dtype=LD) - b @ self.inv)
        Kv = np.array(self.K, dtype=dtype)
        self.Aop = -(Kv[:, None] * self.inv.T)           # Aop[i][j] = -K[i] inv[j][i]
        self.Jac = -(Kv[None, :] * self.inv)             # Jac[i][j] = -K[j] inv[i][j]
        self.dtype = dtype

    def stencil(self, pos):
        """base (n, 3) int, weights W[d][order] (n, 6), X (n, 3) = K_d sum_i |r_i| |inv[i][d]|"""
        pos = np.asarray(pos, dtype=self.dtype)
        Kv = np.array(self.K, dtype=self.dtype)
        rm = (pos @ self.inv) * Kv
        c = np.ceil(rm)
        base = np.mod(c.astype(np.int64) - 3, np.array(self.K, dtype=np.int64))
        f = c - rm
        W = [bspline6(f[:, d]) for d in range(3)]
        X = (np.abs(pos) @ np.abs(self.inv)) * Kv
        return base, W, X, rm


def qtot(Q, Ucart):
    """Q_global_tot: dipole slots (10, 11c, 11s) = (z, x, y) plus the induced dipole"""
    q = np.array(Q, copy=True)
    if Ucart is not None:
        q[:, 1] += Ucart[:, 2]
        q[:, 2] += Ucart[:, 0]
        q[:, 3] += Ucart[:, 1]
    return q


def fold(g, Q):
    """(n, 10) coefficients of TERMS from the total global multipoles (spline_math.h fold_multipole)"""
    A = g.Aop
    d = np.stack([Q[:, 2], Q[:, 3], Q[:, 1]], axis=1)
    c1 = d @ A
    r3 = np.sqrt(g.dtype(3))
    h = r3 / 6
    tzz = Q[:, 4] / 3
    txx = (-Q[:, 4] + r3 * Q[:, 7]) / 6
    tyy = (-Q[:, 4] - r3 * Q[:, 7]) / 6
    txz, tyz, txy = h * Q[:, 5], h * Q[:, 6], h * Q[:, 8]
    Th = np.stack([np.stack([txx, txy, txz], 1), np.stack([txy, tyy, tyz], 1), np.stack([txz, tyz, tzz], 1)], axis=1)
    c2 = np.einsum('im,kij,jn->kmn', A, Th, A)
    return np.stack([Q[:, 0], c1[:, 0], c1[:, 1], c1[:, 2], c2[:, 0, 0], c2[:, 1, 1], c2[:, 2, 2], 2 * c2[:, 0, 1],
                     2 * c2[:, 0, 2], 2 * c2[:, 1, 2]], axis=1)


def fold_abs(g, Qabs):
    """the same from absolute values at every step (float64): an upper bound of |coefficient| and of its rounding scale"""
    A = np.abs(np.asarray(g.Aop, dtype=np.float64))
    Q = np.asarray(Qabs, dtype=np.float64)
    d = np.stack([Q[:, 2], Q[:, 3], Q[:, 1]], axis=1)
    c1 = d @ A
    h = 0.5 * SQRT3 / 3
    tzz = Q[:, 4] / 3
    txx = (Q[:, 4] + SQRT3 * Q[:, 7]) / 6
    txz, tyz, txy = h * Q[:, 5], h * Q[:, 6], h * Q[:, 8]
    Th = np.stack([np.stack([txx, txy, txz], 1), np.stack([txy, txx, tyz], 1), np.stack([txz, tyz, tzz], 1)], axis=1)
    c2 = np.einsum('im,kij,jn->kmn', A, Th, A)
    return np.stack([Q[:, 0], c1[:, 0], c1[:, 1], c1[:, 2], c2[:, 0, 0], c2[:, 1, 1], c2[:, 2, 2], 2 * c2[:, 0, 1],
                     2 * c2[:, 0, 2], 2 * c2[:, 1, 2]], axis=1)


def point_values(coef, W, terms=range(10), bump=None, absw=False):
    """(n, 6, 6, 6) values of every atom at its stencil points: sum over `terms` of coef W0^(a) W1^(b) W2^(c); bump = d: the
    order along axis d raised by one"""
    out = 0
    for t in terms:
        o = list(TERMS[t])
        if bump is not None:
            o[bump] += 1
        w = [W[d][o[d]] for d in range(3)]
        if absw:
            w = [np.abs(x) for x in w]
        out = out + coef[:, t, None, None, None] * w[0][:, :, None, None] * w[1][:, None, :, None] * w[2][:, None, None, :]
    return out


def point_index(base, K):
    """(n, 6, 6, 6) flat mesh index of every stencil point"""
    p = np.arange(6)
    ix = [(base[:, d, None] + p[None, :]) % K[d] for d in range(3)]
    return (ix[0][:, :, None, None] * K[1] + ix[1][:, None, :, None]) * K[2] + ix[2][:, None, None, :]


def scatter(idx, vals, K, keep=None):
    out = np.zeros(K[0] * K[1] * K[2], dtype=vals.dtype)
    if keep is not None:
        idx, vals = idx[keep], vals[keep]
    if vals.dtype == np.float64:
        return np.bincount(idx.reshape(-1), weights=vals.reshape(-1), minlength=out.size).reshape(K)
    np.add.at(out, idx.reshape(-1), vals.reshape(-1))
    return out.reshape(K)


# ---- the brick rule of brick_plan.h, restated (checked against the host-compiled header in test_mesh_ref_cpu.py) -------------
def make_bricks(K):
    return tuple((k + 15) // 16 for k in K)


def brick_of(i, nb, K):
    return ((i + 1) * nb - 1) // K


def brick_lo(b, nb, K):
    return (b * K) // nb


def brick_code(base, K):
    nb = make_bricks(K)
    code = 0
    for d in range(3):
        b = brick_of(int(base[d]), nb[d], K[d])
        end = ((b + 1) * K[d]) // nb[d]
        code |= b << (9 * d)
        if nb[d] > 1 and base[d] + 5 >= end:
            code |= 1 << (27 + d)
    return code


def brick_entries(base, K):
    """(atom, brick id) entries of k_bin: the brick of the stencil's base and, where the reach bit is set, the next one
    (periodic) on that axis; brick id = (bx nby + by) nbz + bz"""
    nb = make_bricks(K)
    atoms, cells = [], []
    for i in range(len(base)):
        code = brick_code(base[i], K)
        b = [[(code >> (9 * d)) & 511] for d in range(3)]
        for d in range(3):
            if (code >> (27 + d)) & 1:
                b[d].append((b[d][0] + 1) % nb[d])
        for x in b[0]:
            for y in b[1]:
                for z in b[2]:
                    atoms.append(i)
                    cells.append((x * nb[1] + y) * nb[2] + z)
    return np.array(atoms, dtype=np.int64), np.array(cells, dtype=np.int64)


def word_bricks(K):
    """brick id of every mesh word, (K1, K2, K3)"""
    nb = make_bricks(K)
    b = [brick_of(np.arange(K[d]), nb[d], K[d]) for d in range(3)]
    return (b[0][:, None, None] * nb[1] + b[1][None, :, None]) * nb[2] + b[2][None, None, :]


def site_kinds(Qt):
    d = np.abs(Qt[:, 1:4]).sum(1)
    q2 = np.abs(Qt[:, 4:9]).sum(1)
    return np.where((q2 == 0) & (d == 0), KIND_CHARGE, np.where((q2 == 0) & (Qt[:, 0] == 0), KIND_DIPOLE, KIND_GENERAL))


def direct_dft_by_default(K):
    """mesh_path (csrc/mesh_path.h) without ADMP_DFT: every axis at most 160 points and one of them with a prime factor above 13"""
    def lpf(n):
        f, p = 1, 2
        while n > 1:
            while n % p == 0:
                f, n = p, n // p
            p += 1
        return f
    return all(2 <= k <= 160 for k in K) and any(lpf(k) > 13 for k in K)


def plane_spread_fits(K, n, prec):
    """dft_zy_spread_fits of dft_kernels.hip: double precision, at most 8192 atoms, two workgroups per plane in one round,
    the plane and its spectrum in 160 KB of LDS, room for at least 16 staged atoms next to the hit list"""
    if prec != 'double' or not (0 < n <= 8192) or 2 * K[0] > 256 or max(K) > 160:
        return False
    N2, N3 = K[1], K[2]
    H3, Kh, cx = (N3 - 1) // 2, N3 // 2 + 1, 16
    total = cx * N3 + cx * N2 + max(cx * H3 * N2, cx * N2 * Kh) + cx * N2 + cx * N2 * Kh
    if total + 2048 > 160 * 1024:
        return False
    spare = cx * N2 * Kh - 2 * 3 * 1024
    return min(spare // (42 * 8 + 8), 1024 // 3) >= 16


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _sites(rng, n):
    """every moment between half and all of its slot's scale, random sign: no site is invisible next to its neighbours"""
    return rng.uniform(0.5, 1.0, (n, 9)) * rng.choice([-1.0, 1.0], (n, 9)) * np.array([1, .5, .5, .5, .3, .3, .3, .3, .3])


def _set_kind(Q, idx, kind):
    if kind == KIND_CHARGE:
        Q[idx, 1:] = 0.0
    elif kind == KIND_DIPOLE:
        Q[idx, 0] = 0.0
        Q[idx, 4:] = 0.0


def _inside(rng, K, cell, n):
    """n mesh coordinates whose whole stencil lies in brick `cell`: base in [lo, lo + len - 6], rm in (base + 2, base + 3)"""
    nb = make_bricks(K)
    out = np.zeros((n, 3))
    for d in range(3):
        lo, hi = brick_lo(cell[d], nb[d], K[d]), brick_lo(cell[d] + 1, nb[d], K[d])
        base = rng.integers(lo, hi - 5, n)
        out[:, d] = base + 2 + rng.uniform(0.05, 0.95, n)
    return out


def _special(K, rng):
    """mesh coordinates at the edges of the stencil rule"""
    nb = make_bricks(K)
    Kv = np.array(K, dtype=np.float64)
    rows = [np.array([2.0, 3.0, 4.0]), np.array([0.0, 0.0, 0.0]),                     # on mesh points (f = 0: last weight 0)
            Kv * (1.0 - 2.0 ** -24), np.array([3.0, 4.0, 5.0]) * (1.0 - 2.0 ** -24)]       # one f32 ulp below a face / a plane
    for d in range(3):                                                                 # both sides of the seam of each axis
        for x in (0.3, Kv[d] - 0.3, 2.6, Kv[d] - 2.6):
            r = rng.uniform(3.0, Kv - 3.0)
            r[d] = x
            rows.append(r)
    corner = np.array([brick_lo(1, nb[d], K[d]) for d in range(3)], dtype=np.float64)      # stencil base = brick end - 3
    rows.append(corner - 0.5)
    mid = np.array([(brick_lo(0, nb[d], K[d]) + brick_lo(1, nb[d], K[d])) / 2.0 for d in range(3)])
    rows.append(mid + 0.45)
    return np.array(rows)


def _finish(name, K, tric, rm, Q, rng, lpol, pol_frac=0.5, precs=('double', 'single'), shift=True, U_on=None, **extra):
    K = tuple(K)
    box = make_box(K, tric)
    n = len(rm)
    frac = rm / np.array(K, dtype=np.float64)
    if shift and n >= 8:                     # atoms outside the cell, some of them 50 cells away
        sel = rng.permutation(n)[:max(2, n // 8)]
        frac[sel] += rng.integers(-2, 3, (len(sel), 3))
        frac[sel[0]] += np.array([50, -50, 50])
        frac[sel[1]] -= np.array([50, 0, -50])
    pos = frac @ box
    pol = np.zeros(n)
    Uc = np.zeros((n, 3))
    if lpol:
        pol[rng.random(n) < pol_frac] = 1.0
        pol *= rng.uniform(0.3, 1.5, n)
        Uc = rng.uniform(0.05, 0.1, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3)) * (pol > 0)[:, None]
        if U_on is not None:                 # induced dipoles on sites that are charge-only without them
            pol[U_on] = 1.0
            Uc[U_on] = rng.uniform(0.05, 0.1, (len(U_on), 3)) * rng.choice([-1.0, 1.0], (len(U_on), 3))
    c = dict(name=name, K=K, tric=bool(tric), box=box, n=n, pos=pos, Q=Q, pol=pol, thole=np.full(n, 1.0) * (pol > 0), U=Uc,
             lpol=bool(lpol), precs=tuple(precs), axis_type=np.full(n, 5, dtype=np.int32),
             axis_indices=-np.ones((n, 3), dtype=np.int32),
             pairs=np.zeros((0, 2), dtype=np.int32))
    c.update(extra)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _case_one_brick(rng):      # every axis one brick: the scan form whatever the switches; the stencil covers the x axis
    K = (6, 7, 16)
    rm = np.concatenate([_special(K, rng)[:16], rng.uniform(0, 1, (17, 3)) * np.array(K)])
    Q = _sites(rng, 33)
    _set_kind(Q, np.arange(0, 33, 3), KIND_CHARGE)
    return _finish('one_brick_n33', K, True, rm, Q, rng, True)


def _case_bricks2(rng):        # 2 x 2 x 3 bricks of 8 + 9, 9 + 9, 11 + 11 + 11; z brick 2 empty; U makes charge-only sites general
    K = (17, 18, 33)
    sp = _special(K, rng)
    body = rng.uniform(0, 1, (65 - len(sp), 3)) * np.array(K)
    rm = np.concatenate([sp, body])
    rm[:, 2] = 4.0 + np.mod(rm[:, 2], 13.0)          # stencils end at z = 19: the bricks z in [22, 33) get no entry
    Q = _sites(rng, 65)
    mono = np.arange(1, 65, 2)
    _set_kind(Q, mono, KIND_CHARGE)
    return _finish('bricks2_n65', K, False, rm, Q, rng, True, shift=True, U_on=mono[:8], empty_z=(22, 33))


CLASS_BRICKS = {(0, 0, 0): (64, 64, 64), (1, 1, 1): (63, 65, 1), (0, 1, 2): (40, 0, 0), (1, 0, 2): (0, 40, 0), (1, 1, 0): (0, 0, 40)}


def _case_classes(rng):        # class runs that end inside a 64-wide group and exactly on one; bricks of a single class
    K = (17, 18, 33)
    rms, kinds = [], []
    for cell, counts in CLASS_BRICKS.items():
        for kind, cnt in enumerate(counts):
            rms.append(_inside(rng, K, cell, cnt))
            kinds += [kind] * cnt
    rm = np.concatenate(rms)
    order = rng.permutation(len(rm))
    rm, kinds = rm[order], np.array(kinds)[order]
    Q = _sites(rng, len(rm))
    for k in (KIND_DIPOLE, KIND_CHARGE):
        _set_kind(Q, np.nonzero(kinds == k)[0], k)
    return _finish('classes', K, True, rm, Q, rng, False, shift=False, kinds=kinds)


def _mixed(rng, K, n):
    rm = rng.uniform(0, 1, (n, 3)) * np.array(K)
    Q = _sites(rng, n)
    k = rng.integers(0, 3, n)
    for kind in (KIND_DIPOLE, KIND_CHARGE):
        _set_kind(Q, np.nonzero(k == kind)[0], kind)
    return rm, Q


def _case_shift32(rng):        # 16 x 16 rows: the shift store loop of the brick form
    rm, Q = _mixed(rng, (32, 32, 32), 600)
    return _finish('shift32_n600', (32, 32, 32), False, rm, Q, rng, False)


def _case_zbrick1(rng):        # one brick along z: the scan form whatever the switches
    rm, Q = _mixed(rng, (32, 48, 16), 500)
    return _finish('zbrick1_n500', (32, 48, 16), True, rm, Q, rng, True, pol_frac=0.3)


def _touching(rng, K, cell, n):
    """n mesh coordinates whose stencil has at least one point in brick `cell`: base in [lo - 5, hi - 1] (periodic)"""
    nb = make_bricks(K)
    out = np.zeros((n, 3))
    for d in range(3):
        lo, hi = brick_lo(cell[d], nb[d], K[d]), brick_lo(cell[d] + 1, nb[d], K[d])
        base = rng.integers(lo - 5, hi, n)
        out[:, d] = np.mod(base + 2 + rng.uniform(0.05, 0.95, n), K[d])
    return out


def _case_chunk(rng):          # one brick with 2200 entries of mixed classes (two chunks of the class sort), the others sparse
    K = (33, 31, 47)
    rm_in = _touching(rng, K, (1, 0, 1), 2200)
    rm_out, Q_out = _mixed(rng, K, 200)
    rm = np.concatenate([rm_in, rm_out])
    Q = np.concatenate([_sites(rng, 2200), Q_out])
    k = rng.integers(0, 3, 2200)
    for kind in (KIND_DIPOLE, KIND_CHARGE):
        _set_kind(Q, np.nonzero(k == kind)[0], kind)
    return _finish('chunk_n2400', K, False, rm, Q, rng, False, shift=False, crowded=(1, 0, 1))


def _case_xplane(rng):         # all atoms in one x plane; 31 atoms: one partial workgroup of the gather
    K = (97, 20, 23)
    rm, Q = _mixed(rng, K, 31)
    rm[:, 0] = 40.0 + rng.uniform(0.05, 0.95, 31)
    return _finish('xplane_n31', K, True, rm, Q, rng, True, shift=False)


def _case_n1(rng):
    K = (17, 18, 33)
    return _finish('n1', K, False, np.array([[7.6, 8.4, 10.7]]), _sites(rng, 1), rng, True, pol_frac=1.0)


def _case_n32(rng):
    rm, Q = _mixed(rng, (6, 7, 16), 32)
    return _finish('n32', (6, 7, 16), False, rm, Q, rng, True)


def _case_range(rng):          # f32: five sites 1000 times the rest, in a crowded brick next to sparse ones
    K = (32, 32, 32)
    rm = np.concatenate([_inside(rng, K, (0, 0, 0), 400), _inside(rng, K, (1, 1, 1), 30), _inside(rng, K, (0, 1, 0), 30)])
    Q = _sites(rng, 460)
    big = np.arange(5)
    Q[big] *= 1000.0
    return _finish('range_f32', K, False, rm, Q, rng, False, precs=('single',), shift=False, big=big, crowded=(0, 0, 0))


def _plane_case(n):
    def build(rng):
        rm, Q = _mixed(rng, (33, 31, 47), n)
        return _finish('plane_n%d' % n, (33, 31, 47), n % 2 == 1, rm, Q, rng, True, pol_frac=0.3)
    return build


_BUILDERS = {'one_brick_n33': _case_one_brick, 'bricks2_n65': _case_bricks2, 'classes': _case_classes,
             'shift32_n600': _case_shift32, 'zbrick1_n500': _case_zbrick1, 'chunk_n2400': _case_chunk,
             'xplane_n31': _case_xplane, 'n1': _case_n1, 'n32': _case_n32, 'range_f32': _case_range,
             'plane_n3072': _plane_case(3072), 'plane_n3073': _plane_case(3073), 'plane_n8192': _plane_case(8192)}
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name](np.random.default_rng(1000 + CASES.index(name)))


class EmptyCov:
    """a covalent map without bonds, in the sparse form ADMPPmeForce accepts (a dense one of 8192 atoms is 256 MB)"""

    def __init__(self, n):
        self.shape = (n, n)
        self.indptr, self.indices, self.data = np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)

    def tocsr(self):
        return self

    def sort_indices(self):
        pass


def rounded(c, prec):
    """the inputs as the handle reads them: rounded to its type, as float64 arrays"""
    r = RT[prec]
    f = lambda a: np.asarray(a, dtype=r).astype(np.float64)      # noqa: E731
    return dict(pos=f(c['pos']), Q=f(c['Q']), U=f(c['U']) if c['lpol'] else None)


def phi_noise(c, prec):
    """white noise with the same modulus in every bin (tests/test_gpu_mesh_convolve.py), rounded to the type"""
    return noise(c['K'], 77, PREC_BYTES[prec]).astype(np.float64)


def phi_wave(c, prec):
    """one plane wave: the energy word sees a smooth phi"""
    K = c['K']
    return wave(K, (1, 2 % max(1, K[1] // 2), 1), PREC_BYTES[prec]).astype(np.float64)


# ---- reference and bars of the spread ---------------------------------------------------------------------------------------------
class SpreadRef:
    """mesh, W, t and the quanta of one case and type"""

    def __init__(self, c, prec, want_parts=False):
        K = c['K']
        x = rounded(c, prec)
        g = Geom(c['box'], K)
        self.c, self.prec, self.K, self.g = c, prec, K, g
        Qt = qtot(x['Q'].astype(LD), None if x['U'] is None else x['U'].astype(LD))
        self.Qt = Qt
        base, W, X, rm = g.stencil(x['pos'])
        self.base, self.Wt, self.X, self.rm = base, W, X, rm
        self.idx = point_index(base, K)
        coef = fold(g, Qt.astype(LD))
        self.coef = coef
        self.vals = point_values(coef, W)
        self.mesh = scatter(self.idx, self.vals, K)
        Qabs = np.abs(x['Q'])
        if x['U'] is not None:
            Qabs = qtot(Qabs, np.abs(x['U']))
        self.cabs = fold_abs(g, Qabs)
        W64 = [[np.asarray(w, dtype=np.float64) for w in Wd] for Wd in W]
        self.W64 = W64
        wv = point_values(self.cabs, W64, absw=True)
        for d in range(3):
            wv = wv + X[:, d, None, None, None].astype(np.float64) * point_values(self.cabs, W64, bump=d, absw=True)
        self.wvals = wv
        self.W = scatter(self.idx, wv, K)
        # A kernel whose rounded coordinate falls on the other side of a mesh point starts its stencil one point earlier or later:
        # the point it gains carries at most sum |coef| delta^3 / 6 (the spline is C^4: M'' near the end of its support is
        # delta^3 / 6, the lower orders are smaller still), delta <= 8 u X.  That floor goes on the widened stencil's shell.
        p8 = np.arange(-1, 7)
        ix8 = [(base[:, d, None] + p8[None, :]) % K[d] for d in range(3)]
        idx8 = (ix8[0][:, :, None, None] * K[1] + ix8[1][:, None, :, None]) * K[2] + ix8[2][:, None, None, :]
        core = (p8 >= 0) & (p8 <= 5)
        shell = ~(core[:, None, None] & core[None, :, None] & core[None, None, :])
        delta = 8.0 * U[prec] * X.astype(np.float64).max(axis=1)
        floor = self.cabs.sum(axis=1) * delta ** 3 / (6.0 * U[prec])
        self.W = self.W + scatter(idx8[:, shell], np.repeat(floor[:, None], int(shell.sum()), axis=1), K)
        self.t = scatter(self.idx, np.ones(self.idx.shape), K)
        # words that no stencil can reach, whichever side of a mesh point the kernel's rounding puts an atom: stencils widened
        wide = np.zeros(K, dtype=bool)
        p = np.arange(-1, 7)
        ix = [(base[:, d, None] + p[None, :]) % K[d] for d in range(3)]
        for i in range(len(base)):
            wide[np.ix_(ix[0][i], ix[1][i], ix[2][i])] = True
        self.unreached = ~wide
        # bricks: entries, kinds, quanta
        self.kinds = site_kinds(Qt)
        self.ent_atom, self.ent_cell = brick_entries(base, K)
        nb = make_bricks(K)
        ncell = nb[0] * nb[1] * nb[2]
        self.cnt = np.bincount(self.ent_cell, minlength=ncell)
        A = np.abs(np.asarray(g.Aop, dtype=np.float64))
        amax = max(A.sum(0).max(), A.sum(1).max())
        Q64 = np.asarray(Qt, dtype=np.float64)
        q0, d1, q2 = np.abs(Q64[:, 0]), np.abs(Q64[:, 1:4]).sum(1), np.abs(Q64[:, 4:9]).sum(1)
        b32 = 0.55 ** 3 * q0 + 0.46004 * 0.55 ** 2 * amax * d1 + 0.55 ** 2 * 2 * amax ** 2 * q2
        b64 = q0 + amax * d1 + 2 * amax ** 2 * q2
        bm32, bm64 = np.zeros(ncell), np.zeros(ncell)
        np.maximum.at(bm32, self.ent_cell, b32[self.ent_atom])
        np.maximum.at(bm64, self.ent_cell, b64[self.ent_atom])
        cnt = np.maximum(self.cnt, 1)
        q32 = 2.0 ** -29 * bm32 * cnt * 1.001
        q64 = np.maximum(np.maximum(2.0 ** -58 * bm64 * cnt, 2.0 ** -49 * bm64), 2.0 ** -60 * (bm64 > 0)) * 1.001
        wb = word_bricks(K)
        self.quantum = (q32 if prec == 'single' else q64)[wb]
        self.quantum_scan = q64[wb]      # the scan form's tile is 64-bit at both precisions, under the f64 rule

    def bar(self, form, C=None):
        """per-word bar of a form ('scan', 'planes', 'bricks', 'plane_kernel' -- the last for the mesh BEFORE the convolution)"""
        u = U[self.prec]
        C = DEVICE_FACTOR * C_HOST[self.prec] if C is None else C
        b = C * u * self.W
        if form == 'bricks':
            b = b + 0.5 * self.quantum * self.t
        if form == 'scan':
            b = b + 0.5 * self.quantum_scan * self.t
        return b


def mutant_ratios(r, form, C=None):
    """smallest over the atoms of: the largest |change| / bar over the words, for each kind of mutation applied where it shows
    most for that atom.  dict kind -> (per-atom ratios)"""
    bar = r.bar(form, C).reshape(-1)
    bar_at = bar[r.idx]
    vals = np.abs(np.asarray(r.vals, dtype=np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bar_at > 0, vals / bar_at, np.where(vals > 0, np.inf, 0.0))
    out = {'column': ratio.max(axis=3).max(axis=(1, 2)), 'xplane': ratio.max(axis=(2, 3)).max(axis=1)}
    # (atom, brick) entry: the points of the atom inside one brick
    wb = word_bricks(r.K).reshape(-1)[r.idx]
    ent = np.zeros(r.c['n'])
    for i in range(r.c['n']):
        cells = np.unique(wb[i])
        ent[i] = max(ratio[i][wb[i] == cl].max() for cl in cells)
    out['entry'] = ent
    # a lower class: a general site loses its quadrupole, a dipole-only site its dipole
    lost = np.zeros_like(vals)
    noquad = np.abs(np.asarray(r.Qt[:, 4:9], dtype=np.float64)).sum(1) == 0      # (charge + dipole: the dipole is what it can lose)
    gen, dip = (r.kinds == KIND_GENERAL) & ~noquad, (r.kinds == KIND_DIPOLE) | ((r.kinds == KIND_GENERAL) & noquad)
    if gen.any():
        lost[gen] = np.abs(np.asarray(point_values(r.coef[gen], [[w[gen] for w in Wd] for Wd in r.Wt], terms=T_QUAD), dtype=np.float64))
    if dip.any():
        lost[dip] = np.abs(np.asarray(point_values(r.coef[dip], [[w[dip] for w in Wd] for Wd in r.Wt], terms=T_DIPOLE), dtype=np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        lr = np.where(bar_at > 0, lost / bar_at, np.where(lost > 0, np.inf, 0.0))
    out['class'] = lr.max(axis=(1, 2, 3))[gen | dip]
    return out


# ---- reference and bars of the gather ----------------------------------------------------------------------------------------------
F_ORDERS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1),
            (3, 0, 0), (0, 3, 0), (0, 0, 3), (2, 1, 0), (2, 0, 1), (1, 2, 0), (0, 2, 1), (1, 0, 2), (0, 1, 2), (1, 1, 1)]
FI = {o: k for k, o in enumerate(F_ORDERS)}


def f_sums(v, W, bump=None, absw=False, drop_z=None):
    """(n, 20) sums of v (n, 6, 6, 6) with the weights of F_ORDERS; drop_z: (n,) stencil index along z left out per atom"""
    if drop_z is not None:
        v = np.array(v, copy=True)
        v[np.arange(len(v)), :, :, drop_z] = 0
    out = []
    for o in F_ORDERS:
        o = list(o)
        if bump is not None:
            o[bump] += 1
        w = [W[d][o[d]] for d in range(3)]
        if absw:
            w = [np.abs(x) for x in w]
        out.append(np.einsum('nabc,na,nb,nc->n', v, w[0], w[1], w[2]))
    return np.stack(out, axis=1)


def unfold(A, Jac, Q, coef, F, absolute=False):
    """pot (n, 9), grad (n, 3) from the F sums (spline_math.h unfold_potential); absolute: every term by magnitude"""
    sg = (lambda x: np.abs(x)) if absolute else (lambda x: x)      # noqa: E731
    s = 1.0 if absolute else -1.0
    F1 = np.stack([F[:, FI[(1, 0, 0)]], F[:, FI[(0, 1, 0)]], F[:, FI[(0, 0, 1)]]], axis=1)
    gx = F1 @ A.T
    two = lambda a, b: F[:, FI[tuple(int(a == d) + int(b == d) for d in range(3))]]      # noqa: E731
    F2 = np.stack([np.stack([two(a, b) for b in range(3)], 1) for a in range(3)], 1)
    G = np.einsum('im,nmk,jk->nij', A, F2, A)
    tr = G[:, 0, 0] + G[:, 1, 1] + G[:, 2, 2]
    r3 = np.sqrt(A.dtype.type(3))
    pot = np.stack([F[:, 0], gx[:, 2], gx[:, 0], gx[:, 1], (3 * G[:, 2, 2] + s * tr) / 6, r3 * G[:, 0, 2] / 3, r3 * G[:, 1, 2] / 3,
                    r3 * (G[:, 0, 0] + s * G[:, 1, 1]) / 6, r3 * G[:, 0, 1] / 3], axis=1)

    def three(j, t):
        o = list(TERMS[t])
        o[j] += 1
        return F[:, FI[tuple(o)]]
    fu = np.stack([sum(sg(coef[:, t]) * three(j, t) for t in range(10)) for j in range(3)], axis=1)
    grad = fu @ Jac.T
    return pot, grad


class GatherRef:
    """pot, grad, fld, E and their bars for one case, type and phi"""

    def __init__(self, sr, phi):
        c, g, K = sr.c, sr.g, sr.K
        self.sr = sr
        phi = np.asarray(phi, dtype=np.float64)
        v = phi.reshape(-1)[sr.idx]
        self.v = v
        F = f_sums(v.astype(LD), sr.Wt)
        self.pot, self.grad = unfold(g.Aop, g.Jac, None, sr.coef, F)
        self.pot = np.asarray(self.pot, dtype=np.float64)
        self.grad = np.asarray(self.grad, dtype=np.float64)
        self.fld = self.pot[:, [2, 3, 1]]
        self.E = 0.5 * float((sr.Qt * self.pot.astype(LD)).sum())
        Fa = f_sums(np.abs(v), sr.W64, absw=True)
        for d in range(3):
            Fa = Fa + sr.X[:, d, None].astype(np.float64) * f_sums(np.abs(v), sr.W64, bump=d, absw=True)
        A = np.abs(np.asarray(g.Aop, dtype=np.float64))
        J = np.abs(np.asarray(g.Jac, dtype=np.float64))
        self.pot_abs, self.grad_abs = unfold(A, J, None, sr.cabs, Fa, absolute=True)
        self.Qabs = np.abs(np.asarray(sr.Qt, dtype=np.float64))

    def bars(self, C=None):
        u = U[self.sr.prec]
        C = DEVICE_FACTOR * C_HOST[self.sr.prec] if C is None else C
        bp, bg = C * u * self.pot_abs, C * u * self.grad_abs
        bE = 0.5 * float((self.Qabs * bp).sum()) + self.sr.c['n'] * 2.0 ** -53 * abs(self.E)
        return dict(pot=bp, grad=bg, fld=bp[:, [2, 3, 1]], E=bE)

    def zcol_mutant_ratio(self, C=None):
        """one lane's z column dropped, for every atom the lane that shows most: per-atom largest |change| / bar over the outputs"""
        b = self.bars(C)
        n = self.sr.c['n']
        best = np.zeros(n)
        for lane in range(6):
            Fm = f_sums(self.v.astype(LD), self.sr.Wt, drop_z=np.full(n, lane))
            pot, grad = unfold(self.sr.g.Aop, self.sr.g.Jac, None, self.sr.coef, Fm)
            with np.errstate(divide='ignore', invalid='ignore'):
                rp = np.abs(np.asarray(pot, dtype=np.float64) - self.pot) / b['pot']
                rg = np.abs(np.asarray(grad, dtype=np.float64) - self.grad) / b['grad']
            rp[~np.isfinite(rp)] = 0.0
            rg[~np.isfinite(rg)] = 0.0
            best = np.maximum(best, np.maximum(rp.max(1), rg.max(1)))
        return best


@functools.lru_cache(maxsize=None)
def spread_ref(name, prec):
    return SpreadRef(case(name), prec)


@functools.lru_cache(maxsize=None)
def gather_ref(name, prec, kind='noise'):
    c = case(name)
    return GatherRef(spread_ref(name, prec), phi_noise(c, prec) if kind == 'noise' else phi_wave(c, prec))


def convolved(sr):
    """phi of which = 1: N ifftn(G fftn(mesh_ref)) with the handle's G at the flat kappa of the mesh, the word bound B_word of
    tests/test_gpu_mesh_convolve.py for the convolution, and what the spread's own bar becomes behind it (an error e of the
    mesh reaches a word of phi as at most sumG |e|_1)"""
    from tests.test_gpu_mesh_convolve import Reference
    c = sr.c
    box = np.array(c['box'])
    kappa = flat_kappa(box, c['K'], 1)
    G = half_spectrum_table(g_table(box, c['K'], kappa, 1))
    mesh = np.asarray(sr.mesh, dtype=np.float64)
    ref = Reference(mesh, G, PREC_BYTES[sr.prec], per_bin=False)
    return dict(kappa=kappa, G=G, phi=ref.ref, B_word=ref.B_word, sumG=float(G.sum()))
