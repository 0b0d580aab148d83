"""The k-space leg  mesh <- IFFT(G * FFT(mesh))  and its energy word, bin by bin, on every transform path of
MeshConv::convolve (admp_mesh_convolve) against numpy.fft in float64 with G built from the oracle alone.

Why: the end-to-end tests run at the production Ewald parameters, where G spans 55 decades and 80-99 % of the bins lie below
their tolerances.  Here the same meshes also run at a FLAT kappa, chosen per mesh from the oracle's table so that
max G / min G over the non-zero bins stays below 1e5 (asserted): there every bin carries signal and a mis-routed bin shows.

Reference (float64, from the T-rounded input x):  S = fftn(x),  ref = N ifftn(G S),  E = 1/2 sum G |S|^2, with
G = 2 DIELECTRIC Ck_1 / theta_k^2 and G(0) = 0 (which = 1), G = 2 Ck_n / theta_k^2 with the gamma point (which = 6, 8, 10)
-- gfactor_at of recip_kernels.hip; in the reference's literal k-point order the table of kspace_tables(quirk=True),
reshaped onto the (K1, K2, K3) spectrum and symmetrised (G(t) + G(-t)) / 2 as k_gtab does.  The unmarked tests of this file
check this reference on the CPU against oracle.pme_recip on spread meshes.

Inputs.  "Noise": white noise with Gaussian samples, built as the inverse transform of a unit-modulus spectrum with seeded
random phases.  Ordinary Gaussian noise has Rayleigh-distributed bin moduli: of 1e6 bins some carry 1e-3 of the rms, and a
wrong bin could hide there; with |S(k)| = sqrt(N) in every bin (up to the rounding to T) none can.  "Waves": real plane
waves cos(2 pi m.n / K) at the gamma point, the Nyquist index of every even axis, (K-1)/2 of every odd axis, the corner
and one random interior bin; each must come back as N G(m) times itself.

Error model (first order in u = 2^-24 / 2^-53).  Every hand-written pass is a direct sum over one axis.  A sum of K terms
x_j w_j with |w_j| = 1 has |err| <= gamma sum_j |x_j| with gamma = (K + c) u; c collects what is not the K - 1 additions:
the twiddle (exact table entries rounded to T, carried between re-seeds every 8 steps by a recurrence: <= 64 u in f64 by
the analysis in dft_math.h TwStep, <= 8 complex products = 8 * 2 sqrt2 u < 24 u in f32), the complex product (2 sqrt2 u),
the pair sums a +- b, the closing additions and the rounding of the stored value (together < 6 u): c = 64 + 3 + 6 < 80 in
f64, c = 24 + 3 + 6 < 32 in f32.  A two-level axis N = N1 N2 is two such sums, (N1 + c) u + (N2 + c) u <= (N + 2 c) u since
N1 + N2 <= N1 N2.  One constant per type (C_AXIS = 2 c) for every axis and path:

    gamma_d = (K_d + 2 c) u = (K_d + 160) 2^-53 | (K_d + 64) 2^-24,    Gamma = gamma_x + gamma_y + gamma_z,
    g_u = u + 32 * 2^-53 (G: double arithmetic, rounded to T).

rocFFT's passes are O(log K) deep; they are held to the same bounds.  Order of the passes: z, y, x forward, x, y, z inverse.
With a = |x| summed along axes, v1 = fft_z x, v2 = fft_y v1 (so S = fft_x v2), T = G S, u2 = K1 ifft_x T, u3 = K2 ifft_y u2:

* forward.  The z pass errs by <= gamma_z sum_z|x| per word; through the exact y and x passes that becomes <= gamma_z |x|_1
  in every bin.  The y pass errs by <= gamma_y sum_y|v1|, through the x pass <= gamma_y b(kz), b(kz) = sum_{x,y} |v1|.
* x pass, line l = (ky, kz).  Either forward * G * inverse or one circulant product out_i = sum_j c[i-j] v_j with the table
  c = ifft(G_l): by the bound of test_dft_circulant_cpu.py |err_i| <= 2 gamma_x sumG_l sum_x|v2_l| (|c| <= sumG_l), which
  also covers the two-transform form (gamma_x G_k sum_x|v2| forward + gamma_x sum_kx G|S| inverse, each <= half of it).
* inverse.  The y pass errs by <= gamma_y sum_ky|u2|, the z pass by <= gamma_z sum_kz|u3| per word.

Word-wise bound (every word n):  an error e in the spectrum reaches a word as at most sum_k |e_k|, so
    |out - ref|(n) <= B_word = (Gamma + gamma_x + g_u) |x|_1 sumG + Gamma sum_k G_k |S_k|.
Energy (summed in double from T values; circulant form: sum_x Re(conj(v) out)):
    |E - E_ref| <= B_E = (Gamma + g_u) |x|_1 sum_l sumG_l sum_x|v2_l| + N 2^-53 E_ref.
Per bin, f64 (fftn(out) against N G S):  an exact forward transform of a word error e gives at most sum_n |e_n|, of an
error in the (x, ky, kz) / (x, y, kz) stage the sum over the remaining real-space axes only:
    D(k) = N G_k (gamma_z |x|_1 + gamma_y b(kz) + g_u |S_k|) + 2 N gamma_x sumG_l sum_x|v2_l|
           + K2 K3 gamma_y sum_{x,ky}|u2|(kz) + K3 gamma_z sum|u3|.
At flat kappa D(k) / (N G_k |S_k|) < 1e-3 in every bin is asserted (gamma bin of which = 1: signal 0, compared absolutely).
Per bin, f32: worst-case bounds exceed the signal (gamma N > 1); the tolerance is a model,
    tol(k) = C u sqrt(K1+K2+K3) N (G_k |S_k| + rms_k'(G |S|)),
C measured in the same run as the largest err / model of the rocFFT 3-D path (ADMP_DFT=0 ADMP_FUSED_X=0) over the mesh
list, one C for the production-kappa cases and one, smaller, for the flat-kappa ones; the hand-written paths get 8 C (an O(N^2) sum's rounding error grows as sqrt N, an FFT's as sqrt log N:
sqrt(160 / log2 160) = 4.7, rounded up to a power of two).  8 tol(k) / signal < 0.1 is asserted in every bin at flat kappa.
Waves: relative 2-norm error |out - N G(m) x|_2 / |N G(m) x|_2 (max-norm worst cases exceed 1 in f32 on 1e6 words).  A pass
errs by <= gamma_d sqrt(K_d) in relative 2-norm (Cauchy-Schwarz on the sum bound); forward errors are amplified by at
most Gmax / G(m); the x pass by line as above:
    rel2 <= (gamma_z sqrt K3 + gamma_y sqrt K2) (Gmax / G(m) + 1) + g_u
            + sqrt(K2 K3 sum_l (2 gamma_x K1 sumG_l |v2_l|_2)^2) / (N G(m) |x|_2).
The bound itself must be below 0.5 (a routing error is 100 %); waves run at flat kappa, where that holds.  The gamma wave
of which = 1 must come back as zero: |out| <= B_word.

G(k) != G(-k) only where an even axis of a triclinic cell has its Nyquist index (one signed frequency, -K/2, for the point and
its mirror point); a real mesh sees the mean of the two, the reference here uses it, and k_gtab stores it (before this test
the two-level layouts, which store other z columns than kz <= K3/2, gave those planes the other point's factor).

Every case prints its ratios, the file its C, the worst ratio per path and type and its wall time (run with -s).  Measured on
an MI355X: C = 33.2 at the production kappa (305x170x183), 2.6 at flat kappa.  Largest ratios of a run, hand-written
paths: f32 bin err / (C model) 1.21 of the 8 allowed (two-level, vector stage A, production kappa; 1.13 at flat kappa), f64
bin err / D 0.079 (direct planes), word err / B_word 1.1e-3, E err / B_E 7.2e-3, wave rel2 / bound 6.0e-5 / 0.34 (f32) and
3.1e-13 / 7.5e-10 (f64); at flat kappa D / signal <= 1.8e-7 and 8 C model / signal <= 0.0095 in every bin.  DESIGN.md has
the table per path.

Detection (two slot->frequency entries swapped on a scratch copy: 42 flat-kappa cases fail, none at production kappa, the
end-to-end tests pass): DESIGN.md, section 2.
"""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_pfa_maps_cpu import expected_split      # noqa: E402  (N1, N2) of pfa_maps.h, checked there

U = {4: 2.0 ** -24, 8: 2.0 ** -53}
RT = {4: np.float32, 8: np.float64}
C_AXIS = {4: 64, 8: 160}                  # 2 c of the module docstring
SPACING = 31.289 / 97                      # mesh spacing of water_pol_1024 (box 31.289 A, 97^3)
KAPPA_PROD = math.sqrt(-math.log(2e-4)) / 4.0      # setup_ewald_parameters(4, 1e-4): 0.7296, whatever the box
FLAT_CANDIDATES = (3.0, 4.5, 7.0, 20.0)
HAND_FACTOR = 8.0


# ---- reference -----------------------------------------------------------------------------------------------------------
try:                                       # pocketfft either way; scipy's front end runs the lines on several threads
    from scipy import fft as _fft
    _FFT_KW = dict(workers=min(16, os.cpu_count() or 1))
except ImportError:
    _fft, _FFT_KW = np.fft, {}


def fft1(a, axis):
    return _fft.fft(a, axis=axis, **_FFT_KW)


def ifft1(a, axis):
    return _fft.ifft(a, axis=axis, **_FFT_KW)


def make_box(K, tric):
    box = np.diag([k * SPACING for k in K]).astype(np.float64)
    if tric:
        box[1, 0] = 0.11 * box[0, 0]
        box[2, 0] = -0.07 * box[0, 0]
        box[2, 1] = 0.09 * box[1, 1]
    return box


def g_table(box, K, kappa, which, ref_order=False):
    """G on the (K1, K2, K3) spectrum, float64, from the oracle's tables alone."""
    import torch
    from oracle import admp_oracle as O
    ksq, theta = O.kspace_tables(torch.as_tensor(box), tuple(K), quirk=bool(ref_order))
    V = float(np.linalg.det(box))
    if which == 1:
        ck = O.Ck_1(ksq[1:], kappa, V)
        G = torch.cat([torch.zeros(1, dtype=ck.dtype), 2.0 * O.DIELECTRIC * ck / theta[1:] ** 2])
    else:
        fn = {6: O.Ck_6, 8: O.Ck_8, 10: O.Ck_10}[which]
        G = 2.0 * fn(ksq, kappa, V) / theta ** 2
    G = G.numpy().reshape(K)                 # row t of the table serves element t of the flattened spectrum
    if ref_order:                            # the half spectrum sees (G(t) + G(-t)) / 2 (k_gtab)
        G = 0.5 * (G + mirrored(G))
    return G


def mirrored(A):
    """A(-k)"""
    for ax in range(3):
        A = np.roll(np.flip(A, axis=ax), 1, axis=ax)
    return A


def half_spectrum_table(G):
    """What a real mesh sees of a table: (G(k) + G(-k)) / 2, since |S(-k)| = |S(k)| -- the oracle's full-spectrum sum is a
    sum over this.  Equal to G wherever G(k) = G(-k): every bin of an orthorhombic cell, and of a triclinic one except
    where an even axis has its Nyquist index (the oracle lists it as -K/2 only, so G(-K/2, ky, kz) != G(-K/2, -ky, -kz)
    there).  The library stores the mean in those bins (k_gtab), so that every spectrum layout computes the same."""
    return 0.5 * (G + mirrored(G))


def g_ratio(G):
    nz = G[G != 0.0]
    return float(nz.max() / nz.min())


def flat_kappa(box, K, which):
    """the candidate with the flattest table"""
    best = None
    for kap in (FLAT_CANDIDATES if np.prod(K) < 2e6 else FLAT_CANDIDATES[1:3]):      # (a table of the 305 x 170 x 183 mesh takes 5 s)
        r = g_ratio(g_table(box, K, kap, which))
        if best is None or r < best[1]:
            best = (kap, r)
    return best[0]


_NOISE_CACHE = {}


def noise(K, seed, prec):
    key = (tuple(K), seed)
    if key not in _NOISE_CACHE:              # one array per mesh serves every table, kappa, cell and type of a process
        rng = np.random.default_rng(seed)
        ang = np.angle(_fftn(rng.standard_normal(tuple(K))))        # phases of a real array's spectrum: odd in k
        _NOISE_CACHE[key] = _fft.ifftn(np.exp(1j * ang), **_FFT_KW).real * math.sqrt(float(np.prod(K)))
    return np.ascontiguousarray(_NOISE_CACHE[key].astype(RT[prec]))


def wave_bins(K, seed):
    rng = np.random.default_rng(seed)
    edge = [k // 2 if k % 2 == 0 else (k - 1) // 2 for k in K]
    ms = [(0, 0, 0)]
    for d in range(3):
        m = [0, 0, 0]
        m[d] = edge[d]
        ms.append(tuple(m))
    ms.append(tuple(edge))
    ms.append(tuple(int(rng.integers(1, max(2, e))) if e > 1 else e for e in edge))
    out = []
    for m in ms:
        if m not in out:
            out.append(m)
    return out


def wave(K, m, prec):
    n = np.meshgrid(*[np.arange(k) for k in K], indexing='ij')
    ph = sum(m[d] * n[d] / K[d] for d in range(3))
    return np.ascontiguousarray(np.cos(2.0 * np.pi * ph).astype(RT[prec]))


def gammas(K, prec):
    return [(k + C_AXIS[prec]) * U[prec] for k in K]


class Reference:
    """float64 reference of one (input, G, type) with every bound of the module docstring"""

    def __init__(self, x, G, prec, per_bin=True):
        K = x.shape
        N = float(x.size)
        u = U[prec]
        gx, gy, gz = gammas(K, prec)
        Gam = gx + gy + gz
        gu = u + 32 * 2.0 ** -53
        x = x.astype(np.float64)
        self.K, self.N, self.G, self.prec = K, N, G, prec
        x1 = float(np.abs(x).sum())
        self.az2 = float(np.sqrt((np.abs(x).sum(axis=2) ** 2).sum()))        # |a_z|_2, a_z = sum_z |x|
        v1 = fft1(x, 2)
        b = np.abs(v1).sum(axis=(0, 1))
        self.q = np.sqrt((np.abs(v1).sum(axis=1) ** 2).sum(axis=0))          # q(kz) = |sum_y |v1(., y, kz)||_2 over x
        v2 = fft1(v1, 1)
        del v1
        vabs1 = np.abs(v2).sum(axis=0)
        self.v2norm = np.sqrt((np.abs(v2) ** 2).sum(axis=0))
        S = fft1(v2, 0)
        del v2
        self.S = S
        self.sumG_l = G.sum(axis=0)
        sumG = float(G.sum())
        aS = np.abs(S)
        GS = G * aS
        self.E = 0.5 * float((GS * aS).sum())
        self.x1, self.x2 = x1, float(np.sqrt((x * x).sum()))
        self.B_word = (Gam + gx + gu) * x1 * sumG + Gam * float(GS.sum())
        lines = float((self.sumG_l * vabs1).sum())
        self.B_E = (Gam + gu) * x1 * lines + N * 2.0 ** -53 * self.E
        u2 = ifft1(G * S, 0) * K[0]
        c2 = np.abs(u2).sum(axis=(0, 1))
        u3 = ifft1(u2, 1) * K[1]
        del u2
        s3 = float(np.abs(u3).sum())
        self.ref = (ifft1(u3, 2) * K[2]).real
        del u3
        if per_bin:
            self.signal = N * GS
            self.D = (N * G * (gz * x1 + gy * b[None, None, :] + gu * aS) + (2.0 * N * gx) * (self.sumG_l * vabs1)[None, :, :]
                      + (K[1] * K[2] * gy) * c2[None, None, :] + K[2] * gz * s3)
            self.model = u * math.sqrt(sum(K)) * N * (GS + math.sqrt(float((GS * GS).mean())))

    def wave_bound(self, m):
        """relative 2-norm bound of the plane wave at bin m (rigorous, first order)"""
        K, N, G = self.K, self.N, self.G
        gx, gy, gz = gammas(K, self.prec)
        gu = U[self.prec] + 32 * 2.0 ** -53
        Gm = float(G[m])
        ref2 = N * Gm * self.x2
        Gz = G.max(axis=(0, 1))
        Gx = G.max(axis=0)
        fz = math.sqrt(N) * gz * math.sqrt(K[0] * K[1]) * self.az2 * math.sqrt(float((Gz ** 2).sum())) / ref2
        fy = math.sqrt(N) * gy * math.sqrt(K[0]) * math.sqrt(float(((Gx * self.q[None, :]) ** 2).sum())) / ref2
        xterm = math.sqrt(K[1] * K[2] * float(((2.0 * gx * K[0] * self.sumG_l * self.v2norm) ** 2).sum())) / ref2
        return fz + fy + xterm + gu + gy * math.sqrt(K[1]) + gz * math.sqrt(K[2])


# ---- CPU: the reference against the oracle ---------------------------------------------------------------------------------
def _spread_case(K, lmax, seed, tric=False):
    import torch
    from oracle import admp_oracle as O
    rng = np.random.default_rng(seed)
    box = make_box(K, tric) * 3.0            # a box a few molecules wide
    na = 24
    pos = rng.random((na, 3)) @ box
    Q = rng.standard_normal((na, 9))
    if lmax == 0:
        Q[:, 1:] = 0.0
    mesh = O.spread_Q(torch.as_tensor(pos), torch.as_tensor(box), torch.as_tensor(Q), list(K), lmax).numpy()
    return box, pos, Q, mesh


@pytest.mark.parametrize('K,tric', [((12, 12, 12), False), ((10, 12, 14), False), ((10, 12, 14), True)])
def test_reference_energy_equals_oracle_pme_recip(K, tric):
    import torch
    from oracle import admp_oracle as O
    box, pos, Q, mesh = _spread_case(K, 2, 11 + sum(K), tric)
    kappa = 0.4
    tb, tp, tq = torch.as_tensor(box), torch.as_tensor(pos), torch.as_tensor(Q)
    for ref_order in (False, True):
        want = float(O.pme_recip(tp, tb, tq, kappa, list(K), 2, quirk=ref_order))
        got = Reference(mesh, g_table(box, K, kappa, 1, ref_order), 8, per_bin=False).E
        print('K=%s tric=%d ref_order=%d  E %.12e  oracle %.12e' % (K, tric, ref_order, got, want))
        assert abs(got - want) <= 1e-12 * abs(want)
    # dispersion tables: gamma point kept
    box, pos, Q, mesh = _spread_case(K, 0, 5 + sum(K), tric)
    tp, tq = torch.as_tensor(pos), torch.as_tensor(Q)
    for which, fn in ((6, O.Ck_6), (8, O.Ck_8), (10, O.Ck_10)):
        want = float(O.pme_recip(tp, tb, tq, kappa, list(K), 0, Ck_fn=fn, gamma=True, quirk=False))
        got = Reference(mesh, g_table(box, K, kappa, which), 8, per_bin=False).E
        print('K=%s tric=%d which=%d  E %.12e  oracle %.12e' % (K, tric, which, got, want))
        assert abs(got - want) <= 1e-12 * abs(want)


def test_reference_is_consistent_and_inputs_are_white():
    K = (10, 12, 9)
    box = make_box(K, True)
    G = g_table(box, K, 3.0, 1)
    # the half-spectrum form: even under k -> -k (a real mesh needs it), gamma point zero, positive elsewhere; equal to the
    # oracle's table except on the Nyquist planes of the even x and y axes of this triclinic cell
    Gh = half_spectrum_table(G)
    assert np.array_equal(Gh, mirrored(Gh))
    diff = Gh != G
    assert diff.any() and not diff[np.ix_(np.arange(10) != 5, np.arange(12) != 6, np.arange(9))].any()
    Go = g_table(make_box(K, False), K, 3.0, 1)
    assert np.array_equal(half_spectrum_table(Go), Go)
    for w in (6, 8, 10):
        Gw = g_table(make_box(K, False), K, 3.0, w)
        assert (Gw > 0).all() and np.array_equal(half_spectrum_table(Gw), Gw)
    G = Gh
    assert G[0, 0, 0] == 0.0 and (G.reshape(-1)[1:] > 0).all()
    x = noise(K, 3, 8)
    S = np.abs(np.fft.fftn(x))
    assert np.abs(S / math.sqrt(x.size) - 1.0).max() < 1e-9           # every bin carries the same signal
    r = Reference(x, G, 8)
    assert np.abs(r.ref - np.fft.ifftn(G * np.fft.fftn(x)).real * x.size).max() <= 1e-12 * np.abs(r.ref).max()
    # a plane wave is an eigenvector: N G(m) times itself, and the bounds are positive
    for m in wave_bins(K, 1):
        w = wave(K, m, 8)
        rw = Reference(w, G, 8, per_bin=False)
        assert np.abs(rw.ref - x.size * G[m] * w).max() <= 1e-12 * x.size * G.max()
        if G[m] > 0:
            assert 0.0 < rw.wave_bound(m) < 1e-9
    assert (r.D > 0).all() and r.B_word > 0 and r.B_E > 0


# ---- GPU: every path ---------------------------------------------------------------------------------------------------------
DIRECT_MESHES = [(31, 34, 38), (97, 64, 100), (64, 100, 97), (2, 3, 160), (160, 2, 3), (3, 160, 2)]
FUSED_MESHES = [(32, 33, 36), (64, 36, 35), (128, 45, 40)]
# two-level: (long, short, short) triples in their three rotations, so that every length meets the x, y and z kernels.
#   314 = 2 * 157 (H = 78)   393 = 3 * 131 (65)   508 = 4 * 127 (63)   222 = 6 * 37 (18)   248 = 8 * 31 (15)
#   24 = 8 * 3 (1)   30 = 6 * 5 (2)   96 = 32 * 3   119 = 7 * 17   153 = 9 * 17   170 = 10 * 17   6 = 2 * 3   10 = 2 * 5
#   7 and 9 stay whole (prime powers): mixed plain and split axes
#   The matrix-core stage A needs an odd N2 and 8 columns (16 z lines) in the LDS budget: N <= 463 in f32, N <= 235 in f64
#   (mfma_xy below).  508 is too long for it in either type and 248, 314, 393 in f64, so the shortest lengths with the same
#   N2 run too (35 = 5 * 7 gives every process an N1 = 5):   254 = 2 * 127 (H = 63, four tiles, one row short of the tile edge; f32)   122 = 2 * 61 (30)   62 = 2 * 31 (15)
PFA_TRIPLES = [(314, 24, 30), (393, 96, 7), (508, 119, 6), (222, 153, 10), (248, 170, 9), (254, 35, 7), (122, 62, 9)]
LISTED_N2 = (3, 5, 31, 37, 61, 127, 131, 157)      # H = 1, 2, 15, 18, 30, 63, 65, 78
PFA_MESHES = [r for t in PFA_TRIPLES for r in (t, (t[2], t[0], t[1]), (t[1], t[2], t[0]))]
BIG = (305, 170, 183)                      # setup_ewald_parameters' mesh of the 98 304-atom water box: 5 * 61, 10 * 17, 3 * 61
QUIRK_MESH = (31, 34, 38)

PATHS = ('rocfft', 'fused_x', 'direct_lines', 'direct_planes', 'two_level')

PROCESSES = [
    # name, switches, meshes (K, options)
    ('rocfft', {'ADMP_DFT': '0', 'ADMP_FUSED_X': '0'}),
    ('default', {}),
    ('direct', {'ADMP_DFT': '1'}),
    ('direct_separate', {'ADMP_DFT': '1', 'ADMP_DFT_PLANES': '0', 'ADMP_DFT_XCIRC': '0'}),
    ('two_level', {'ADMP_DFT': '2', 'ADMP_PFA_MIN': '0'}),
    ('two_level_vector', {'ADMP_DFT': '2', 'ADMP_PFA_MIN': '0', 'ADMP_PFA_MFMA': '0'}),
    ('two_level_small_lds', {'ADMP_DFT': '2', 'ADMP_PFA_MIN': '0', 'ADMP_PFA_LDS_KB': '16'}),
    # 16 KB brings f64 down to one column and one z line, f32 only to two z lines; 8 KB on the longest length does the rest
    ('two_level_lds8', {'ADMP_DFT': '2', 'ADMP_PFA_MIN': '0', 'ADMP_PFA_LDS_KB': '8'}),
]
LDS_KB = {name: int(sw.get('ADMP_PFA_LDS_KB', 60)) for name, sw in PROCESSES}


def mfma_xy(N1, N2, prec, lds_kb=60):
    """(columns per workgroup, matrix-core stage A) of an x or y axis: pfa_cols and pfa_use_mfma of pfa_kernels.hip"""
    N, nc = N1 * N2, 8
    while nc > 1 and 2 * prec * (N2 + N1 + 2 * N * nc) + 4 * N > lds_kb * 1024:
        nc //= 2
    return nc, int(nc == 8 and N2 % 2 == 1 and (N2 - 1) // 2 <= 128)


def mesh_plan(proc):
    """[(K, dict(tric=.., waves=.., tables=.., quirk=.., big=..))] of one process"""
    def opt(tric=True, waves=True, tables=False, quirk=False, big=False):
        return dict(tric=tric, waves=waves, tables=tables, quirk=quirk, big=big)
    small_direct = [(K, opt(tables=(K == QUIRK_MESH), quirk=(K == QUIRK_MESH))) for K in DIRECT_MESHES]
    fused = [(K, opt()) for K in FUSED_MESHES]
    # triclinic on one rotation per triple, another one from triple to triple: the long axis meets it on x, y and z
    pfa = [(K, opt(tric=(i % 3 == (i // 3) % 3), tables=(i == 0))) for i, K in enumerate(PFA_MESHES)]
    pfa.append((QUIRK_MESH, opt(tric=False, waves=False, quirk=True)))
    big = [(BIG, opt(tric=False, waves=False, big=True))]
    def quiet(rows):
        # noise only.  The waves probe routing, which the rocFFT path does not have and which the vector and small-LDS
        # processes share with two_level (same maps and tables); they are left out there, and on 305 x 170 x 183 in f64
        # (cases_of), for the time they take, not for their bound
        return [(K, dict(o, waves=False)) for K, o in rows]
    if proc == 'rocfft':                     # the calibration of C: every mesh of the other processes, noise
        return quiet(small_direct + fused + pfa[:-1] + big)
    if proc == 'default':
        return fused + big
    if proc == 'direct':
        return small_direct
    if proc == 'direct_separate':
        return [(K, dict(o, tables=False)) for K, o in small_direct]
    if proc == 'two_level':
        return pfa + [(BIG, opt(tric=False, waves=True, big=True))]
    if proc == 'two_level_vector':
        return quiet(pfa + big)
    if proc == 'two_level_lds8':
        return quiet([(K, dict(o, tric=False)) for K, o in pfa if 508 in K])
    return quiet(pfa)


_KAPPA_CACHE = {}


def kappa_flat(K, tric, which):
    key = (tuple(K), tric, which)
    if key not in _KAPPA_CACHE:
        _KAPPA_CACHE[key] = flat_kappa(make_box(K, tric), K, which)
    return _KAPPA_CACHE[key]


def cases_of(proc):
    out = []
    for K, o in mesh_plan(proc):
        for prec in (4, 8):
            for tric in ((False, True) if o['tric'] else (False,)):
                tag = '%dx%dx%d_%s_f%d' % (K + ('tric' if tric else 'ortho', 8 * prec))
                base = dict(K=list(K), tric=tric, prec=prec, ref_order=0, dev=0)
                for which in ((1, 6, 8, 10) if (o['tables'] and not tric) else (1,)):
                    for kind in ('prod', 'flat'):
                        kap = KAPPA_PROD if kind == 'prod' else kappa_flat(K, tric, which)
                        out.append(dict(base, id='%s_w%d_%s_noise' % (tag, which, kind), which=which, kappa=kap, kind=kind,
                                        input=dict(kind='noise', seed=1000 + sum(K))))
                if o['waves'] and not (o['big'] and prec == 8):
                    ms = wave_bins(K, 7)
                    if o['big']:
                        ms = [ms[0], ms[1], ms[4]]           # gamma, the x edge, the corner
                    for which in (1,):
                        kap = kappa_flat(K, tric, which)
                        for m in ms:
                            out.append(dict(base, id='%s_w%d_flat_wave_%d_%d_%d' % ((tag, which) + m), which=which, kappa=kap,
                                            kind='flat', input=dict(kind='wave', m=list(m))))
                if o['quirk'] and not tric:
                    for kind in ('prod', 'flat'):
                        kap = KAPPA_PROD if kind == 'prod' else kappa_flat(K, tric, 1)
                        out.append(dict(base, id='%s_w1_%s_noise_reforder' % (tag, kind), which=1, kappa=kap, kind=kind,
                                        ref_order=1, input=dict(kind='noise', seed=1000 + sum(K))))
    out[0]['dev'] = 1                        # one case per process on a device pointer
    return out


def make_input(case):
    K = tuple(case['K'])
    if case['input']['kind'] == 'noise':
        return noise(K, case['input']['seed'], case['prec'])
    return wave(K, tuple(case['input']['m']), case['prec'])


def child_main(cases_path, outdir):
    import ctypes
    import torch                             # before the library, as everywhere else: one HIP runtime per process, torch's
    torch.cuda.init()
    from admp_amd import _lib
    L = _lib.load()
    cases = json.load(open(cases_path))
    handles, results = {}, {}
    for c in cases:
        K, prec = tuple(c['K']), c['prec']
        if (K, prec) not in handles:
            h = ctypes.c_void_p()
            rc = L.admp_create(ctypes.byref(h), 0, prec)
            assert rc == 0, 'admp_create %d' % rc
            handles[(K, prec)] = h
        h = handles[(K, prec)]
        _lib.check(h, L.admp_set_ewald(h, float(c['kappa']), K[0], K[1], K[2], 2, 0), 'admp_set_ewald')
        _lib.check(h, L.admp_set_option(h, _lib.OPT_REFERENCE_KPOINTS, int(c['ref_order'])), 'admp_set_option')
        x = make_input(c)
        box = _lib.darr(make_box(K, c['tric']))
        E = ctypes.c_double(0.0)
        info = (ctypes.c_int * _lib.MESH_INFO_WORDS)()
        if c['dev']:
            t = torch.from_numpy(x).cuda()
            torch.cuda.synchronize()
            _lib.check(h, L.admp_mesh_convolve(h, box, c['which'], ctypes.c_void_p(t.data_ptr()), 1, ctypes.byref(E), info),
                       'admp_mesh_convolve')
            out = t.cpu().numpy()
        else:
            out = x.copy()
            _lib.check(h, L.admp_mesh_convolve(h, box, c['which'], out.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(E), info),
                       'admp_mesh_convolve')
        np.save(os.path.join(outdir, c['id'] + '.npy'), out)
        results[c['id']] = dict(E=E.value, info=list(info))
    json.dump(results, open(os.path.join(outdir, 'results.json'), 'w'))
    print('MESH-CHILD-OK %d cases' % len(cases))


def _fftn(a):
    return _fft.fftn(a, **_FFT_KW)


def ref_key(c):
    return (tuple(c['K']), c['tric'], c['kappa'], c['which'], c['ref_order'], c['prec'], json.dumps(c['input'], sort_keys=True))


def check_case(c, r, out, E):
    """bounds that need no calibration are asserted here; returns the figures of the case"""
    K = tuple(c['K'])
    fig = {}
    noise_in = c['input']['kind'] == 'noise'
    lo = 1 if c['which'] == 1 else 0         # the gamma bin of which = 1 carries no signal: compared absolutely only
    out = out.astype(np.float64)
    if not noise_in:
        m = tuple(c['input']['m'])
        Gm = float(r.G[m])
        if Gm == 0.0:
            fig['wave_abs/B_word'] = float(np.abs(out).max() / r.B_word)
            assert fig['wave_abs/B_word'] <= 1.0, (c['id'], fig)
        else:
            bound = r.wave_bound(m)
            rel = float(np.sqrt(((out - r.ref) ** 2).sum()) / np.sqrt((r.ref ** 2).sum()))
            fig['wave_rel2'], fig['wave_bound'] = rel, bound
            assert bound < 0.5, (c['id'], fig)
            assert rel <= bound, (c['id'], fig)
    fig['word/B_word'] = float(np.abs(out - r.ref).max() / r.B_word)
    fig['E/B_E'] = abs(E - r.E) / r.B_E
    assert fig['word/B_word'] <= 1.0 and fig['E/B_E'] <= 1.0, (c['id'], fig)
    if noise_in:
        err = np.abs(_fftn(out) - r.N * r.G * r.S)
        if c['prec'] == 8:
            fig['bin/D'] = float((err / r.D).max())
            kbad = np.unravel_index(int(np.argmax(err / r.D)), K)
            assert fig['bin/D'] <= 1.0, (c['id'], fig, 'worst bin', kbad)
            if c['kind'] == 'flat':
                fig['D/signal'] = float((r.D.reshape(-1)[lo:] / r.signal.reshape(-1)[lo:]).max())
                assert fig['D/signal'] < 1e-3, (c['id'], fig)
        else:
            q = err / r.model
            fig['bin/model'] = float(q.max())
            fig['worst_bin'] = [int(v) for v in np.unravel_index(int(np.argmax(q)), K)]
            if c['kind'] == 'flat':
                fig['model/signal'] = float((r.model.reshape(-1)[lo:] / r.signal.reshape(-1)[lo:]).max())
    return fig


def expected_info(proc, c, info):
    """which form must have run"""
    K = tuple(c['K'])
    path = PATHS[info[0]]
    if proc == 'rocfft':
        assert path == 'rocfft', (c['id'], path)
    elif proc == 'default':
        assert path == ('two_level' if K == BIG else 'fused_x'), (c['id'], path)
        if K == BIG:
            assert [tuple(info[2:5]), tuple(info[5:8])] == [(5, 10, 3), (61, 17, 61)], (c['id'], info)
    elif proc == 'direct':
        assert path in ('direct_planes', 'direct_lines'), (c['id'], path)
        if c['which'] == 1 and not c['ref_order']:
            # circulant iff the table is even along x: an orthorhombic cell, or K1 = 2, where -kx is kx
            assert info[1] == (2 if c['tric'] and K[0] > 2 else 1), (c['id'], info)
        else:
            assert info[1] == 2 or c['ref_order'], (c['id'], info)           # the circulant table belongs to Ck_1
    elif proc == 'direct_separate':
        assert path == 'direct_lines' and info[1] == 2, (c['id'], info)
    else:
        assert path == 'two_level', (c['id'], path)
        for d in range(3):
            assert (info[2 + d], info[5 + d]) == expected_split(K[d], 0), (c['id'], d, info)
        for d in range(2):                   # columns per workgroup and stage A of the split x and y axes
            if info[2 + d] > 1:
                nc, mf = mfma_xy(info[2 + d], info[5 + d], c['prec'], LDS_KB[proc])
                assert (info[8 + d], info[12 + d]) == (nc, mf if proc != 'two_level_vector' else 0), (c['id'], d, info)
        if proc == 'two_level_vector':
            assert info[12] == 0 and info[13] == 0 and info[14] == 0, (c['id'], info)
        if proc == 'two_level' and K == BIG:
            # the form of the 98 304-atom configuration: f32 holds 8 columns (MFMA stage A, H = 30 in two tiles), f64 only 4
            assert (info[8], info[12]) == ((8, 1) if c['prec'] == 4 else (4, 0)), (c['id'], info)


def coverage(proc, infos):
    """the forms the info arrays of one process must show at least once, in both types where the type allows it"""
    for prec in (4, 8):
        rows = [(c, i) for c, i in infos if c['prec'] == prec]
        paths = {PATHS[i[0]] for c, i in rows}
        if proc == 'direct':
            assert {(PATHS[i[0]], i[1]) for c, i in rows} >= {('direct_planes', 1), ('direct_planes', 2), ('direct_lines', 1),
                                                             ('direct_lines', 2)}, (prec, paths)
        if proc == 'two_level_lds8':
            if prec == 4:                    # what 16 KB leaves to f32: one column, one z line
                assert 1 in {i[8 + d] for c, i in rows for d in range(2)}, prec
                assert 1 in {i[10 + d] for c, i in rows for d in range(2)}, prec
        elif proc.startswith('two_level'):
            n1 = {i[2 + d] for c, i in rows for d in range(3)}
            n2 = {i[5 + d] for c, i in rows for d in range(3)}
            assert n1 >= {1, 2, 3, 4, 5, 6, 8, 7, 9, 10, 32}, (prec, sorted(n1))
            assert n2 >= set(LISTED_N2) | {17, 7, 9}, (prec, sorted(n2))
            for d in range(3):               # a split on every axis, and a whole axis next to split ones
                assert any(i[2 + d] > 1 for c, i in rows), (prec, d)
            assert any(min(i[2:5]) == 1 and max(i[2:5]) > 1 for c, i in rows), prec
            if proc == 'two_level':
                for d in range(3):
                    assert any(i[12 + d] for c, i in rows), ('no MFMA stage A on axis', d, prec)
                # the matrix cores at every listed H that fits them in this type (shortest length 2 N2): all in f32,
                # up to H = 30 in f64 -- the tile tails H = 15, 63 (one short of an edge), 65 (one past), MT up to 5
                need = {n2 for n2 in LISTED_N2 if mfma_xy(2, n2, prec)[1]}
                assert need == (set(LISTED_N2) if prec == 4 else {3, 5, 31, 37, 61}), (prec, sorted(need))
                got = {i[5 + d] for c, i in rows for d in range(3) if i[12 + d]}
                assert got >= need, ('MFMA stage A never ran at N2 =', sorted(need - got), prec)
            if proc == 'two_level_small_lds':
                nc = {i[8] for c, i in rows} | {i[9] for c, i in rows}
                nl = {i[10] for c, i in rows} | {i[11] for c, i in rows}
                assert nc >= {1, 2, 4} and nl >= {2, 4}, (prec, sorted(nc), sorted(nl))
                assert 1 in nl or prec == 4, (prec, sorted(nl))         # f32: two_level_lds8


@pytest.mark.gpu
def test_mesh_convolve_every_path_bin_by_bin(tmp_path):
    t_start = time.time()
    clean = {k: v for k, v in os.environ.items() if not k.startswith('ADMP_') or k == 'ADMP_HIP_LIB'}
    runs = {}
    for proc, switches in PROCESSES:          # the children, one after the other; the first that fails ends the test
        cases = cases_of(proc)
        d = tmp_path / proc
        d.mkdir()
        (d / 'cases.json').write_text(json.dumps(cases))
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), 'child', str(d / 'cases.json'), str(d)],
                           capture_output=True, text=True, env=dict(clean, **switches), timeout=600, cwd=ROOT)
        assert r.returncode == 0 and 'MESH-CHILD-OK' in r.stdout, (proc, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        runs[proc] = (cases, json.load(open(d / 'results.json')), d)
        print('%s: %d cases on the GPU in %.1f s' % (proc, len(cases), time.time() - t0))
    # which form ran
    for proc, (cases, res, d) in runs.items():
        for c in cases:
            expected_info(proc, c, res[c['id']]['info'])
        coverage(proc, [(c, res[c['id']]['info']) for c in cases])
    # numbers: one reference per (mesh, box, kappa, table, type, input), every process that ran it checked against it
    groups = {}
    for proc, (cases, res, d) in runs.items():
        for c in cases:
            groups.setdefault(ref_key(c), []).append((proc, c, res[c['id']], d))
    figures = []
    table_of, G = None, None
    for key in sorted(groups, key=lambda k: (k[0], k[1], k[3], k[4], k[2], k[5], k[6])):      # keys of one table together
        members = groups[key]
        c0 = members[0][1]
        K = tuple(c0['K'])
        if table_of != key[:5]:
            G = half_spectrum_table(g_table(make_box(K, c0['tric']), K, c0['kappa'], c0['which'], c0['ref_order']))
            table_of = key[:5]
        noise_in = c0['input']['kind'] == 'noise'
        if c0['kind'] == 'flat':
            assert g_ratio(G) < 1e5, (c0['id'], g_ratio(G))
        r = Reference(make_input(c0), G, c0['prec'], per_bin=noise_in)
        for proc, c, res, d in members:
            out = np.load(d / (c['id'] + '.npy'))
            fig = check_case(c, r, out, res['E'])
            figures.append((proc, c, fig))
            print('%-20s %-52s %s' % (proc, c['id'], ' '.join('%s=%.3g' % (k, v) for k, v in fig.items() if k != 'worst_bin')))
        del r
    # f32 per bin: C from the rocFFT 3-D path, the hand-written paths within 8 C
    # One C per kind of kappa: the issue's single C (the larger, from the production kappa, where the error of a small-G
    # bin comes from the large-G bins of its lines) would leave the flat-kappa cases some 13 times more room than rocFFT needs
    Ck = {}
    for kind in ('prod', 'flat'):
        cal = [f['bin/model'] for p, c, f in figures if p == 'rocfft' and 'bin/model' in f and c['kind'] == kind]
        Ck[kind] = max(cal)
        print('f32 model constant C(%s kappa) = %.4g (rocFFT 3-D path, %d cases)' % (kind, Ck[kind], len(cal)))
    worst = {}
    for proc, c, f in figures:
        for k, v in f.items():
            if k != 'worst_bin':
                kk = '%s f%d %s' % (proc, 8 * c['prec'], k)
                worst[kk] = max(worst.get(kk, 0.0), v)
        if 'bin/model' in f:
            kk = '%s f32 %s bin/(C model)' % (proc, c['kind'])
            worst[kk] = max(worst.get(kk, 0.0), f['bin/model'] / Ck[c['kind']])
    for k in sorted(worst):
        print('worst  %-48s %.3g' % (k, worst[k]))
    for proc, c, f in figures:
        if 'bin/model' not in f:
            continue
        factor = 1.0 if proc == 'rocfft' else HAND_FACTOR
        C = Ck[c['kind']]
        assert f['bin/model'] <= factor * C, (proc, c['id'], f, C)
        if 'model/signal' in f:
            # the tolerance of the hand-written paths, 8 C model(k), below a tenth of the signal in every bin: a mis-routed
            # bin, which is off by the whole signal, fails
            assert HAND_FACTOR * C * f['model/signal'] < 0.1, (proc, c['id'], f, C)
    print('wall time of the file: %.0f s' % (time.time() - t_start))


@pytest.mark.gpu
def test_mesh_convolve_refuses_a_slab_handle_and_bad_arguments():
    import ctypes
    import torch                             # before the library, as everywhere else
    torch.cuda.init()
    from admp_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.admp_create(ctypes.byref(h), 0, 8) == 0
    x = np.zeros((8, 8, 8))
    box = _lib.darr(make_box((8, 8, 8), False))
    E = ctypes.c_double(0.0)
    info = (ctypes.c_int * _lib.MESH_INFO_WORDS)()
    p = x.ctypes.data_as(ctypes.c_void_p)
    assert L.admp_mesh_convolve(h, box, 1, p, 0, ctypes.byref(E), info) != 0          # no admp_set_ewald yet
    _lib.check(h, L.admp_set_ewald(h, 0.5, 8, 8, 8, 2, 0), 'admp_set_ewald')
    assert L.admp_mesh_convolve(h, box, 7, p, 0, ctypes.byref(E), info) != 0          # no such table
    assert L.admp_mesh_convolve(h, box, 1, p, 0, ctypes.byref(E), info) == 0
    _lib.check(h, L.admp_slab_configure(h, 0, 2), 'admp_slab_configure')
    assert L.admp_mesh_convolve(h, box, 1, p, 0, ctypes.byref(E), info) != 0
    assert b'single rank' in L.admp_last_error(h)
    L.admp_destroy(h)


@pytest.mark.gpu
def test_an_evaluation_on_a_mesh_below_six_points_is_refused():
    """admp_set_ewald takes short meshes for admp_mesh_convolve; whatever spreads or gathers (order-6 splines) must refuse them"""
    import torch                             # before the library, as everywhere else
    torch.cuda.init()
    from admp_amd import _lib
    from admp_amd import systems as S
    from admp_amd.pme import ADMPPmeForce
    n_mol = 64
    pos, box = S.synthetic_water_box(n_mol, seed=7)
    at, ai, cov = S.water_topology(n_mol)
    par = S.water_parameters(n_mol, polarizable=True)
    pairs = S.build_pairs(pos, box, 4.0)
    for K in ((4, 8, 8), (8, 5, 8), (8, 8, 2)):
        f = ADMPPmeForce(box, at, ai, cov, 4.0, 1e-4, 2, lpol=True)
        f.K1, f.K2, f.K3 = K
        f.refresh_calculators()
        with pytest.raises(_lib.AdmpHipError, match='at least 6 points'):
            f.get_forces(pos, box, pairs, par['Q_local'], par['pol'], par['tholes'], par['mScales'], par['pScales'], par['dScales'])


if __name__ == '__main__' and len(sys.argv) == 4 and sys.argv[1] == 'child':
    child_main(sys.argv[2], sys.argv[3])
