"""No GPU: the reference, the inputs and the bars of tests/mesh_ref.py, which tests/test_gpu_mesh_spread_gather.py holds the
spread and gather kernels to.

* The long-double recursion reference equals oracle.spread_Q (mesh) and autograd of sum phi * spread_Q (pot, grad: exactly
  what test_kernel_math_cpu.py::test_spread_and_gather_match_oracle compares, including the reference's operator matrix on
  triclinic cells) to the oracle's own accuracy: its truncated-power splines lose ~1e-13 absolute in float64.
* The brick rule of brick_plan.h (make_bricks, brick_of, brick_code) is restated in mesh_ref.py and checked here against the
  host-compiled header (tests/hostshim/brick_plan_shim.cpp), the way cell_plan.h is checked.
* Every case has what it is named for: entry counts, class runs, seam crossings, scan rounds, empty bricks, atoms on mesh
  points and one ulp below a face.
* C_host: the largest err / (u W) of the host-compiled arithmetic (tests/hostshim shim_mesh_spread / shim_mesh_gather: the
  inline functions of spline_math.h in T, atoms summed in double) against the reference, over all cases.  Asserted below the
  recorded value mesh_ref.C_HOST (the measurement rounded up in its third digit; the device bars are DEVICE_FACTOR = 4 times it) and below C_CAP, counted from the
  operation chain to first order: a mesh value is a sum of products coefficient x weight x weight x weight; a weight comes out
  of bspline6 after 4 recursion levels of 6 roundings each (f + p, n - f - p, two products, one sum, one scale) and up to 5
  more for a derivative's differences: 29 per weight, 87 for three; fold_multipole adds 13 (Theta/3 from the harmonics 3,
  Theta Aop 5, Aop^T (.) 5), the site's rotation and dipole sum 7, the row factors P0..P2 and the three-term sum over the z
  weights 7 + 5: 119 <= C_CAP = 120.  (The coordinate's own 7 roundings are charged to the coordinate term of W.)
  Measured: C_host = 4.25 (f32) and 2.74 (f64), both on shift32_n600; the gather outputs stay below 1.0; recorded as 4.3
  and 2.75, so the device bars are 17.2 u W and 11 u W.  The file takes 35 s (references in long double, shared with the GPU test).
* Unreached words are exactly zero, and two host spreads agree bit for bit.
* Sensitivity: for every case, type and form, dropping one (atom, x, y) column, one x plane of an atom, one (atom, brick)
  entry, or a site's highest moments (a lower class) changes at least one word by more than the DEVICE bar -- for the atom for
  which it changes least, each mutation taken where it shows most for that atom (a column at the stencil's edge has weight
  f^5 / 120, exactly 0 on a mesh point: no test can see it).  Likewise one z column of one atom in the gather, in pot or grad,
  and in phi behind the convolution for the plane kernel.  The f32 range case: asserted for the large sites and for the
  atoms of the uncrowded bricks; the ratio of the rest is printed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import admp_oracle as O
from tests import mesh_ref as R
from tests.hostshim_util import lib, dp, c64

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostshim', 'brick_plan_shim.cpp')
LIB = os.path.join(HERE, 'hostshim', 'libadmp_brickplanshim.so')
HDR = os.path.join(os.path.dirname(HERE), 'admp_amd', 'csrc', 'brick_plan.h')
_blib = None
FORMS = ('scan', 'planes', 'bricks')


def blib():
    global _blib
    if _blib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in (SRC, HDR)):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC])
        _blib = ctypes.CDLL(LIB)
    return _blib


def T(a):
    return torch.as_tensor(np.array(a, dtype=np.float64))


def test_brick_rule_restatement_matches_the_header():
    L = blib()
    rng = np.random.default_rng(3)
    for K in [(6, 7, 16), (17, 18, 33), (32, 32, 32), (32, 48, 16), (33, 31, 47), (97, 20, 23), (160, 15, 200), (16, 17, 511)]:
        Ki = np.array(K, dtype=np.int32)
        nb4 = np.zeros(4, dtype=np.int32)
        L.brick_plan_grid(dp(Ki), dp(nb4))
        nb = R.make_bricks(K)
        assert tuple(nb4[:3]) == nb and nb4[3] == nb[0] * nb[1] * nb[2]
        for d in range(3):
            got = [L.brick_plan_of(i, nb[d], K[d]) for i in range(K[d])]
            assert got == [int(b) for b in R.brick_of(np.arange(K[d]), nb[d], K[d])]
            # bricks are the intervals [b K / nb, (b + 1) K / nb), each of at least 6 points where the axis has more than one
            assert got == sorted(got) and got[0] == 0 and got[-1] == nb[d] - 1
            assert all(got[R.brick_lo(b, nb[d], K[d])] == b and (b == 0 or got[R.brick_lo(b, nb[d], K[d]) - 1] == b - 1) for b in range(nb[d]))
            assert nb[d] == 1 or np.bincount(got).min() >= 6
        bases = np.stack([rng.integers(0, K[d], 400) for d in range(3)], axis=1).astype(np.int32)
        bases[:3] = [[0, 0, 0], [K[0] - 1, K[1] - 1, K[2] - 1], [K[0] - 6, K[1] - 6, K[2] - 6]]
        codes = np.zeros(len(bases), dtype=np.int32)
        L.brick_plan_codes(len(bases), dp(np.ascontiguousarray(bases)), dp(Ki), dp(codes))
        assert [int(x) for x in codes] == [R.brick_code(b, K) for b in bases]
        # the entries of the rule are exactly the bricks that hold a point of the stencil
        atoms, cells = R.brick_entries(bases, K)
        wb = R.word_bricks(K).reshape(-1)[R.point_index(bases.astype(np.int64), K)]
        for i in range(0, len(bases), 7):
            if min(nb) > 1:
                assert sorted(cells[atoms == i]) == sorted(np.unique(wb[i])), (K, bases[i])


SMALL = [n for n in R.CASES if R.case(n)['n'] <= 700]


@pytest.mark.parametrize('name', SMALL)
def test_reference_matches_oracle(name):
    c = R.case(name)
    prec = c['precs'][0]
    r = R.spread_ref(name, prec)
    x = R.rounded(c, prec)
    Qt = R.qtot(x['Q'], x['U'])
    K = list(c['K'])
    mesh = O.spread_Q(T(x['pos']), T(c['box']), T(Qt), K, 2).numpy()
    d = np.abs(np.asarray(r.mesh, dtype=np.float64) - mesh).max()
    print('%-14s mesh: |ref - oracle| %.2e of %.2e' % (name, d, np.abs(mesh).max()))
    assert d <= 1e-11 * np.abs(mesh).max()
    for kind in ('noise', 'wave'):
        g = R.gather_ref(name, prec, kind)
        phi = R.phi_noise(c, prec) if kind == 'noise' else R.phi_wave(c, prec)
        p, q = T(x['pos']).requires_grad_(True), T(Qt).requires_grad_(True)
        s = torch.sum(O.spread_Q(p, T(c['box']), q, K, 2) * T(phi))
        gp, gq = torch.autograd.grad(s, [p, q])
        assert np.abs(g.pot - gq.numpy()).max() <= 1e-10 * np.abs(g.pot).max()
        assert np.abs(g.grad - gp.numpy()).max() <= 1e-10 * np.abs(g.grad).max()
        assert abs(g.E - 0.5 * float(s.detach())) <= 1e-11 * max(abs(g.E), float(np.abs(Qt * g.pot).sum()))     # E = 1/2 sum Q . pot
        b = g.bars()
        assert (b['pot'] > 0).all() and (b['grad'] > 0).all() and b['E'] > 0


def _seam_crossings(base, K):
    return [(base[:, d] + 5 >= K[d]).sum() for d in range(3)]


@pytest.mark.parametrize('name', R.CASES)
def test_case_has_what_it_is_named_for(name):
    c = R.case(name)
    K, n = c['K'], c['n']
    nb = R.make_bricks(K)
    for prec in c['precs']:
        r = R.spread_ref(name, prec)
        cnt = r.cnt.reshape(nb)
        kinds_of = lambda cell: np.bincount(r.kinds[r.ent_atom[r.ent_cell == (cell[0] * nb[1] + cell[1]) * nb[2] + cell[2]]], minlength=3)      # noqa: E731
        assert (np.asarray(r.rm, dtype=np.float64) == np.asarray(r.rm, dtype=np.float64)).all()
        if name == 'one_brick_n33':
            assert nb == (1, 1, 1) and n == 33 and c['tric']
            f = np.asarray(np.ceil(r.rm) - r.rm, dtype=np.float64)
            assert (f < 1e-6).any() and (f > 1 - 1e-5).any()        # on / just below mesh points: the last / the first weight ~ 0
            assert all(s >= 2 for s in _seam_crossings(r.base, K))   # stencils across the seam of every axis
            assert (np.abs(np.asarray(c['pos']) @ np.linalg.inv(c['box'])).max(0) > 49).all()     # 50 cells away
            assert R.plane_spread_fits(K, n, 'double') is False
        if name == 'bricks2_n65':
            assert nb == (2, 2, 3) and n == 65 and not c['tric'] and c['lpol']
            assert [R.brick_lo(1, 2, 17), R.brick_lo(1, 2, 18), R.brick_lo(1, 3, 33), R.brick_lo(2, 3, 33)] == [8, 9, 11, 22]
            assert (cnt[:, :, 2] == 0).all() and (cnt[:, :, :2] > 0).all()      # bricks without a single entry
            assert r.unreached[:, :, 23:32].all() and not r.unreached[:, :, :20].all()
            per_atom = np.bincount(r.ent_atom, minlength=n)
            assert per_atom.max() == 8 and per_atom.min() == 1                   # a stencil over a brick corner; one inside a brick
            mono = np.abs(np.asarray(c['Q'])[:, 1:]).sum(1) == 0
            hasU = np.abs(np.asarray(c['U'])).sum(1) > 0
            assert (mono & hasU & (r.kinds == R.KIND_GENERAL)).sum() == (mono & hasU).sum() >= 8      # U makes charge-only sites general
            assert (mono & ~hasU & (r.kinds == R.KIND_CHARGE)).sum() == (mono & ~hasU).sum() >= 4
        if name == 'classes':
            assert nb == (2, 2, 3) and c['tric']
            for cell, want in R.CLASS_BRICKS.items():
                assert tuple(kinds_of(cell)) == want, (cell, kinds_of(cell))
            # sorted places 0..63 general, 64..127 dipole, 128..191 charge: boundaries ON a group of 64; 63 | 65 | 1: inside
            assert cnt.sum() == n == 441
        if name == 'shift32_n600':
            assert nb == (2, 2, 2) and all(R.brick_lo(1, 2, 32) == 16 for _ in range(1)) and cnt.min() > 0
        if name == 'zbrick1_n500':
            assert nb == (2, 3, 1) and c['tric']
        if name == 'chunk_n2400':
            cell = c['crowded']
            assert cnt[cell] > R.BRICK_CHUNK and cnt[cell] <= 2 * R.BRICK_CHUNK and (kinds_of(cell) > 500).all()
            assert np.sort(cnt.reshape(-1))[-2] < R.BRICK_CHUNK
            assert all(s >= 20 for s in _seam_crossings(r.base, K)[1:2])        # the crowded brick lies on the y seam
        if name == 'xplane_n31':
            assert n == 31 and len(np.unique(r.base[:, 0])) == 1 and nb == (7, 2, 2)
        if name in ('n1', 'n32'):
            assert n == int(name[1:])
        if name == 'range_f32':
            assert c['precs'] == ('single',) and cnt[c['crowded']] == 400
            Qa = np.abs(np.asarray(c['Q']))
            assert Qa[c['big']].min() > 100 * Qa[5:].max()
        if name.startswith('plane_n'):
            assert K == (33, 31, 47) and R.plane_spread_fits(K, n, 'double') and not R.plane_spread_fits(K, n, 'single')
            assert (n + R.SCAN_ROUND - 1) // R.SCAN_ROUND == {3072: 1, 3073: 2, 8192: 3}[n]
            assert not R.plane_spread_fits(K, 8193, 'double')
    # gather workgroups of 32 atoms: the sizes around one and two workgroups and the padded grid of eight
    assert sorted(R.case(m)['n'] for m in ('n1', 'xplane_n31', 'n32', 'one_brick_n33', 'bricks2_n65')) == [1, 31, 32, 33, 65]
    for Km in [(17, 18, 33), (32, 32, 32), (32, 48, 16), (97, 20, 23), (6, 7, 16)]:
        assert not R.plane_spread_fits(Km, 100, 'double')       # the plane kernel spreads on 33 x 31 x 47 only, of these meshes


def _host(c, prec, r):
    x = R.rounded(c, prec)
    Ki = np.array(c['K'], dtype=np.int32)
    Uc = dp(c64(x['U'])) if c['lpol'] else None
    mesh = np.zeros(c['K'])
    args = (R.PREC_BYTES[prec], c['n'], dp(c64(x['pos'])), dp(c64(x['Q'])), Uc, dp(c64(c['box'])), dp(Ki))
    lib().shim_mesh_spread(*args, dp(mesh))
    again = np.zeros(c['K'])
    lib().shim_mesh_spread(*args, dp(again))
    phi = R.phi_noise(c, prec)
    pot, grad, fld = np.zeros((c['n'], 9)), np.zeros((c['n'], 3)), np.zeros((c['n'], 3))
    lib().shim_mesh_gather(*args, dp(c64(phi)), dp(pot), dp(grad), dp(fld))
    return mesh, again, pot, grad, fld


@pytest.mark.parametrize('name', R.CASES)
def test_host_constant_and_mutants(name):
    c = R.case(name)
    for prec in c['precs']:
        u = R.U[prec]
        r = R.spread_ref(name, prec)
        mesh, again, pot, grad, fld = _host(c, prec, r)
        assert np.array_equal(mesh, again)
        assert not mesh[r.unreached].any()
        err = np.abs(mesh - np.asarray(r.mesh, dtype=np.float64))
        ok = r.W > 0
        assert not err[~ok].any()
        Cs = float((err[ok] / (u * r.W[ok])).max())
        g = R.gather_ref(name, prec)
        with np.errstate(divide='ignore', invalid='ignore'):
            Cg = max(float(np.nanmax(np.abs(pot - g.pot) / (u * g.pot_abs))), float(np.nanmax(np.abs(grad - g.grad) / (u * g.grad_abs))),
                     float(np.nanmax(np.abs(fld - g.fld) / (u * g.pot_abs[:, [2, 3, 1]]))))
        print('C_HOST %-14s %-6s spread %.2f gather %.2f (recorded %.1f, cap %.0f)' % (name, prec, Cs, Cg, R.C_HOST[prec], R.C_CAP))
        assert max(Cs, Cg) <= R.C_HOST[prec] <= R.C_CAP
        # ---- sensitivity at the device bars
        forms = FORMS + (('plane_kernel',) if R.plane_spread_fits(c['K'], c['n'], prec) else ())
        for form in forms:
            m = R.mutant_ratios(r, form)
            if name == 'range_f32':
                wb = R.word_bricks(c['K'])
                base_cell = wb.reshape(-1)[R.point_index(r.base, c['K'])[:, 0, 0, 0]]
                crowd = (c['crowded'][0] * 2 + c['crowded'][1]) * 2 + c['crowded'][2]
                held = np.zeros(c['n'], dtype=bool)
                held[c['big']] = True
                held |= base_cell != crowd
                rest = ~held
                print('SENS  %-14s %-6s %-12s small sites of the crowded brick (not asserted): %s' % (
                    name, prec, form, ' '.join('%s %.3g' % (k, v[rest].min()) for k, v in m.items() if len(v) == c['n'])))
                m = {k: (v[held] if len(v) == c['n'] else v) for k, v in m.items()}
                m.pop('class')                   # (every site is general here: the class mutant is the column check's)
            print('SENS  %-14s %-6s %-12s %s' % (name, prec, form, ' '.join('%s %.3g' % (k, v.min()) for k, v in m.items())))
            for k, v in m.items():
                assert len(v) and v.min() > 1.0, (name, prec, form, k, float(v.min()))
        z = g.zcol_mutant_ratio()
        print('SENS  %-14s %-6s gather z column %.3g' % (name, prec, z.min()))
        assert z.min() > 1.0
        if 'plane_kernel' in forms:
            # behind the convolution: the least visible atom's column, convolved, against the bar of phi
            cv = R.convolved(r)
            bar_phi = cv['B_word'] + cv['sumG'] * float(r.bar('plane_kernel').sum())
            col = R.mutant_ratios(r, 'plane_kernel')['column']
            i = int(np.argmin(col))
            v = np.abs(np.asarray(r.vals[i], dtype=np.float64))
            a, b = np.unravel_index(np.argmax(v.max(axis=2)), (6, 6))
            d = np.zeros(int(np.prod(c['K'])))
            np.add.at(d, R.point_index(r.base, c['K'])[i, a, b, :], np.asarray(r.vals[i, a, b, :], dtype=np.float64))
            dphi = np.fft.ifftn(cv['G'] * np.fft.fftn(d.reshape(c['K']))).real * d.size
            print('SENS  %-14s %-6s phi behind the convolution %.3g' % (name, prec, np.abs(dphi).max() / bar_phi))
            assert np.abs(dphi).max() > bar_phi
