"""No GPU: the reference, the cases and the bars of tests/disp_mesh_ref.py, which tests/test_gpu_disp_mesh_legs.py holds the
dispersion spread and gather legs to.

* the scalar reference equals the oracle's dispersion spread (spread_Q with lmax = 0, as disp_pme_parts calls it through
  pme_recip) and its autograd, at the accuracy tests/test_mesh_ref_cpu.py uses for the multipolar one;
* the per-type meshes recombine to the per-power meshes, sum_t c_p,t M_t = M_p, to long-double rounding; the typed and untyped
  self terms agree;
* every case puts in play what its name says; the path table names every path for some (case, child, pmax, precision);
* mutants: every defect of the list exceeds its bar for every atom it touches -- the condition under which the GPU test cannot
  hide it.  The smallest ratio per mutant and precision is printed (-s).  A case that cannot show a mutant (a zero coefficient
  hides a swap; equal coefficients hide a stride) is left out of THAT mutant only: at most a quarter of the cases it applies
  to, the count is printed and asserted.  Two such exclusions exist, both of crowded_range in f32: the 595 small-coefficient
  atoms of its crowded brick in the entry / column mutants (the brick's quantum is set by its five large atoms: a lost entry of
  a small atom there is undetectable in f32), and those five atoms in the swap mutant (their C10 rounding alone is the size of
  their C6 and C8 terms);
* the composition check's inputs mean what the oracle means: the reference gather of the float64-convolved reference meshes
  (phi_p per power, psi_t per type) equals the oracle's reciprocal gradient to 1e-11."""
import numpy as np
import pytest
import torch

from oracle import admp_oracle as O
from tests import disp_mesh_ref as D
from tests import mesh_ref as R

PRECS = ('double', 'single')
UNTYPED = [n for n in D.CASES if D.case(n)['types'] is None]
TYPED = [n for n in D.CASES if D.case(n)['types'] is not None]


def T(a):
    return torch.as_tensor(np.array(a, dtype=np.float64))


def test_scalar_reference_matches_the_oracles_dispersion_spread():
    name, prec = 'n65_rocfft', 'double'
    c = D.case(name)
    K = list(c['K'])
    cr = D.rounded_c(c, prec)
    pos = np.asarray(c['pos'], dtype=np.float64)
    phi = D.phi_batch(c, prec, 3)
    for p in range(3):
        r = D.channel_ref(name, prec, p)
        mesh = O.spread_Q(T(pos), T(c['box']), T(cr[:, p:p + 1]), K, 0).numpy()
        d = np.abs(np.asarray(r.mesh, dtype=np.float64) - mesh).max()
        print('channel %d mesh: |ref - oracle| %.2e of %.2e' % (p, d, np.abs(mesh).max()))
        assert d <= 1e-11 * np.abs(mesh).max()
        g = R.GatherRef(r, phi[p])
        x, q = T(pos).requires_grad_(True), T(cr[:, p:p + 1]).requires_grad_(True)
        s = torch.sum(O.spread_Q(x, T(c['box']), q, K, 0) * T(phi[p]))
        gx, gq = torch.autograd.grad(s, [x, q])
        assert np.abs(g.grad - gx.numpy()).max() <= 1e-10 * np.abs(g.grad).max()
        assert np.abs(g.pot[:, 0] - gq.numpy()[:, 0]).max() <= 1e-10 * np.abs(g.pot[:, 0]).max()


@pytest.mark.parametrize('name', TYPED)
def test_type_meshes_recombine_to_power_meshes_and_self_terms_agree(name):
    c = D.case(name)
    for prec in c['precs']:
        tab = D.rounded_ctab(c, prec)
        for p in range(3):
            Mp = D.channel_ref(name, prec, p).mesh
            Mt = sum(D.LD(tab[t, p]) * D.type_ref(name, prec, t).mesh for t in range(c['nt']))
            scale = float(np.abs(np.asarray(D.channel_ref(name, prec, p).W, dtype=np.float64)).max()) + 1e-300
            assert float(np.abs(Mp - Mt).max()) <= 64 * 2.0 ** -64 * c['n'] * scale, (name, prec, p)
        for pmax in (6, 8, 10):
            e, bar, et = D.self_reference(c, prec, pmax)
            assert abs(e - et) <= bar, (name, prec, pmax, e, et, bar)


@pytest.mark.parametrize('name,pmax,per_type,prec', D.COMPOSITION[:3])
def test_composition_reference_meets_the_oracle(name, pmax, per_type, prec):
    """the reference gather of the float64-convolved reference meshes (phi_p, or psi_t per type) is the oracle's reciprocal
    gradient: what the GPU test's composition check hands to the gather leg means what the oracle means"""
    phi, g_oracle = D.composition(name, prec, pmax, per_type)
    g, _ = D.gather_reference(name, prec, pmax, per_type, phi)
    rel = np.linalg.norm(g - g_oracle) / np.linalg.norm(g_oracle)
    print('composition %-20s pmax %2d %-8s |ref - oracle| / |oracle| = %.2e' % (name, pmax, 'per type' if per_type else 'per power', rel))
    assert rel < 1e-11


def _brick_cnt(c, r):
    nb = R.make_bricks(c['K'])
    return r.cnt.reshape(nb)


@pytest.mark.parametrize('name', D.CASES)
def test_case_has_what_it_is_named_for(name):
    c = D.case(name)
    K, n = c['K'], c['n']
    nb = R.make_bricks(K)
    r = D.channel_ref(name, 'double', 0)
    cnt = _brick_cnt(c, r)
    frac = np.asarray(c['pos']) @ np.linalg.inv(c['box'])
    assert c['c'].shape == (n, 3) and all(p in (6, 8, 10) for p in c['pmaxes'])
    if 'shifted' in c:
        assert (np.abs(frac).max(0) > 47).all() and ((frac < 0) | (frac > 1)).any(axis=1).sum() >= 2      # about 50 cells away; outside the cell
    if name == 'n1':
        assert n == 1
    if name == 'n31_negative_onpoints':
        assert n == 31 and (c['c'] < 0).any() and (c['c'] > 0).any()
        f = np.asarray(np.ceil(r.rm) - r.rm, dtype=np.float64)
        assert (f[c['on_points']] < 1e-9).all()                    # exactly on mesh points: the last weight is 0
    if name == 'n33_zero_rows':
        assert n == 33 and (np.abs(c['c'][c['zero_rows']]).sum() == 0) and len(c['zero_rows']) == 3
    if name.startswith('n65_'):
        assert n == 65
    if name == 'n65_general':
        assert nb == (2, 3, 3) and c['tric'] and len({R.brick_lo(b + 1, 3, 33) - R.brick_lo(b, 3, 33) for b in range(3)} |
                                                    {R.brick_lo(b + 1, 3, 35) - R.brick_lo(b, 3, 35) for b in range(3)}) > 1
    if name == 'n65_one_brick_y':
        assert nb[1] == 1 and nb[0] > 1 and nb[2] > 1
    if name == 'n65_dft17':
        assert nb == (2, 2, 2) and [R.brick_lo(1, 2, k) for k in K] == [16, 8, 9] and D.mesh_is_direct(K, {})
    if name == 'n257_nt3_minority':
        t = np.bincount(c['types'], minlength=3)
        assert n == 257 and t[c['minority']] == 3 and c['types'][256] == 1 and np.abs(c['ctab'][2]).sum() == 0 and t[2] > 0
    if name == 'n65_nt2_empty_type':
        assert np.bincount(c['types'], minlength=2)[c['empty_type']] == 0 and c['nt'] == 2
    if name in ('n40_nt1', 'n40_nt1_fx'):
        assert c['nt'] == 1
    if name == 'n257_nt2_dft':
        assert n == 257 and c['nt'] == 2 and c['types'][256] == 1 and D.mesh_is_direct(K, {'ADMP_DFT': '1'})
    if name == 'crowded_range':
        assert 590 <= cnt[c['crowded']] <= 610 and cnt[c['crowded']] == 600
        assert (cnt == 0).any() and 0 < np.sort(cnt.reshape(-1))[-2] <= 20
        ca = np.abs(c['c'])
        assert ca[c['big'], 0].min() > 500 * ca[5:, 0].max() and np.allclose(ca[c['big'], 2], 1e4 * ca[c['big'], 0])
        cell = (c['zero_c8_brick'][0] * nb[1] + c['zero_c8_brick'][1]) * nb[2] + c['zero_c8_brick'][2]
        atoms = r.ent_atom[r.ent_cell == cell]
        assert len(atoms) == 12 and (c['c'][atoms, 1] == 0).all() and (c['c'][atoms, 0] != 0).all()      # the ex = 20 branch
    if name == 'xplane_n40':
        assert len(np.unique(r.base[:, 0])) == 1
    if name == 'n2100_nt2_chunks':
        assert n == 2100 > 2048 and 2048 < cnt[c['crowded']] <= 4096 and np.bincount(c['types']).min() > 256
    if c['types'] is not None:
        assert (c['c'] == c['ctab'][c['types']]).all()


def test_sizes_and_paths_cover_what_the_issue_names():
    ns = sorted(D.case(m)['n'] for m in D.CASES)
    assert {1, 31, 33, 65, 257, 2100} <= set(ns)
    seen = set()
    for tag, (env, meshes) in D.CHILDREN.items():
        assert len(meshes) <= 3
        for name in D.CASES:
            c = D.case(name)
            if c['K'] not in meshes:
                continue
            for prec in c['precs']:
                for pmax in c['pmaxes']:
                    for nt in ({0, c['nt']}):
                        path, nmesh, per_type = D.expected_path(c['K'], c['n'], env, pmax, nt, prec)
                        seen.add((path, prec, (pmax - 4) // 2 if not per_type else nmesh))
                        if path in D.BRICK_PATHS + ('DftTyped', 'DftBatched', 'PerPower'):
                            seen.add((tag, path))
    for path in ('BricksBatched', 'DftBatched'):
        assert {(path, p, k) for p in PRECS for k in (2, 3)} <= seen, path
    for path in ('BricksPerPower', 'PerPower'):
        assert {(path, p, 1) for p in PRECS} <= seen, path
    assert {('BricksTyped', 'single', k) for k in (1, 2, 3)} | {('DftTyped', p, k) for p in PRECS for k in (1, 2)} <= seen, seen
    assert ('BricksTyped', 'double', 2) not in seen
    assert {('default', 'PerPower'), ('bricks', 'BricksTyped'), ('bricks', 'BricksBatched'), ('bricks', 'BricksPerPower'),
            ('bricks', 'PerPower'), ('dft', 'DftTyped'), ('dft', 'DftBatched'), ('dft_bricks', 'DftBatched')} <= seen


BRICK_CASES = [n for n in UNTYPED if min(R.make_bricks(D.case(n)['K'])) > 1]


def _allowed_out(total):
    return total // 4


@pytest.mark.parametrize('prec', PRECS)
def test_spread_mutants_exceed_their_bars(prec):
    worst = {'entry': np.inf, 'column': np.inf, 'tile': np.inf}
    left_out = []
    for name in BRICK_CASES:
        c = D.case(name)
        for p in range((max(c['pmaxes']) - 4) // 2):
            ent, col = D.mutant_entry_dropped(name, prec, p)
            if p == 0 and len(ent) < (D.rounded_c(c, prec)[:, 0] != 0).sum():
                left_out.append((name, int((D.rounded_c(c, prec)[:, 0] != 0).sum() - len(ent))))
            worst['entry'] = min(worst['entry'], ent.min())
            worst['column'] = min(worst['column'], col.min())
    for name in TYPED:
        if min(R.make_bricks(D.case(name)['K'])) > 1:
            worst['tile'] = min(worst['tile'], D.mutant_wrong_tile(name, prec).min())
    # crowded_range in f32: the quantum of the crowded brick is set by its five large atoms, so a lost entry (or column) of one
    # of its 595 small-coefficient atoms lies UNDER the bar and is undetectable in f32 by any test that grants the kernel its
    # scale rule.  Those atoms are left out of the entry and column mutants there; the case counts as left out.
    print('MUTANT %-8s spread entry / column: cases left out (atoms): %d of %d %s' % (prec, len(left_out), len(BRICK_CASES), left_out))
    assert len(left_out) <= _allowed_out(len(BRICK_CASES))
    assert left_out == ([('crowded_range', 595)] if prec == 'single' else [])
    for k, v in worst.items():
        print('MUTANT %-8s spread %-7s smallest change / bar over the atoms it touches: %.3g' % (prec, k, v))
        assert v > 1.0, (k, v)


@pytest.mark.parametrize('prec', PRECS)
def test_gather_mutants_exceed_their_bars(prec):
    cases = [n for n in UNTYPED if D.case(n)['n'] <= 700]
    for kind in ('swap', 'stride', 'zcol'):
        worst, left_out = np.inf, []
        for name in cases:
            c = D.case(name)
            pmax = max(c['pmaxes'])
            if pmax == 6 and kind == 'swap':
                left_out.append(name)             # one channel: nothing to swap
                continue
            ratios, touched = D.mutant_gather(name, prec, pmax, kind)
            assert touched.sum() >= max(1, c['n'] - 4), (name, kind, touched.sum())
            if 'big' in c and prec == 'single' and kind == 'swap':
                # the five large atoms carry C10 = 1e4 C6: in f32 the rounding of their C10 term alone, which the bar must
                # grant, is of the size of their whole C6 and C8 terms.  The case shows the swap on its other 627 atoms only,
                # and is counted as left out.
                keep = np.ones(c['n'], dtype=bool)
                keep[c['big']] = False
                ratios = ratios[keep[touched]]
                left_out.append(name)
            worst = min(worst, ratios.min())
        print('MUTANT %-8s gather %-7s smallest change / bar over the atoms it touches: %.3g; cases left out: %d of %d %s'
              % (prec, kind, worst, len(left_out), len(cases), left_out))
        assert len(left_out) <= _allowed_out(len(cases))
        assert worst > 1.0, (kind, worst)


@pytest.mark.parametrize('prec', PRECS)
def test_self_mutant_exceeds_its_bar(prec):
    worst = np.inf
    for name in D.CASES:
        c = D.case(name)
        worst = min(worst, D.mutant_self(c, prec, max(c['pmaxes'])))
    print('MUTANT %-8s self word, channel 0 with the kp of the next power: smallest change / bar %.3g' % (prec, worst))
    assert worst > 1.0
