"""No GPU: the cases, the reference, the float32 floors and the expected launch forms of tests/site_ref.py, which
tests/test_gpu_site_close.py holds the site table and the closing kernels to.

* every case builds and meets its conditioning; the edges each case is there for are really in it;
* the reference agrees with the host-compiled kernel arithmetic (tests/hostshim shim_frames at prec 8) within the bars
  tests/test_kernel_math_cpu.py uses for this comparison: frames 1e-12, Q_global and dQ_local 1e-10, grad 1e-9 -- and the
  gradient scattered from the per-frame contributions of the extended system is the autograd gradient of the system as it is;
* the float32 floors (shim_frames at prec 4 on the potential formed in float32) are finite and at most 1e-5: with the
  conditioning of site_ref they measure 1e-7 .. 3e-6 (grad), 2e-7 (dQ), 7e-7 (Q_global), 2e-6 (virial);
* the frame virial is minus the derivative of L under a cell strain at fixed positions (central differences);
* the launch forms and run counts admp_site_close must report, from the topology by the rules of admp_set_topology;
* a reference with one term wrong is further from the true one than ten times the bar (test_sensitivity)."""
import numpy as np
import pytest

from tests import site_ref as S


@pytest.mark.parametrize('name', S.CASES)
def test_case_builds_and_is_well_conditioned(name):
    c = S.case(name)
    q = S.check_conditioning(c['pos'], c['box'], c['axis_type'], c['axis_indices'])
    frac = c['pos'] @ np.linalg.inv(c['box'])
    assert frac.min() >= 0.0 and frac.max() < 1.0 + 1e-12                      # wrapped into the cell
    assert c['pot_in'].shape == (c['n'], 9) and np.isfinite(c['pot_in']).all()
    free = c['axis_type'] == S.NOAXIS
    assert not c['Q_local'][free, 1:].any()
    if not name.startswith('mixed_n760'):      # (there one workgroup of the site pass is all polarizable, its axis-free sites included)
        assert c['mono'][free].all()
    if q['angles'].size:
        print('%-20s n %4d angles %.1f .. %.1f bonds %.2f .. %.2f' % (name, c['n'], q['angles'].min(), q['angles'].max(),
                                                                      q['bonds'].min(), q['bonds'].max()))


def test_cases_hold_the_edges_they_are_there_for():
    for name in ('rules_ortho', 'rules_tric', 'rules_noise', 'rules_ortho_unused'):
        c = S.case(name)
        assert set(c['axis_type']) == {0, 1, 2, 3, 4, 5}, name
        lay = S.group_layout(c['axis_type'], c['axis_indices'])
        sizes = np.diff(lay['groups'])
        assert (sizes == 4).sum() >= 8 and (c['axis_type'] == S.NOAXIS).sum() >= 3
        st = S.straddling(c)
        grp = np.searchsorted(lay['groups'], np.arange(c['n']), side='right') - 1
        share = len(set(grp[st])) / float((sizes > 1).sum())
        assert 0.2 <= share <= 0.6, (name, share)
    assert not np.allclose(S.case('rules_tric')['box'], np.diag(np.diag(S.case('rules_tric')['box'])))
    for name in ('n31', 'n33', 'n255', 'n257', 'mixed_n760'):
        lay = S.group_layout(S.case(name)['axis_type'], S.case(name)['axis_indices'])
        assert set(np.diff(lay['groups'])) == {1, 2, 3, 4}, name
    for name, n in (('n1', 1), ('n4', 4), ('n31', 31), ('n32', 32), ('n33', 33), ('n255', 255), ('n256', 256), ('n257', 257)):
        assert S.case(name)['n'] == n
    assert S.case('n31')['n'] < S.E_WORDS < S.case('n255')['n']
    # the unused slots point outside the site's group and outside its runs, at atoms of the same system
    for uname, cname in S.UNUSED_OF.items():
        c, u = S.case(cname), S.case(uname)
        lay = S.group_layout(u['axis_type'], u['axis_indices'])
        where = lambda blk: np.searchsorted(blk, np.arange(u['n']), side='right') - 1      # noqa: E731
        grp, run, row = where(lay['groups']), where(lay['gath_blk']), where(lay['rows_blk'])
        use = S.used_slots(u['axis_type'])
        far = 0
        for i in range(u['n']):
            for k in range(3):
                if not use[i, k] and u['axis_type'][i] != S.NOAXIS:
                    j = u['axis_indices'][i, k]
                    assert c['axis_indices'][i, k] == -1 and 0 <= j < u['n'] and grp[j] != grp[i] and run[j] != run[i]
                    assert len(lay['rows_blk']) == 2 or row[j] != row[i]
                    far += 1
                else:
                    assert u['axis_indices'][i, k] == c['axis_indices'][i, k]
        assert far >= 20
        for k in ('pos', 'Q_local', 'pot_in', 'U', 'pol'):
            assert np.array_equal(c[k], u[k])
    # polarizable mix by workgroup of k_prepare_sites
    c = S.case('mixed_n760')
    act = c['pol'] > 0
    assert not act[:256].any() and act[256:512].all() and 0.4 < act[512:].mean() < 0.8
    # the states next to charge-only, each present and none of them marked
    seen = np.zeros(4, dtype=bool)
    for name in S.CASES:
        c = S.case(name)
        bare = (np.abs(c['Q_local'][:, 1:]).max(1) == 0)
        framed = c['axis_type'] != S.NOAXIS
        seen |= [(bare & framed & c['mono']).any(), (bare & (c['pol'] > 0) & ~c['mono']).any(),
                 (bare & (c['pol'] == 0) & (np.abs(c['U']).max(1) > 0) & ~c['mono']).any(), (~bare & (c['pol'] == 0) & ~c['mono']).any()]
    assert seen.all(), seen
    assert not S.straddling(S.case('inside_n33')).any()
    # the hub: more than four frames meet on one atom, one frame reaches 5 places
    c = S.case('hub_n18')
    lay = S.group_layout(c['axis_type'], c['axis_indices'])
    assert lay['groups'] is None and max(len(v) for v in lay['inv']) >= 7
    assert np.abs(c['axis_indices'][3] - 3).max() == 5


@pytest.mark.parametrize('name', S.CASES)
def test_reference_matches_host_arithmetic_and_floors_are_small(name):
    c = S.case(name)
    ref = S.reference(name, 'double')
    tab = S.site_table_ref(c)
    got = S.shim_frames(c, 8, ref['P'])
    keep = c['axis_type'] != S.NOAXIS
    np.testing.assert_allclose(got['frames'][keep], tab['frames'][keep], atol=1e-12)
    np.testing.assert_allclose(got['Qg'], tab['Q'], atol=1e-10)
    np.testing.assert_allclose(got['Qg'], ref['Qg'], atol=1e-10)
    np.testing.assert_allclose(got['grad'], ref.get('grad_frames', ref['grad']), atol=1e-9)
    np.testing.assert_allclose(got['dQ'], ref['dQ'], atol=1e-10)
    free = c['axis_type'] == S.NOAXIS
    assert np.array_equal(ref['dQ'][free], ref['P'][free])
    # the scatter of the per-frame contributions is the gradient of the system as it is
    if c['n'] > 1:      # (the oracle points the unused slots of a site at the next atom: a single atom has none)
        direct = S.direct_grad(c, ref['P'])
        np.testing.assert_allclose(ref.get('grad_frames', ref['grad']), direct, atol=1e-10 * max(1.0, np.abs(direct).max()))
    else:
        assert not ref['grad'].any()
    ext = S.shim_frames(c, 8, ref['P'], extended=True)
    for a, b in zip(ext['parts'], ref['parts']):
        np.testing.assert_allclose(a, b, atol=1e-9)
    fl = S.floors(name)
    print('%-20s f32 floors: %s' % (name, ' '.join('%s %.2e' % kv for kv in fl.items())))
    for k in ('grad', 'dQ', 'Qg', 'vir'):
        assert np.isfinite(fl[k]) and fl[k] <= S.F32_FLOOR_CAP, (name, k, fl[k])
    assert np.isfinite(fl['E_self']) and np.isfinite(fl['E_pen'])
    assert fl['E_self'] <= 1e-5 * max(1.0, abs(ref['E_self'])) and fl['E_pen'] <= 1e-5 * max(1.0, abs(ref['E_pen']))


@pytest.mark.parametrize('name', ['rules_ortho', 'rules_tric', 'n33', 'inside_n33'])
def test_frame_virial_is_the_strain_derivative(name):
    c = S.case(name)
    ref = S.reference(name)
    h = 1e-6
    fd = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            eps = np.zeros((3, 3))
            eps[a, b] = h
            fd[a, b] = (S.frame_energy(c, ref['P'], box=c['box'] @ (np.eye(3) + eps)) -
                        S.frame_energy(c, ref['P'], box=c['box'] @ (np.eye(3) - eps))) / (2 * h)
    scale = max(np.abs(ref['vir']).max(), np.abs(ref['grad']).max())
    assert np.abs(fd + ref['vir']).max() <= 1e-6 * scale, (fd, ref['vir'])
    if name == 'inside_n33':
        assert not ref['vir'].any()
    else:
        assert np.abs(ref['vir']).max() > 0.1


def test_expected_forms_and_run_counts():
    E = S.expected_info
    c = S.case('groups4_n260')       # 65 groups of 4: 64 fill run 0 exactly, 8 fill a run of the gather exactly
    assert E(c, 'rows') == dict(form='rows', ngroups=65, nrowblk=2, rows_grid=2)
    assert E(c, 'rows', rows_grid=1) == dict(form='rows', ngroups=65, nrowblk=2, rows_grid=1)
    assert E(c, 'gather') == dict(form='gather_epilogue', ngathblk=9)
    assert list(S.group_layout(c['axis_type'], c['axis_indices'])['rows_blk']) == [0, 256, 260]
    c = S.case('groups3_n258')       # 86 groups of 3: run 0 ends at 255, a run of the gather at 30
    lay = S.group_layout(c['axis_type'], c['axis_indices'])
    assert list(lay['rows_blk']) == [0, 255, 258] and list(lay['gath_blk'][:3]) == [0, 30, 60]
    assert E(c, 'groups') == dict(form='groups', ngroups=86, nrowblk=2, rows_grid=0)
    c = S.case('mixed_n760')
    lay = S.group_layout(c['axis_type'], c['axis_indices'])
    assert len(lay['rows_blk']) == 4 and (np.diff(lay['rows_blk']) <= 256).all() and np.diff(lay['rows_blk'])[0] < 256
    assert [E(c, 'rows', rows_grid=g)['rows_grid'] for g in (1024, 2, 1, 0, 5000)] == [3, 2, 1, 1, 3]
    assert E(c, 'pull') == dict(form='pull4', ngroups=len(lay['groups']) - 1, nrowblk=3, rows_grid=0)
    assert E(c, 'pull', lanes4=False)['form'] == 'pull1'
    assert E(c, 'rows', groups_on=False) == dict(form='pull4', ngroups=0, nrowblk=0, rows_grid=0)
    assert E(c, 'gather', groups_on=False) is None
    for name, nrow, ngath in (('n1', 1, 1), ('n4', 1, 1), ('n31', 1, 1), ('n32', 1, 1), ('n33', 1, 2), ('n255', 1, 9), ('n256', 1, 9),
                              ('n257', 2, 9)):
        c = S.case(name)
        assert E(c, 'rows')['nrowblk'] == nrow and E(c, 'gather')['ngathblk'] == ngath, name
    # the last partial run, and a run that ends early because the next group would not fit
    lay = S.group_layout(S.case('n257')['axis_type'], S.case('n257')['axis_indices'])
    assert list(lay['rows_blk']) == [0, 255, 257]
    lay = S.group_layout(S.case('n33')['axis_type'], S.case('n33')['axis_indices'])
    assert 28 < lay['gath_blk'][1] < 32
    # unused slots do not change the grouping; the hub has no groups at all
    assert E(S.case('rules_ortho_unused'), 'rows') == E(S.case('rules_ortho'), 'rows')
    assert E(S.case('mixed_n760_unused'), 'rows', rows_grid=2) == E(S.case('mixed_n760'), 'rows', rows_grid=2)
    assert E(S.case('rules_ortho_unused'), 'gather') == E(S.case('rules_ortho'), 'gather') == dict(form='gather_epilogue', ngathblk=2)
    c = S.case('hub_n18')
    assert E(c, 'rows') == E(c, 'groups') == E(c, 'pull') == dict(form='pull4', ngroups=0, nrowblk=0, rows_grid=0)
    assert E(c, 'gather') is None


CATCHES = {       # perturbation -> the cases that must catch it
    'drop_y': ('rules_ortho', 'rules_tric', 'groups4_n260'),             # ThreeFold and ZBisect sites
    'drop_mate_at_run_boundary': ('groups4_n260', 'groups3_n258'),       # atom 255 / 254 closes run 0 inside a full group
    'swap_xy': ('rules_ortho', 'rules_tric'),
    'self_from_Q': ('rules_ortho', 'mixed_n760', 'hub_n18'),             # polarizable sites with a dipole
    'run_shifted': ('mixed_n760',),                                      # a run 1 of more than one group
    'lane3_dropped': ('groups4_n260', 'hub_n18'),                        # centres of groups of 4; the hub (frames 3 and 7)
}


@pytest.mark.parametrize('what', S.PERTURBATIONS)
def test_sensitivity(what):
    """A reference with one term wrong must differ from the true one by more than ten times the widest bar an output is held
    to (float32: FLOOR_FACTOR x the host floor, relative to the array's largest entry), on every case listed in CATCHES:
    drop_y (the y-atom term of ThreeFold / ZBisect) and swap_xy on the axis-rules cases; drop_mate_at_run_boundary on the
    uniform groups, where the last atom of run 0 sits inside a full group; self_from_Q wherever dipoles are; run_shifted on
    the cases whose run 1 holds several groups; lane3_dropped where an atom takes part in four frames or more."""
    for name in CATCHES[what]:
        ref = S.reference(name)
        bars = S.single_bars(name)
        p = S.perturbed(name, what)
        d = S.rel_err(p['grad'], ref['grad'])
        print('%-26s %-14s grad moves by %.3g, bar %.3g' % (what, name, d, bars['grad']))
        assert d > 10.0 * bars['grad'], (what, name, d, bars['grad'])
        if what == 'self_from_Q':
            assert S.rel_err(p['dQ'], ref['dQ']) > 10.0 * bars['dQ']
            assert abs(p['E_self'] - ref['E_self']) > 10.0 * bars['E_self']
