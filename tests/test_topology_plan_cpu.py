"""What admp_set_topology derives from the frame definitions (admp_amd/csrc/topology_plan.h `topology_plan`) without a GPU:
the header compiled by the host compiler into a stand-alone program (tests/topology_shim/main.cpp) against the Python
restatement the GPU tests of the closing kernels trust, tests/site_ref.py `group_layout`, plus a restatement of grp_of.
Array for array: inv_ptr, inv_idx, grp_ptr, rows_blk, gath_blk, grp_of.  The same program runs under the address and
undefined-behaviour sanitizers; two wrong restatements show that the comparison can fail."""
import shutil
import subprocess

import numpy as np
import pytest

from tests import site_ref as S
from tests.test_md_random_cpu import CSRC, ROOT

SHIM = ROOT + '/tests/topology_shim/main.cpp'
NAMES = ('inv_ptr', 'inv_idx', 'grp_ptr', 'rows_blk', 'gath_blk', 'grp_of')
CONSTANTS = (S.MAX_GROUP, S.FINISH_BLOCK, S.GATHER_RUN)      # kMaxGroup, kFinishBlock, kGatherRun of launch.h (checked below)
RULES = (S.ZTHENX, S.BISECTOR, S.ZBISECT, S.THREEFOLD, S.ZONLY, S.NOAXIS)


def restated(at, ai, groups_on=True):
    lay = S.group_layout(at, ai)
    n = len(at)
    out = dict(inv_ptr=np.concatenate([[0], np.cumsum([len(v) for v in lay['inv']])]).astype(int).tolist(),
               inv_idx=[i for v in lay['inv'] for i in v], grp_ptr=[], rows_blk=[], gath_blk=[], grp_of=[])
    if lay['groups'] is not None and groups_on:
        gp = [int(g) for g in lay['groups']]
        gof = [0] * n
        for a0, a1 in zip(gp[:-1], gp[1:]):
            for a in range(a0, a1):
                gof[a] = (a0 << 2) | (a1 - a0 - 1)      # first atom of the group, its size - 1 in the low two bits
        out.update(grp_ptr=gp, rows_blk=[int(b) for b in lay['rows_blk']], gath_blk=[int(b) for b in lay['gath_blk']], grp_of=gof)
    return out


def groups(sizes, rule=None, rng=None):
    """Consecutive groups of the given sizes.  rule: every atom takes it, its axis atoms the next atoms of its group in cyclic
    order (-1 where the group has no more); rng: a rule per atom, axis atoms drawn from the group, some slots left empty."""
    at, ai, a0 = [], [], 0
    for s in sizes:
        for m in range(s):
            others = [a0 + (m + k) % s for k in range(1, s)]
            if rng is not None:
                rng.shuffle(others)
                others = [o if rng.random() > 0.15 else -1 for o in others]
            at.append(rule if rng is None else int(rng.choice(RULES)))
            ai.append((others + [-1, -1, -1])[:3])
        a0 += s
    return np.array(at, dtype=np.int32), np.array(ai, dtype=np.int32).reshape(-1, 3)


def fixed_cases():
    cases = {}
    for rule in RULES:
        for s in (1, 2, 3, 4):
            cases['rule%d_size%d' % (rule, s)] = groups([s] * 5, rule)
        cases['rule%d_sizes' % rule] = groups([1, 2, 3, 4, 4, 3, 2, 1], rule)
    cases['component_of_5'] = groups([4, 5, 4], S.ZONLY)
    cases['component_of_5_alone'] = groups([5], S.ZTHENX)
    at, ai = groups([1, 1, 1, 2], S.ZONLY)
    at[2], ai[2, 0] = S.ZONLY, 0                         # atoms 0 and 2 in one frame, atom 1 between them
    cases['not_consecutive'] = (at, ai)
    at, ai = groups([2, 2, 1], S.ZONLY)
    at[4], ai[4, 0] = S.ZONLY, 0                         # the last atom uses an atom of the first, already closed run
    cases['earlier_run'] = (at, ai)
    at, ai = groups([1] * 9, S.NOAXIS)
    at[1:], ai[1:, 0] = S.ZONLY, 0                       # atom 0 in 8 frames besides its own
    cases['atom_in_8_frames'] = (at, ai)
    for n in (1, 7, 300):
        cases['no_axis_n%d' % n] = groups([1] * n, S.NOAXIS)
    cases['one_atom_with_a_rule'] = groups([1], S.ZTHENX)
    # a group across the ends of the runs of rows_blk and gath_blk: singles up to the boundary, then the group
    for bound in (S.FINISH_BLOCK, S.GATHER_RUN):
        for lead in range(bound - 6, bound + 3):
            for s in (2, 3, 4):
                cases['bound%d_lead%d_size%d' % (bound, lead, s)] = groups([1] * lead + [s] + [3, 4, 1], S.BISECTOR)
        for n in (bound - 1, bound, bound + 1):
            for s in (2, 3, 4):
                sizes = [s] * (n // s) + ([n % s] if n % s else [])
                cases['n%d_size%d' % (n, s)] = groups(sizes, S.ZTHENX)
    for name in S.CASES:
        c = S.case(name)
        cases['site_ref_' + name] = (np.asarray(c['axis_type'], dtype=np.int32), np.asarray(c['axis_indices'], dtype=np.int32))
    return cases


def random_cases(count=300, seed=20251):
    rng = np.random.default_rng(seed)
    cases = {}
    for k in range(count):
        na = int(rng.integers(1, 301))
        sizes = []
        while sum(sizes) < na:
            sizes.append(min(int(rng.choice((1, 2, 3, 4, 4, 4, 5) if k % 7 == 0 else (1, 2, 3, 4))), na - sum(sizes)))
        at, ai = groups(sizes, rng=rng)
        if k % 5 == 0 and na > 6:                          # a frame that reaches out of its molecule
            i = int(rng.integers(0, na))
            at[i], ai[i, 0] = S.ZONLY, int(rng.integers(0, na))
        cases['random%d' % k] = (at, ai)
    return cases


def build(tmp_path_factory, name, flags):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the header cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, '-o', exe, SHIM] + flags)
    return exe


def run_cases(exe, cases, groups_on=True):
    """{name: {array name: list}} of the program for the topologies in `cases`"""
    text = ['%d %d %d' % CONSTANTS]
    for at, ai in cases.values():
        text.append('%d %d' % (len(at), int(groups_on)))
        text.extend('%d %d %d %d' % (t, z, x, y) for t, (z, x, y) in zip(at, ai))
    lines = subprocess.run([exe], input='\n'.join(text) + '\n', capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(NAMES) * len(cases)
    out = {}
    for k, name in enumerate(cases):
        out[name] = {}
        for j, arr in enumerate(NAMES):
            v = [int(x) for x in lines[len(NAMES) * k + j].split()]
            assert v[0] == len(v) - 1
            out[name][arr] = v[1:]
    return out


def mismatches(got, cases, groups_on=True):
    bad = []
    for name, (at, ai) in cases.items():
        want = restated(at, ai, groups_on)
        bad += [(name, arr) for arr in NAMES if got[name][arr] != want[arr]]
    return bad


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    return build(tmp_path_factory, 'topology_shim', ['-O2'])


@pytest.fixture(scope='module')
def cases():
    return dict(fixed_cases(), **random_cases())


@pytest.fixture(scope='module')
def outputs(shim, cases):
    return run_cases(shim, cases)


def test_the_constants_are_the_kernels():
    text = open(CSRC + '/launch.h').read()
    for line in ('constexpr int kMaxGroup = %d;' % S.MAX_GROUP, 'constexpr int kFinishBlock = %d;' % S.FINISH_BLOCK,
                 'constexpr int kGatherRun = %d;' % S.GATHER_RUN):
        assert line in text, line
    assert CONSTANTS == (4, 256, 32)


def test_every_array_against_the_restatement(outputs, cases):
    assert len(cases) > 400
    assert mismatches(outputs, cases) == []


def test_the_cases_hold_what_they_are_there_for(outputs, cases):
    for rule in RULES:
        for s in (1, 2, 3, 4):
            o = outputs['rule%d_size%d' % (rule, s)]
            # (NoAxis atoms are groups of their own; so are the atoms of a "group" of one)
            want = s if rule != S.NOAXIS else 1
            assert o['grp_ptr'] == list(range(0, 5 * s + 1, want)), (rule, s)
            assert [g & 3 for g in o['grp_of']] == [want - 1] * (5 * s)
    for name in ('component_of_5', 'component_of_5_alone', 'not_consecutive', 'earlier_run', 'atom_in_8_frames'):
        o = outputs[name]
        assert o['grp_ptr'] == o['rows_blk'] == o['gath_blk'] == o['grp_of'] == [], name
        assert len(o['inv_ptr']) == len(cases[name][0]) + 1
    o = outputs['atom_in_8_frames']
    assert o['inv_ptr'][:2] == [0, 9] and o['inv_idx'][:9] == list(range(9))
    o = outputs['no_axis_n300']
    assert o['inv_idx'] == list(range(300)) and o['grp_ptr'] == list(range(301)) and o['rows_blk'] == [0, 256, 300]
    for name in ('no_axis_n1', 'one_atom_with_a_rule'):
        assert outputs[name] == dict(inv_ptr=[0, 1], inv_idx=[0], grp_ptr=[0, 1], rows_blk=[0, 1], gath_blk=[0, 1], grp_of=[0])
    # a run ends before the group that would not fit into it
    for bound, arr in ((S.FINISH_BLOCK, 'rows_blk'), (S.GATHER_RUN, 'gath_blk')):
        for s in (2, 3, 4):
            for lead in range(bound - 6, bound + 3):
                starts = np.concatenate([[0], np.cumsum([1] * lead + [s, 3, 4, 1])])
                first = next(int(a) for a, b in zip(starts[:-1], starts[1:]) if b > bound)      # the first group that ends beyond
                assert outputs['bound%d_lead%d_size%d' % (bound, lead, s)][arr][1] == first, (bound, s, lead)
                if bound - s < lead < bound:
                    assert first == lead                   # ... is the group across the boundary
    # the layouts tests/test_site_ref_cpu.py asserts of the restatement
    assert outputs['site_ref_groups4_n260']['rows_blk'] == [0, 256, 260]
    assert outputs['site_ref_groups3_n258']['rows_blk'] == [0, 255, 258]
    assert outputs['site_ref_n257']['rows_blk'] == [0, 255, 257]
    assert outputs['site_ref_hub_n18']['grp_ptr'] == []
    some = [outputs['random%d' % k]['grp_ptr'] != [] for k in range(300)]
    assert 60 < sum(some) < 290                            # the random topologies are of both kinds


def test_groups_switched_off(shim, cases):
    sub = {k: cases[k] for k in list(cases)[::9]}
    got = run_cases(shim, sub, groups_on=False)
    assert mismatches(got, sub, groups_on=False) == []
    assert all(got[k][arr] == [] for k in sub for arr in NAMES[2:])


def test_wrong_restatements_are_told_apart(outputs, cases, monkeypatch):
    # a run closed at `>` instead of `>=` kMaxGroup takes components of five atoms for groups
    monkeypatch.setattr(S, 'MAX_GROUP', S.MAX_GROUP + 1)
    bad = mismatches(outputs, cases)
    assert ('component_of_5', 'grp_ptr') in bad and ('component_of_5_alone', 'grp_of') in bad
    monkeypatch.undo()
    assert mismatches(outputs, cases) == []
    monkeypatch.setattr(S, 'FINISH_BLOCK', 257)            # rows_blk cut at 257
    bad = mismatches(outputs, cases)
    assert bad and {arr for _, arr in bad} == {'rows_blk'}
    assert ('site_ref_n257', 'rows_blk') in bad and ('no_axis_n300', 'rows_blk') in bad


def test_under_the_sanitizers(tmp_path_factory, cases):
    exe = build(tmp_path_factory, 'topology_shim_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    assert mismatches(run_cases(exe, cases), cases) == []
