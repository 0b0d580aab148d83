"""The integer planning of a slab rank's decomposition (admp_amd/csrc/slab_plan.h `slab_column_plan`, `slab_segments`) without
a GPU: the header compiled by the host compiler into a stand-alone program (tests/slab_plan_shim/main.cpp) against a Python
restatement written here.  Field by field: the number of columns, every mask / want / binned word, what each column runs over,
every c_* index, and -- from totals with zeros and a peer that counts nothing -- all counts, the four offset arrays with their
columns and the rows of the exchange buffers.  The same program runs under the address and undefined-behaviour sanitizers; two
wrong restatements show that the comparison can fail."""
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_md_random_cpu import CSRC, ROOT

SHIM = ROOT + '/tests/slab_plan_shim/main.cpp'
HOME, POLAR, MAX_RANKS = 1 << 30, 1 << 29, 28      # kSlabHome, kSlabPolar, kSlabMaxRanks (checked below)
MAX_COLS = 3 + 4 * MAX_RANKS
NA = 7                                             # the atom count the program binds its plans to
RANKS = (2, 3, 5, 8, 28)


def restated(N, me, track, bins_on, totals, skip_me=True, swap_wants=False):
    """What the program prints for this case, as {name: list of int}."""
    cols = []                                      # (mask, want, binned, seq, src)

    def col(mask, want, binned=True, seq=0, src=0):
        cols.append((mask, want, int(binned and bins_on), seq, src))
        return len(cols) - 1
    c_home = col(HOME, HOME)
    c_rows = col(HOME, HOME, binned=False, seq=1)
    c_act = col(HOME | POLAR, HOME | POLAR)
    c = {k: [-1] * MAX_RANKS for k in ('imp', 'exp', 'min', 'mout')}
    for t in range(N):
        if t == me and skip_me:
            continue
        reads, owns = (1 << t, HOME | 1 << t) if not swap_wants else (HOME | 1 << t, 1 << t)
        c['imp'][t] = col(HOME | 1 << t, reads)          # atoms of rank t that this rank reads
        c['exp'][t] = col(HOME | 1 << t, owns)           # atoms of this rank that rank t reads
        if track:
            c['min'][t] = col(HOME | 1 << t, reads, src=1)
            c['mout'][t] = col(HOME | 1 << t, owns, src=1)
    out = dict(head=[len(cols), N, N if bins_on else 0, me, c_home, c_rows, c_act], len=[NA] * len(cols))
    for k, name in enumerate(('mask', 'want', 'binned', 'seq', 'src')):
        out[name] = [x[k] for x in cols]
    total = {}
    for name in ('imp', 'exp', 'min', 'mout'):
        out['c_' + name] = c[name]
        present = [t for t in range(N) if c[name][t] >= 0]
        out[name + '_cnt'] = [totals[c[name][t]] if c[name][t] >= 0 else 0 for t in range(N)]
        out[name + '_off'] = [0] + np.cumsum([totals[c[name][t]] for t in present], dtype=int).tolist()
        out[name + '_col'] = [c[name][t] for t in present]
        total[name] = out[name + '_off'][-1]
    out['n'] = [totals[c_home], totals[c_act], total['imp'], total['exp'], total['min'], total['mout'], max(1, *total.values())]
    return out


def make_cases():
    """{(N, me, track, bins_on): totals}: totals with zeros among them; every count of one peer zero; once all of them zero"""
    rng = np.random.default_rng(20261)
    cases = {}
    for N in RANKS:
        for me in range(N):
            for track in (0, 1):
                for bins_on in (0, 1):
                    tot = rng.integers(1, 60, MAX_COLS)
                    tot[rng.random(MAX_COLS) < 0.2] = 0
                    if me == N - 1 and track:
                        tot[:] = 0
                    else:
                        quiet = (me + 1) % N                              # a peer that neither sends nor receives
                        first = 3 + (4 if track else 2) * (quiet - (1 if quiet > me else 0))
                        tot[first:first + (4 if track else 2)] = 0
                    cases[(N, me, track, bins_on)] = [int(x) for x in tot]
    return cases


def run_cases(exe, cases):
    text = ''.join('%d %d %d %d\n%s\n' % (key + (' '.join(map(str, tot)),)) for key, tot in cases.items())
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    out, it = {}, iter(lines)
    for key in cases:
        rec = {}
        for ln in it:
            w = ln.split()
            if w[0] == 'end':
                break
            if w[0] == 'refused':
                rec = ln
                break
            rec[w[0]] = [int(x) for x in w[1:]]
        out[key] = rec
    assert next(it, None) is None
    return out


def mismatches(got, cases, **wrong):
    bad = []
    for key, tot in cases.items():
        want = restated(*key, tot, **wrong)
        assert set(got[key]) == set(want)
        bad += [(key, name) for name in want if got[key][name] != want[name]]
    return bad


def build(tmp_path_factory, name, flags):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the header cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, '-o', exe, SHIM] + flags)
    return exe


@pytest.fixture(scope='module')
def cases():
    return make_cases()


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    return build(tmp_path_factory, 'slab_plan_shim', ['-O2'])


@pytest.fixture(scope='module')
def outputs(shim, cases):
    return run_cases(shim, cases)


def test_the_constants_are_the_kernels():
    text = open(CSRC + '/slab_plan.h').read()
    for line in ('constexpr int kSlabHome = 1 << 30, kSlabPolar = 1 << 29;',
                 'constexpr int kSlabMaxRanks = 28, kSlabMaxCols = 3 + 4 * kSlabMaxRanks;'):
        assert line in text, line
    assert '#include <hip' not in text and '#include "' not in text      # host code alone
    assert '#include "slab_plan.h"' in open(CSRC + '/launch.h').read()


def test_every_field_against_the_restatement(outputs, cases):
    assert len(cases) == 4 * sum(RANKS)
    assert mismatches(outputs, cases) == []


def test_the_cases_hold_what_they_are_there_for(outputs, cases):
    assert outputs[(28, 5, 1, 1)]['head'][0] == 111 <= MAX_COLS == 115
    assert outputs[(28, 5, 0, 1)]['head'][0] == 57 and outputs[(2, 0, 0, 0)]['head'][0] == 5
    for (N, me, track, bins_on), o in outputs.items():
        for name in ('c_imp', 'c_exp', 'c_min', 'c_mout'):
            present = [t for t in range(MAX_RANKS) if o[name][t] >= 0]
            assert present == ([t for t in range(N) if t != me] if track or name in ('c_imp', 'c_exp') else []), (N, me, name)
        assert sum(o['binned']) == (o['head'][0] - 1 if bins_on else 0) and o['binned'][1] == 0
        assert sum(o['seq']) == 1 and sum(o['src']) == (2 * (N - 1) if track else 0)
        quiet = (me + 1) % N
        assert all(o[k + '_cnt'][quiet] == 0 and o[k + '_cnt'][me] == 0 for k in ('imp', 'exp', 'min', 'mout'))
        assert len(o['imp_off']) == N and o['imp_off'][-1] == sum(o['imp_cnt']) == o['n'][2]
    zeros = [o for key, o in outputs.items() if not any(cases[key])]
    assert len(zeros) == 2 * len(RANKS) and all(o['n'] == [0, 0, 0, 0, 0, 0, 1] for o in zeros)
    some = [o for o in outputs.values() if 0 in o['imp_cnt'][:1] + o['exp_cnt'] and max(o['n'][2:6]) > 1]
    assert len(some) > 100                                  # zero counts next to non-zero ones
    assert any(o['n'][6] == o['n'][k] for o in outputs.values() for k in (4, 5) if o['n'][k] > max(o['n'][2:4]))


def test_29_ranks_are_refused(shim):
    key = (29, 3, 1, 1)
    assert run_cases(shim, {key: [1] * MAX_COLS, (28, 3, 1, 1): [1] * MAX_COLS})[key] == 'refused at most 28 slab ranks'


def test_wrong_restatements_are_told_apart(outputs, cases):
    bad = mismatches(outputs, cases, skip_me=False)          # a column pair for the rank itself
    assert ((3, 1, 0, 1), 'head') in bad and ((3, 1, 0, 1), 'c_imp') in bad and ((2, 0, 1, 0), 'imp_off') in bad
    bad = mismatches(outputs, cases, swap_wants=True)        # imports listed where the exports belong
    assert {name for _, name in bad} == {'want'} and len({key for key, _ in bad}) == len(cases)
    assert mismatches(outputs, cases) == []


def test_under_the_sanitizers(tmp_path_factory, cases):
    exe = build(tmp_path_factory, 'slab_plan_shim_san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    assert mismatches(run_cases(exe, cases), cases) == []
