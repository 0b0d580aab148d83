"""The predictor-corrector arithmetic of the engine without a GPU (admp_amd/csrc/scf_aspc.h): a stand-alone host program
(tests/aspc_shim/main.cpp) prints the coefficient table and drives the ring of dipole sets; the table is checked against
Kolafa's closed formula in exact fractions, the ring against a list."""
import shutil
import subprocess
from fractions import Fraction
from math import comb

import pytest

from tests.test_md_random_cpu import CSRC, ROOT

SHIM = ROOT + '/tests/aspc_shim/main.cpp'
ORDERS = (0, 1, 2, 3, 4)
# the issue's table, typed in once more
TABLE = {0: ('2', '-1', '2/3'), 1: ('5/2', '-2', '1/2', '3/5'), 2: ('14/5', '-14/5', '6/5', '-1/5', '4/7'),
         3: ('3', '-24/7', '27/14', '-4/7', '1/14', '5/9'), 4: ('22/7', '-55/14', '55/21', '-22/21', '5/21', '-1/42', '6/11')}


def closed_B(k, j):
    return Fraction((-1) ** (j + 1) * j * comb(2 * k + 4, k + 2 - j), comb(2 * k + 2, k + 1))


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ not found: the header cannot be checked on the host')
    exe = str(tmp_path_factory.mktemp('aspc_shim') / 'aspc_shim')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, '-o', exe, SHIM])
    return exe


@pytest.fixture(scope='module')
def table(shim):
    out = subprocess.run([shim, 'table'], capture_output=True, text=True, check=True).stdout.strip().split('\n')
    rows = {}
    for line in out[:-1]:
        w = line.split()
        rows[int(w[0])] = ([Fraction(x) for x in w[1:-2]], Fraction(w[-2]), float(w[-1]))
    assert out[-1].split() == ['limits', '4', '6', '6']
    return rows


def script(shim, text):
    return subprocess.run([shim, 'script'], input=text, capture_output=True, text=True, check=True).stdout.strip().split('\n')


def state(line):
    head, _, tags = line.partition('|')
    w = head.split()
    return dict(on=int(w[0]), order=int(w[1]), n_corrector=int(w[2]), omega=float(w[3]), slots=int(w[4]), count=int(w[5]),
                full=int(w[6]), next_slot=int(w[7]), tags=[int(t) for t in tags.split()])


def test_table_equals_the_closed_formula(table):
    assert sorted(table) == list(ORDERS)
    for k in ORDERS:
        B, omega, omega_f = table[k]
        assert B == [closed_B(k, j) for j in range(1, k + 3)], k
        assert omega == Fraction(k + 2, 2 * k + 3) and omega_f == (k + 2) / (2 * k + 3)
        assert B + [omega] == [Fraction(x) for x in TABLE[k]], k


def test_coefficients_sum_to_one(table):
    for k in ORDERS:
        assert sum(table[k][0]) == 1


@pytest.mark.parametrize('k', ORDERS)
def test_predictor_reproduces_a_linear_sequence(shim, table, k):
    """exactly in fractions with the table's numbers; to rounding in the double accumulation of the kernel's order"""
    B = table[k][0]
    for a, b in ((Fraction(3, 7), Fraction(-5, 11)), (Fraction(0), Fraction(1)), (Fraction(-2), Fraction(0))):
        n = 17
        assert sum(B[j - 1] * (a + b * (n - j)) for j in range(1, k + 3)) == a + b * n
    a, b, n = 0.3712, -0.0179, 9
    hist = ' '.join('%.17g' % (a + b * (n - j)) for j in range(1, k + 3))
    got = float(subprocess.run([shim, 'predict', str(k)], input=hist, capture_output=True, text=True, check=True).stdout)
    mags = sum(abs(float(B[j - 1])) * abs(a + b * (n - j)) for j in range(1, k + 3))
    assert abs(got - (a + b * n)) <= (k + 4) * 2.0 ** -52 * mags      # one rounding per product, per sum and per coefficient


@pytest.mark.parametrize('k', [0, 4])
def test_ring_order_across_wrap_arounds(shim, k):
    """after every push slot(j) holds the set pushed j calls ago, through four turns of the ring; a set never lands in a
    slot that a stored set within reach of the predictor occupies, except the oldest one of a full ring"""
    n_push = 4 * (k + 2) + 3
    text = 'cfg %d 1 0\nstate\n' % k + ''.join('push %d\nstate\n' % (100 + n) for n in range(n_push))
    out = script(shim, text)
    assert out[0] == 'ok'
    s = state(out[1])
    assert (s['on'], s['order'], s['slots'], s['count'], s['full'], s['tags']) == (1, k, k + 2, 0, 0, [])
    used = []
    for n in range(n_push):
        slot, s = int(out[2 + 2 * n]), state(out[3 + 2 * n])
        used.append(slot)
        want = [100 + n - j for j in range(0, min(n + 1, k + 2))]
        assert s['tags'] == want, (n, s)
        assert s['count'] == min(n + 1, k + 2) and s['full'] == int(n + 1 >= k + 2)
        assert 0 <= slot < k + 2 and 0 <= s['next_slot'] < k + 2
    assert used == [n % (k + 2) for n in range(n_push)]      # round robin from slot 0


def test_drop_and_refill(shim):
    text = ('cfg 1 2 0.5\npush 1\npush 2\npush 3\npush 4\nstate\ndrop\nstate\npush 7\nstate\npush 8\npush 9\nstate\n'
            'cfg 1 2 0.5\nstate\npush 5\nstate\ncfg -1 1 0\nstate\n')
    out = script(shim, text)
    assert out[0] == 'ok'
    s = state(out[5])
    assert s['tags'] == [4, 3, 2] and s['full'] == 1 and s['omega'] == 0.5 and s['n_corrector'] == 2
    s = state(out[6])      # drop keeps the mode
    assert (s['on'], s['order'], s['n_corrector'], s['omega'], s['count'], s['full'], s['tags']) == (1, 1, 2, 0.5, 0, 0, [])
    assert state(out[8])['tags'] == [7] and state(out[8])['full'] == 0
    assert state(out[11])['tags'] == [9, 8, 7] and state(out[11])['full'] == 1
    assert out[12] == 'ok' and state(out[13])['count'] == 0          # the same values again: the history goes
    assert state(out[15])['tags'] == [5]
    s = state(out[17])
    assert out[16] == 'ok' and (s['on'], s['order'], s['slots'], s['count'], s['omega']) == (0, -1, 0, 0, 0.0)


def test_omega_in_effect(shim, table):
    for k in ORDERS:
        out = script(shim, 'cfg %d 1 0\nstate\ncfg %d 1 -3\nstate\ncfg %d 6 1\nstate\ncfg %d 3 0.8\nstate\n' % (k, k, k, k))
        assert out[0::2] == ['ok'] * 4
        assert [state(x)['omega'] for x in out[1::2]] == [table[k][2], table[k][2], 1.0, 0.8]
        assert [state(x)['n_corrector'] for x in out[1::2]] == [1, 1, 6, 3]


@pytest.mark.parametrize('bad', ['-2 1 0', '5 1 0', '17 1 0', '2 0 0', '2 7 0', '2 -1 0', '2 1 1.5', '2 1 1.0000001', '2 1 nan', '2 1 inf'])
def test_refusals_leave_the_ring_as_it_was(shim, bad):
    out = script(shim, 'cfg 3 2 0.75\npush 1\npush 2\nstate\ncfg %s\nstate\n' % bad)
    assert out[0] == 'ok' and out[4] == 'refused'
    assert out[5] == out[3] and state(out[5])['tags'] == [2, 1]
    # ... and an unconfigured ring stays off
    out = script(shim, 'cfg %s\nstate\n' % bad)
    assert out[0] == 'refused' and state(out[1])['on'] == 0
