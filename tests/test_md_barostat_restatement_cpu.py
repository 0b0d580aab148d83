"""The float64 restatement of the ideal-gas NPT loop (tests/test_gpu_md_barostat.py gas_restatement) without a GPU: the two
figures that test takes from it are tied to the code here.  The bar on ln V is ten times what two summation orders of sum m v^2
move it, and the analytic centre N kB T / P0 of the volume band stands only while the restatement's own mean lies inside 2.5
sigma of it."""
import numpy as np

from tests.test_gpu_md_barostat import GAS, LNV_BAR, gas_restatement, gas_start


def test_ln_v_bar_is_ten_times_the_summation_order_difference():
    d = np.abs(gas_restatement(0) - gas_restatement(1)).max()
    print('max |ln V (order 0) - ln V (order 1)| = %.3e, bar %.1e' % (d, LNV_BAR))
    assert 0.0 < 10.0 * d <= LNV_BAR <= 10.5 * d


def test_restatement_mean_volume_inside_2p5_sigma_of_the_analytic_centre():
    _, _, _, v_eq = gas_start()
    mean_v = np.exp(gas_restatement(0)[-2000:]).mean()
    sigma = 1.0 / np.sqrt(50.0 * GAS['n'])
    print('mean V / (N kB T / P0) - 1 = %+.4e = %.2f sigma' % (mean_v / v_eq - 1.0, (mean_v / v_eq - 1.0) / sigma))
    assert abs(mean_v / v_eq - 1.0) <= 2.5 * sigma
