"""bench.py on the GPU: a plain run prints the headline line without the --full legs, and --dump-outputs writes what the
timed path returned in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '2', '--dump-outputs',
                        str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['steps'] == 3 and line['warmup'] == 2 and line['ms_per_step'] > 0
    assert line['unit'] == 'ns/day' and line['higher_is_better'] is True and line['dtype'] == 'f64'
    assert abs(line['value'] - 0.0864 / (line['ms_per_step'] * 1e-3)) < 1e-3 * line['value']
    assert not {'roofline', 'kernel_ms_per_step', 'scf_tight', 'cpu_baseline', 'md_all_terms', 'at_scale'} & set(line)
    n = line['config']['n_atoms']
    E, G, U = (np.load(str(tmp_path / (k + '.npy'))) for k in ('energy', 'grad', 'U_ind'))
    assert E.shape == (1,) and G.shape == U.shape == (n, 3)
    assert E.dtype == G.dtype == U.dtype == np.float64
    assert np.isfinite(E).all() and np.isfinite(G).all() and np.isfinite(U).all() and np.abs(G).max() > 0
