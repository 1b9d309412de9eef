"""GPU: bench.py's plain run - the headline steps and nothing after them - and --dump-outputs (the timed step run once more from the
seeded starting state, its outputs as .npy files that agree from run to run with the same arguments, so that two builds can be
compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ['--batch', '8', '--T', '32', '--L', '8', '--C', '5', '--vdim', '256', '--steps', '6', '--warmup', '2', '--prewarm', '2']
NAMES = ['end_index', 'end_logits', 'loss', 'loss_terms', 'match_scores', 'params', 'start_index', 'start_logits']


def _run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + ARGS + ['--dump-outputs', out_dir],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_steps_only_and_dumps_its_outputs(tmp_path):
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    out = _run(a)
    assert out['metric'] == 'train clips/sec' and out['unit'] == 'clips/s' and out['higher_is_better'] is True
    assert out['steps'] == 6 and out['ms_per_step'] > 0 and out['value'] > 0 and out['dtype']
    assert out['roofline'] is None and out['cpu_baseline'] is None          # the legs after the timed region run with --full only
    for k in ('other_feature_dtype', 'forward_only', 'host_fed', 'epoch_loop', 'epoch_loop_anet', 'rccl', 'legs_cut_short'):
        assert k not in out
    assert sorted(f[:-4] for f in os.listdir(a)) == NAMES
    arrays = {n: np.load(os.path.join(a, n + '.npy')) for n in NAMES}
    assert sum(x.nbytes for x in arrays.values()) <= 64 << 20
    for n, x in arrays.items():
        assert x.dtype in (np.float32, np.float64) and np.all(np.isfinite(x)), n
    assert arrays['start_logits'].shape == (8, 32) and arrays['match_scores'].shape == (8, 32, 4) and arrays['end_index'].shape == (8,)
    assert np.all(arrays['start_index'] <= arrays['end_index'])
    assert np.isclose(arrays['loss'][0], arrays['loss_terms'][0], rtol=1e-6)
    # the same arguments give the same inputs: a second run computes the same forward bit for bit, and parameters
    # that differ at most where a gradient summed with float atomics has a rounding-noise sign: one Adam step, ~3.2 x lr = 3.2e-4
    _run(b)
    again = {n: np.load(os.path.join(b, n + '.npy')) for n in NAMES}
    for n in ('start_logits', 'end_logits', 'match_scores', 'start_index', 'end_index'):
        np.testing.assert_array_equal(again[n], arrays[n], err_msg=n)
    np.testing.assert_allclose(again['loss_terms'], arrays['loss_terms'], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(again['params'], arrays['params'], rtol=0, atol=1e-3)
