"""
bench.py's contract: a plain run prints only the headline line, --full adds the extra legs, --dump-outputs DIR writes what the
last timed step computed (returned losses + updated weights) as float32 / float64 .npy files, at most 64 MB in all.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Model(object):
    def __init__(self, params):
        self.params = params

    def state_dict(self):
        return self.params


class _Workload(bench.Workload):
    def __init__(self, models):
        self.models = models

    def trained_models(self):
        return self.models


def test_step_outputs_names_and_dtypes():
    """The workflow's (loss, {'ce', 'nip', 'dcn'}): a part the configuration lacks (NaN placeholder) is left out; weights are
    named <model>.<parameter> with '/' -> '.'; everything is float32 unless it already is float64."""
    w = np.arange(6, dtype=np.float32).reshape(2, 3)
    wl = _Workload([('nip', _Model({'ec11/kernel': w, 'ec11/bias': np.zeros(3, np.float16)}))])
    out = bench.step_outputs(wl, (np.float32(1.5), {'ce': np.float32(0.25), 'nip': np.float64(2.0), 'dcn': np.nan}))
    assert sorted(out) == ['loss', 'loss_ce', 'loss_nip', 'nip.ec11.bias', 'nip.ec11.kernel']
    assert out['loss'].dtype == np.float32 and float(out['loss']) == 1.5
    assert out['loss_nip'].dtype == np.float64
    assert out['nip.ec11.bias'].dtype == np.float32
    assert np.array_equal(out['nip.ec11.kernel'], w)
    # a model step's dict (TwitterDCN) and a bare loss (NIPModel)
    assert sorted(bench.step_outputs(_Workload([]), {'loss': 1.0, 'ssim': np.nan, 'entropy': np.float32(3)})) == \
        ['entropy', 'loss']
    assert list(bench.step_outputs(_Workload([]), np.float32(4))) == ['loss']


def test_dump_outputs_writes_every_array(tmp_path):
    arrays = {'loss': np.asarray(1.25, np.float64), 'fan.conv1.kernel': np.linspace(0, 1, 1000, dtype=np.float32)}
    bench.dump_outputs(arrays, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['fan.conv1.kernel.npy', 'loss.npy']
    for k, v in arrays.items():
        got = np.load(str(tmp_path / (k + '.npy')))
        assert got.dtype == v.dtype and np.array_equal(got, v)


def test_dump_outputs_samples_a_larger_output_the_same_way_every_time(tmp_path):
    """Above the limit every array keeps the same share, at seeded positions: two dumps of the same arrays are identical and
    stay under the limit."""
    rng = np.random.default_rng(3)
    arrays = {'a': rng.random(600000).astype(np.float32), 'b': rng.random(200000), 's': np.asarray(7.0, np.float32)}
    limit = 3 << 20                                            # 4 MB of data against 3 MB - 1 MB usable
    for d in ('one', 'two'):
        bench.dump_outputs(arrays, str(tmp_path / d), limit=limit)
    size = sum(os.path.getsize(str(tmp_path / 'one' / f)) for f in os.listdir(str(tmp_path / 'one')))
    assert size <= limit
    for k in arrays:
        one, two = np.load(str(tmp_path / 'one' / (k + '.npy'))), np.load(str(tmp_path / 'two' / (k + '.npy')))
        assert np.array_equal(one, two) and one.dtype == arrays[k].dtype
        assert np.isin(one, arrays[k]).all()
    assert np.load(str(tmp_path / 'one' / 's.npy')) == 7.0
    assert 0 < np.load(str(tmp_path / 'one' / 'a.npy')).size < 600000


def test_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True,
                         timeout=120, check=True).stdout
    assert '--full' in out and '--dump-outputs' in out and '--steps' in out


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run (small batch): exactly the headline keys - no leg of --full - and the dump of its last step: the losses it
    returned and the updated UNet / FAN weights, finite, float32."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    d = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--batch', '32', '--dump-outputs', str(d)],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['steps'] == 3 and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['unit'] == 'patches/s' and line['higher_is_better'] is True and line['dtype'] == 'bf16'
    for extra in ('roofline', 'roofline_f32', 'cpu_baseline', 'f32_mode_patches_per_s', 'parity_fan_accuracy_bf16',
                  'c2_patches_per_s', 'dp1_nccl_ms_per_step'):
        assert extra not in line, extra
    files = sorted(os.listdir(str(d)))
    assert 'loss.npy' in files and 'loss_ce.npy' in files and 'loss_nip.npy' in files
    assert any(f.startswith('nip.') for f in files) and any(f.startswith('fan.') for f in files)
    total = 0
    for f in files:
        a = np.load(str(d / f))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    assert abs(float(np.load(str(d / 'loss.npy'))) - line['config']['loss']) <= 1e-6 * max(1.0, abs(line['config']['loss']))
