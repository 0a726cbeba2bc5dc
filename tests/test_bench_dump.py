# -*- coding: utf-8 -*-
"""bench.py --dump-outputs: what the last timed step computed, as DIR/<name>.npy, so that two builds can be compared output
for output.  The helpers are checked on the CPU; on the GPU, two runs with the same arguments must write the same bits (the
inputs are seeded and the kernels deterministic) and the loss the JSON line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_whole_or_a_fixed_seeded_subset():
    t = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    whole = bench.dump_sample(t, 1000, 0)
    assert whole.dtype == np.float32 and np.array_equal(whole, np.arange(1000, dtype=np.float32))
    a, b = bench.dump_sample(t, 64, 3), bench.dump_sample(t, 64, 3)
    assert a.dtype == np.float32 and a.shape == (64,) and np.array_equal(a, b)
    assert len(np.unique(a)) == 64 and np.all(np.diff(a) > 0)        # distinct positions, in storage order
    assert not np.array_equal(a, bench.dump_sample(t, 64, 4))
    # logical (NCHW) order whatever the memory layout
    x = torch.randn(2, 8, 4, 4)
    assert np.array_equal(bench.dump_sample(x.to(memory_format=torch.channels_last), 10 ** 6, 0), x.reshape(-1).numpy())


def test_dump_outputs_writes_float_npy_within_budget(tmp_path):
    d = str(tmp_path / 'out')
    bench.dump_outputs(d, {'loss': np.array(1.5, np.float64), 'x': np.ones((3, 4), np.float32)})
    assert sorted(os.listdir(d)) == ['loss.npy', 'x.npy']
    loss = np.load(os.path.join(d, 'loss.npy'))
    assert loss.dtype == np.float64 and loss.shape == () and float(loss) == 1.5
    with pytest.raises(AssertionError):
        bench.dump_outputs(d, {'i': np.ones(4, np.int32)})
    with pytest.raises(AssertionError):
        bench.dump_outputs(d, {'big': np.zeros((64 << 20) // 4 + 1, np.float32)})


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--size', '64', '--batch', '2'] + list(args),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_bit_for_bit(tmp_path):
    train = ('--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--no-infer-leg')
    runs = []
    for i in range(2):
        d = str(tmp_path / f'train{i}')
        line = _bench(*train, '--dump-outputs', d)
        assert line['steps'] == 3
        runs.append((line, _load(d)))
    (line, a), (_, b) = runs
    names = ['grads', 'loss'] + [f'head{l}_{k}' for l in range(3) for k in ('output', 'pred')]
    assert sorted(a) == sorted(names)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a['grads'].shape == (bench.DUMP_GRAD_SAMPLE,) and np.isfinite(a['grads']).all() and np.abs(a['grads']).max() > 0
    assert a['head0_output'].size == 2 * 3 * 8 * 8 * 85                 # smaller than the sample: the whole tensor
    assert a['loss'].shape == () and float(a['loss']) == line['config']['loss']
    for k in names:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k

    d = str(tmp_path / 'infer')
    line = _bench('--infer', '--steps', '2', '--warmup', '1', '--dump-outputs', d)
    assert line['steps'] == 2
    got = _load(d)
    assert sorted(got) == ['detections', 'predictions']
    assert got['predictions'].dtype == np.float32 and got['predictions'].size == 2 * 3 * (8 * 8 + 4 * 4 + 2 * 2) * 85
    det = got['detections']
    assert det.dtype == np.float32 and det.ndim == 2 and det.shape[1] == 8
    assert set(np.unique(det[:, 0])) <= {0.0, 1.0}
