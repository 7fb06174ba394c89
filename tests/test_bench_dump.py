"""`bench.py --dump-outputs DIR`: the sample of the timed step's logits and masks that lets two builds be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT
from totalsegmentator2d_amd.engine import unpack_mask


def _pack(bits):
    """[.., W] {0,1} -> [.., W/32] int32, pixel w in bit w % 32 of word w // 32 (the engine's mask layout)."""
    return np.packbits(bits.astype(np.uint8), axis=-1, bitorder='little').view(np.int32)


@pytest.mark.parametrize('keep', [1 << 22, 1000])
def test_dump_is_the_flat_sample_of_logits_and_unpacked_masks(tmp_path, monkeypatch, keep):
    """Whole arrays when they fit, else sorted seeded positions - the same ones in both files and in every call."""
    import torch
    import bench
    monkeypatch.setattr(bench, 'DUMP_ELEMS', keep)
    rng = np.random.default_rng(5)
    logits = rng.standard_normal((3, 5, 8, 64)).astype(np.float32)
    bits = rng.integers(0, 2, logits.shape).astype(np.uint8)
    mask = _pack(bits)
    assert np.array_equal(unpack_mask(mask, 64), bits)
    for d in ('a', 'b'):
        bench.dump_outputs(torch, str(tmp_path / d), torch.from_numpy(logits), torch.from_numpy(mask))
    lg, mk = np.load(tmp_path / 'a' / 'logits.npy'), np.load(tmp_path / 'a' / 'mask.npy')
    assert lg.dtype == np.float32 and mk.dtype == np.float32 and lg.shape == mk.shape and lg.ndim == 1
    assert np.array_equal(lg, np.load(tmp_path / 'b' / 'logits.npy')) and np.array_equal(mk, np.load(tmp_path / 'b' / 'mask.npy'))
    if keep >= logits.size:
        assert np.array_equal(lg, logits.ravel()) and np.array_equal(mk, bits.ravel())
    else:
        assert 0.9 * keep <= lg.size <= keep                       # repeated draws are dropped
        # every dumped (logit, bit) pair is a pair of the arrays, in flat order: walk the arrays once
        pairs = iter(zip(logits.ravel(), bits.ravel()))
        for want in zip(lg, mk):
            assert any(want == (a, float(b)) for a, b in pairs), 'sample is not an ordered sub-sequence of the outputs'


def test_dump_outputs_is_refused_where_no_logits_come_back():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--workload', 'config3', '--dump-outputs', 'x'],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and '--dump-outputs' in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_in_every_run(tmp_path):
    """Two runs with the same arguments: identical inputs, hence identical files; the masks are the thresholded logits; 64 MB at most."""
    from bench import SIGMOID_HALF_THRESHOLD
    got = []
    for d in ('a', 'b'):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--no-cpu-baseline',
                            '--no-other-modes', '--dump-outputs', str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert len(lines) == 1 and json.loads(lines[0])['steps'] == 2
        files = sorted(os.listdir(tmp_path / d))
        assert files == ['logits.npy', 'mask.npy']
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= 64 << 20
        got.append([np.load(tmp_path / d / f) for f in files])
    (la, ma), (lb, mb) = got
    assert la.dtype == np.float32 and ma.dtype == np.float32 and np.isfinite(la).all()
    assert np.array_equal(la, lb) and np.array_equal(ma, mb)
    assert np.array_equal(ma, (la > SIGMOID_HALF_THRESHOLD).astype(np.float32)) and 0 < ma.mean() < 1
