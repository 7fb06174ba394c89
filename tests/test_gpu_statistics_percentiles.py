"""ts2d_label_percentiles (csrc/kernels_stats_select.h) against its statement, statistics.label_percentiles_statement, bit for bit - counts, the
float32 bits of the rank values, the float64 bits of the weights -, the chunks, the refusals, the status bit, and the device route of
statistics.label_statistics(percentiles=...) and TS2D.Result.statistics(percentiles=...)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, engine, image, nrrd, statistics as S
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = os.path.join(GOLDEN, 'assets')
QS = (0.0, 25.0, 37.5, 50.0, 95.0, 100.0)
Q8 = QS + (5.0, 75.0)


def _segmentation(rng, kind, K, spatial):
    """planes [K, *spatial] that overlap, the last one empty where K > 1; or a label map with K values that are not 1 ... K, the last absent."""
    if kind == 'planes':
        seg = ((rng.random((K,) + spatial) < 0.6) * rng.integers(1, 256, (K,) + spatial)).astype(np.uint8)
        seg[0].flat[0] = 1
        if K > 1:
            seg[K - 1] = 0
        return seg, None
    values = [int(v) for v in rng.permutation(np.arange(2, 256))[:K]]
    pool = np.array([0] + values[:max(K - 1, 1)], np.uint8)
    seg = pool[rng.integers(0, len(pool), spatial)]
    seg.flat[0] = values[0]
    return seg, values


def _intensities(rng, C, spatial):
    x = (rng.normal(size=(C,) + spatial) * 10.0 ** rng.integers(-3, 5, (C,) + spatial)).astype(np.float32)
    x[0] = np.round(x[0])                                                              # ties
    return x


def _check(seg, values, x, qs, max_scratch=0):
    spatial = seg.shape if values is not None else seg.shape[1:]
    ref = S.label_percentiles_statement(seg, x, qs, values)
    dev = S._device_percentiles(np.ascontiguousarray(seg), values, spatial, np.ascontiguousarray(x), list(qs), 0, max_scratch)
    assert dev is not None
    assert dev['count'].dtype == np.int64 and np.array_equal(dev['count'], ref['count'])
    assert dev['rank_value'].dtype == np.float32 and dev['rank_value'].shape == ref['rank_value'].shape
    assert np.array_equal(dev['rank_value'].view(np.uint32), ref['rank_value'].view(np.uint32))
    assert dev['rank_weight'].dtype == np.float64 and np.array_equal(dev['rank_weight'].view(np.uint64), ref['rank_weight'].view(np.uint64))
    assert np.array_equal(dev['percentile'].view(np.uint64), ref['percentile'].view(np.uint64))
    return dev


EXTENTS = [(5, 9, 70), (3, 66, 7), (1, 6, 6), (2, 2, 2), (1, 1, 1)]


@pytest.mark.parametrize('spatial', EXTENTS)
def test_entry_equals_the_statement_bit_for_bit(spatial):
    """K = 1, 3, 5 with one label absent, both kinds, C = 1, 2, 3 and P = 1, 2, 8 (6 for the full set of q), as 3-D and, where Z = 1, as 2-D."""
    i = EXTENTS.index(spatial)
    rng = np.random.default_rng(3500 + i)
    for j, K in enumerate((1, 3, 5)):
        for kind in ('planes', 'labelmap'):
            shape = spatial[1:] if spatial[0] == 1 and j == 1 else spatial
            seg, values = _segmentation(rng, kind, K, shape)
            C = 1 + (i + j + (kind == 'planes')) % 3
            qs = ((50.0,), (25.0, 95.0), Q8, QS)[(i + 2 * j + (kind == 'planes')) % 4]
            dev = _check(seg, values, _intensities(rng, C, shape), qs)
            assert K == 1 or dev['count'][K - 1] == 0


def test_a_box_inside_the_extent():
    """A box that starts at x = 65 and row 7 of (3, 5, 140): the walk begins at the box's first row and column, beyond the first 64 lanes."""
    spatial = (3, 5, 140)
    rng = np.random.default_rng(3510)
    x = _intensities(rng, 2, spatial)
    planes = np.zeros((2,) + spatial, np.uint8)
    planes[0, 1, 2:, 65:] = rng.random((3, 75)) < 0.7
    planes[0, 2, :4, 65:139] = 1
    planes[0, 1, 2, 65] = 1
    planes[1, 1, 2, 65:131] = 1                                                        # one row of 66 samples
    dev = _check(planes, None, x, QS)
    assert dev['count'][1] == 66
    lab = np.where(planes[0] > 0, 200, 0).astype(np.uint8)
    lab[0, 0, 0] = 9                                                                   # a second label in the far corner: its box is one sample
    _check(lab, [200, 9], x, QS)


def _const_hist_blocks():
    with open(os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc', 'kernels_stats_select.h')) as f:
        return int(re.search(r'constexpr int kLsHistMaxBlocks = (\d+);', f.read()).group(1))


def test_a_box_of_more_rows_than_one_pass_of_the_histogram_blocks():
    blocks = _const_hist_blocks()
    rng = np.random.default_rng(3511)
    for spatial in ((1, blocks + 1, 3), (2, blocks // 2 + 1, 3)):                      # block 0 walks two box rows; the second spans two z
        seg, values = _segmentation(rng, 'labelmap', 2, spatial)
        seg[0, 0, 0], seg[-1, -1, -1] = values[0], values[0]                           # the box is the whole extent
        _check(seg, values, _intensities(rng, 1, spatial), (0.0, 50.0, 100.0))


def test_sample_sets_that_drive_the_rounds():
    spatial = (2, 7, 70)
    rng = np.random.default_rng(3512)
    n = int(np.prod(spatial))
    seg, _ = _segmentation(rng, 'planes', 4, spatial)
    seg[1] = 255                                                                       # a label that covers everything
    seg[2] = 0; seg[2, 1, 3, 66] = 1                                                   # n = 1
    seg[3] = 0; seg[3, 0, 6, 69] = 1; seg[3, 1, 0, 0] = 1                              # n = 2
    const = np.full(spatial, -7.25, np.float32)                                        # one bin in every round, all ties
    low = (np.float32(1.0).view(np.uint32) + rng.integers(0, 256, spatial).astype(np.uint32)).view(np.float32)      # the decision falls in round 3
    top = np.array([1e-30, 1e-10, 1.0, 1e10, 1e30, -1e-30, -1e-10, -1.0, -1e10, -1e30], np.float32)[rng.integers(0, 10, spatial)]
    low_bytes = (top.view(np.uint32) & np.uint32(0xFF000000)).view(np.float32)         # values that differ in the top byte alone
    mixed = rng.choice(np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, -1e-39, 3e38, -3e38, 1.0, -1.0], np.float32), spatial)
    assert len(np.unique(low.view(np.uint32) >> 8)) == 1 and not (low_bytes.view(np.uint32) & np.uint32(0x00FFFFFF)).any()
    dev = _check(seg, None, np.stack([const, low, low_bytes]), Q8)
    assert (dev['rank_value'][:, 0] == -7.25).all() and dev['count'].tolist()[1:] == [n, 1, 2]
    dev = _check(seg, None, np.stack([mixed, top]), Q8)
    assert np.signbit(dev['rank_value'][1, 0]).any() and (dev['rank_value'][1, 0] == 0).any()
    zeros = np.where(rng.random(spatial) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    dev = _check(seg, None, zeros[None], (0.0, 50.0, 100.0))                           # -0.0 right below +0.0
    assert np.signbit(dev['rank_value'][1, 0, 0, 0]) and not np.signbit(dev['rank_value'][1, 0, 2, 1])


@pytest.mark.parametrize('kind', ['planes', 'labelmap'])
def test_the_label_chunks_and_the_bound(kind):
    rng = np.random.default_rng(3513)
    spatial = (2, 8, 70)
    K, C, qs = 8, 2, (5.0, 50.0, 95.0)
    seg, values = _segmentation(rng, kind, K, spatial)
    x = _intensities(rng, C, spatial)
    whole = _check(seg, values, x, qs)
    per_label = C * 2 * len(qs) * (8 + 8 + 256 * 4) + 2 * 8 * 20                       # the state of one label (include/ts2d_engine.h)
    for labels in (8, 4, 2, 1, 3):                                                     # 1, 2, 4 and 8 chunks; 3 + 3 + 2
        part = _check(seg, values, x, qs, max_scratch=per_label * labels + per_label // 2)
        for f in whole:
            assert np.array_equal(whole[f], part[f]), (labels, f)
    with pytest.raises(RuntimeError, match='ONE label'):
        S._device_percentiles(np.ascontiguousarray(seg), values, spatial, x, list(qs), 0, per_label - 1)


def test_refusals_by_name_leave_the_outputs_untouched():
    lib = _lib.load()
    K, Z, H, W, C, P = 3, 2, 4, 9, 2, 2
    seg = np.ones((K, Z, H, W), np.uint8)
    vals = np.array([5, 6, 7], np.uint8)
    zero = np.array([5, 0, 7], np.uint8)
    x = np.ones((C, Z, H, W), np.float32)
    q = np.array([50.0, 95.0], np.float64)
    count = np.full(K, -77, np.int64)
    rank = np.full((K, C, P, 2), -77.5, np.float32)
    weight = np.full((K, P), -77.5, np.float64)
    status = ctypes.c_int(0)
    good = dict(seg=seg.ctypes.data, kind=0, values=None, K=K, Z=Z, H=H, W=W, x=x.ctypes.data, C=C, q=q.ctypes.data, P=P, bound=0,
                count=count.ctypes.data, rank=rank.ctypes.data, weight=weight.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ts2d_label_percentiles(0, a['seg'], a['kind'], a['values'], a['K'], a['Z'], a['H'], a['W'], a['x'], a['C'], a['q'], a['P'],
                                          a['bound'], a['count'], a['rank'], a['weight'], ctypes.byref(status))

    def qv(*v):
        arr = np.array(v, np.float64)
        keep.append(arr)
        return arr.ctypes.data

    keep = []
    refusals = [(dict(seg=None), 'null'), (dict(x=None), 'null'), (dict(q=None), 'null'), (dict(count=None), 'null'), (dict(rank=None), 'null'),
                (dict(weight=None), 'null'), (dict(kind=2), 'kind'), (dict(K=0), 'labels'), (dict(K=256), 'labels'), (dict(Z=0), 'voxels'),
                (dict(Z=65536, H=65536, W=1), 'voxels'), (dict(C=0), 'channels'), (dict(C=_lib.STATS_MAX_CHANNELS + 1), 'channels'),
                (dict(P=0), 'percentiles outside'), (dict(P=_lib.STATS_MAX_PERCENTILES + 1), 'percentiles outside'),
                (dict(q=qv(50.0, np.nan)), r'percentiles\[1\]'), (dict(q=qv(-0.5, 50.0)), r'percentiles\[0\]'), (dict(q=qv(50.0, 100.5)), r'percentiles\[1\]'),
                (dict(q=qv(np.inf, 50.0)), r'percentiles\[0\]'), (dict(kind=1), 'values'), (dict(kind=1, values=zero.ctypes.data), 'background'),
                (dict(bound=C * 2 * P * 1040 + Z * H * 20 - 1), 'ONE label')]
    for kw, word in refusals:
        assert call(**kw) != 0, kw
        assert 'ts2d_label_percentiles' in _lib.last_error() and re.search(word, _lib.last_error()), (kw, _lib.last_error())
        assert (count == -77).all() and (rank == -77.5).all() and (weight == -77.5).all()
    assert call(bound=C * 2 * P * 1040 + Z * H * 20) == 0 and status.value == 0          # exactly one label fits: served
    assert count.tolist() == [Z * H * W] * 3 and (rank == 1.0).all()
    lab = seg[0] * 6
    assert call(kind=1, values=vals.ctypes.data, seg=lab.ctypes.data) == 0 and count.tolist() == [0, Z * H * W, 0]
    assert not rank[0].view(np.uint32).any() and not weight[0].view(np.uint64).any()      # an empty label: +0.0 everywhere


def _annotated(seg):
    img = nrrd.Image(np.moveaxis(seg, 0, -1), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).reshape(-1)), seg.shape[0], {}, None)
    image.set_annotation_meta(img, {i + 1: f'l{i}' for i in range(seg.shape[0])})
    return img


def test_a_non_finite_intensity_is_a_status_and_the_statement_answers():
    rng = np.random.default_rng(3514)
    spatial = (2, 9, 100)
    seg, _ = _segmentation(rng, 'planes', 4, spatial)
    seg[1, 1, 4, 77] = 1
    outside = seg.max(axis=0) == 0
    assert outside.any()
    lib = _lib.load()
    q = np.array([5.0, 50.0], np.float64)
    for bad in (np.nan, np.inf, -np.inf):
        x = _intensities(rng, 2, spatial)
        x[1, 1, 4, 77] = bad
        assert S._device_percentiles(seg, None, spatial, x, [5.0, 50.0], 0) is None
        count = np.full(4, -77, np.int64)
        rank = np.full((4, 2, 2, 2), -77.5, np.float32)
        weight = np.full((4, 2), -77.5, np.float64)
        status = ctypes.c_int(0)
        rc = lib.ts2d_label_percentiles(0, seg.ctypes.data, _lib.STATS_PLANES, None, 4, 2, 9, 100, x.ctypes.data, 2, q.ctypes.data, 2, 0, count.ctypes.data,
                                        rank.ctypes.data, weight.ctypes.data, ctypes.byref(status))
        assert rc == 0 and status.value == _lib.STATS_NONFINITE
        assert (count == -77).all() and (rank == -77.5).all() and (weight == -77.5).all()                                   # outputs untouched
        img = _annotated(seg)
        with np.errstate(all='ignore'):
            dev = S.label_statistics(img, {'a': x[0], 'b': x[1]}, device=0, percentiles=(5, 50))
            host = S.label_statistics(img, {'a': x[0], 'b': x[1]}, percentiles=(5, 50))
        assert json.dumps(dev, sort_keys=True) == json.dumps(host, sort_keys=True)
        assert bad == bad or np.isnan(dev['l1']['intensity']['b']['percentile']['50.0'])              # a NaN under the label: NaN
        x[1, 1, 4, 77] = 1.0
        x[0][outside] = bad                                                            # non-finite under NO label: served
        _check(seg, None, x, (5.0, 50.0))


def test_label_statistics_on_the_device_equals_the_host_route(monkeypatch):
    calls = {'statistics': 0, 'percentiles': 0}
    orig_s, orig_p = engine.label_statistics, engine.label_percentiles
    monkeypatch.setattr(engine, 'label_statistics', lambda *a, **kw: (calls.__setitem__('statistics', calls['statistics'] + 1), orig_s(*a, **kw))[1])
    monkeypatch.setattr(engine, 'label_percentiles', lambda *a, **kw: (calls.__setitem__('percentiles', calls['percentiles'] + 1), orig_p(*a, **kw))[1])
    rng = np.random.default_rng(3515)
    for spatial in ((3, 20, 131), (33, 70)):
        seg, _ = _segmentation(rng, 'planes', 5, (1,) * (3 - len(spatial)) + spatial)
        x = _intensities(rng, 2, spatial)
        img = nrrd.Image(np.moveaxis(seg.reshape((5,) + spatial), 0, -1), (1.0,) * len(spatial), (0.0,) * len(spatial),
                         tuple(np.eye(len(spatial)).reshape(-1)), 5, {}, None)
        image.set_annotation_meta(img, {i + 1: f'l{i}' for i in range(5)})
        chans = {'a': x[0], 'b': x[1]}
        before = dict(calls)
        dev = S.label_statistics(img, chans, device=0, percentiles=(5, 50, 95))
        assert calls == {'statistics': before['statistics'] + 1, 'percentiles': before['percentiles'] + 1}
        host = S.label_statistics(img, chans, percentiles=(5, 50, 95))
        assert calls == {'statistics': before['statistics'] + 1, 'percentiles': before['percentiles'] + 1}      # the host route made no call
        assert dev == host and dev['l4']['intensity']['a']['percentile'] == {'5.0': None, '50.0': None, '95.0': None}
        assert all(isinstance(v, float) for v in dev['l0']['intensity']['b']['percentile'].values())
        # percentiles=(): the dict and the device calls of before
        plain = S.label_statistics(img, chans, device=0)
        assert calls == {'statistics': before['statistics'] + 2, 'percentiles': before['percentiles'] + 1}
        assert plain == S.label_statistics(img, chans) and all('percentile' not in i for e in plain.values() for i in e['intensity'].values())
        assert {n: {c: {k: v for k, v in i.items() if k != 'percentile'} for c, i in e['intensity'].items()} for n, e in dev.items()} == \
            {n: e['intensity'] for n, e in plain.items()}
    # a label map with values that are not 1 ... K
    lab, values = _segmentation(rng, 'labelmap', 4, (2, 9, 70))
    img = nrrd.Image(lab, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).reshape(-1)), 1, {}, None)
    image.set_annotation_meta(img, {int(v): f'v{v}' for v in np.unique(lab) if v})
    x = _intensities(rng, 1, (2, 9, 70))
    assert S.label_statistics(img, {'a': x[0]}, device=0, percentiles=(50,)) == S.label_statistics(img, {'a': x[0]}, percentiles=(50,))


def test_result_statistics_on_the_device_equal_the_host_route(tmp_path, monkeypatch):
    models = {'ts2d-v2-ep4000b2_cardiac': synthetic_model('ts2d-v2-ep4000b2_cardiac', 3, 31, patch=(64, 64), mirror=False)[0]}
    calls = []
    orig = engine.label_percentiles
    monkeypatch.setattr(engine, 'label_percentiles', lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    with TS2D(models=models) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device == 0
        plain = res.statistics()
        dev_files = res.save_statistics(str(tmp_path / 'plain'), 'case')
        assert not calls                                                               # without percentiles ts2d_label_percentiles is not called
        dev = res.statistics(percentiles=(5, 50, 95))
        dev_files = res.save_statistics(str(tmp_path / 'dev'), 'case', percentiles=(5, 50, 95))
        n_dev = len(calls)
        res.device = None
        host = res.statistics(percentiles=(5, 50, 95))
        host_files = res.save_statistics(str(tmp_path / 'host'), 'case', percentiles=(5, 50, 95))
        assert n_dev == 2 and len(calls) == n_dev
        assert dev == host and any(e['exists'] for e in dev.values())
        assert all(list(i['percentile']) == ['5.0', '50.0', '95.0'] for e in dev.values() for i in e['intensity'].values())
        assert {n: {c: {k: v for k, v in i.items() if k != 'percentile'} for c, i in e['intensity'].items()} for n, e in dev.items()} == \
            {n: e['intensity'] for n, e in plain.items()}
        for a, b in zip(dev_files, host_files):
            with open(a, 'rb') as fa, open(b, 'rb') as fb:
                assert fa.read() == fb.read()
