"""ts2d_label_statistics (csrc/kernels_stats.h) against its statement, statistics.label_statistics_statement, bit for bit - the float64 bits of
sum, ssq, mean and std included -, the status bit, and the device route of TS2D.Result.statistics / save_statistics and of a label-map stack."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import cases
from tests.conftest import GOLDEN
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, engine, nrrd, prng, statistics as S
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu
A = os.path.join(GOLDEN, 'assets')
INT_FIELDS = ('count', 'bbox_min', 'bbox_max', 'index_sum', 'exists')
F64_FIELDS = ('sum', 'ssq', 'mean', 'std', 'mm')


def _segmentation(rng, kind, K, spatial):
    """planes [K, *spatial] with overlaps, an empty and a full plane where K allows; or a label map with K values, one of them absent."""
    if kind == 'planes':
        seg = ((rng.random((K,) + spatial) < rng.random((K,) + (1,) * len(spatial))) * rng.integers(1, 256, (K,) + spatial)).astype(np.uint8)
        if K > 1:
            seg[K - 1] = 0
        if K > 2:
            seg[K - 2] = 7
        return seg, None
    values = [int(v) for v in rng.permutation(np.arange(1, 256))[:K]]
    pool = np.array([0] + values[:max(K - 1, 1)], np.uint8)                     # the last value stays absent (K > 1)
    return pool[rng.integers(0, len(pool), spatial)], values


def _intensities(rng, C, spatial):
    if not C:
        return None
    x = (rng.normal(size=(C,) + spatial) * 10.0 ** rng.integers(-3, 5, (C,) + spatial)).astype(np.float32)
    return x


def _assert_same(dev, ref):
    assert dev is not None
    for f in INT_FIELDS:
        assert dev[f].dtype == ref[f].dtype and np.array_equal(dev[f], ref[f]), f
    for f in F64_FIELDS:
        assert dev[f].dtype == np.float64 and np.array_equal(dev[f].view(np.uint64), ref[f].view(np.uint64)), f
    for f in ('min', 'max'):
        assert dev[f].dtype == np.float32 and np.array_equal(dev[f].view(np.uint32), ref[f].view(np.uint32)), f


def _check(seg, values, x, max_scratch=0):
    spatial = seg.shape if values is not None else seg.shape[1:]
    sp = (0.7, 1.3, 2.9)[:len(spatial)]
    ref = S.label_statistics_statement(seg, x, sp, values)
    dev = S._device_statistics(np.ascontiguousarray(seg), values, spatial, x, sp, 0, max_scratch)
    _assert_same(dev, ref)
    return dev


SHAPES = [(Z, H, W) for Z in (1, 3) for H in (1, 2, 65) for W in (1, 63, 64, 65, 129, 337)]


@pytest.mark.parametrize('Z,H,W', SHAPES)
def test_entry_equals_the_statement_bit_for_bit(Z, H, W):
    """Every W x H x Z at which a lane, a wave or a row edge can go wrong, with K = 1, 2 and 117; both kinds and C = 1, 2 alternate over the cases."""
    i = SHAPES.index((Z, H, W))
    rng = np.random.default_rng(2800 + i)
    for j, K in enumerate((1, 2, 117)):
        kind = 'planes' if (i + j) % 2 == 0 else 'labelmap'
        spatial = (Z, H, W) if (Z > 1 or (i + j) % 3 == 0) else (H, W)          # a 2-D image is Z = 1 at the entry
        seg, values = _segmentation(rng, kind, K, spatial)
        _check(seg, values, _intensities(rng, 1 + (i + j) % 2, spatial))


@pytest.mark.parametrize('kind', ['planes', 'labelmap'])
def test_255_labels_and_the_label_chunks(kind):
    rng = np.random.default_rng(2855)
    spatial = (4, 8, 70)
    seg, values = _segmentation(rng, kind, 255, spatial)
    x = _intensities(rng, 2, spatial)
    whole = _check(seg, values, x)
    per_label = 4 * 8 * (20 + 16 * 2)                                            # the row partials of one label (include/ts2d_engine.h)
    for labels in (100, 1, 254):                                                # 3 chunks (100, 100, 55); one label at a time; 254 + 1
        part = _check(seg, values, x, max_scratch=per_label * labels + per_label // 2)
        for f in whole:
            assert np.array_equal(whole[f], part[f], equal_nan=True), (labels, f)
    with pytest.raises(RuntimeError, match='ONE label'):
        S._device_statistics(np.ascontiguousarray(seg), values, spatial, x, (1.0, 1.0, 1.0), 0, per_label - 1)


def test_index_sums_beyond_int32_no_channels_and_special_values():
    full = np.ones((1, 1, 3, 8192), np.uint8)                                    # one [1, 3, 8192] full plane
    dev = _check(full, None, None)
    assert dev['count'][0] == 3 * 8192 and dev['index_sum'][0].tolist() == [0, 8192 * 3, 3 * 8192 * 8191 // 2]
    wide = np.ones((1, 9, 65536), np.uint8)                                      # ... and one whose x sum really passes 2^31 (and 2^34)
    dev = _check(wide, None, None)
    assert dev['index_sum'][0, 1] == 9 * 65536 * 65535 // 2 > 2 ** 34
    tall = np.ones((1, 70000, 9), np.uint8)                                      # the row index times the row count, summed over 70 000 rows
    tall[0, ::3] = 0
    dev = _check(tall, None, np.arange(630000, dtype=np.float32).reshape(1, 70000, 9))
    assert dev['index_sum'][0, 0] > 2 ** 31
    rng = np.random.default_rng(2803)
    for kind in ('planes', 'labelmap'):                                          # C = 0: counts, boxes and index sums only
        seg, values = _segmentation(rng, kind, 5, (3, 20, 131))
        dev = _check(seg, values, None)
        assert dev['sum'].shape == (5, 0)
    # -0.0, denormals, +-3e38 (their float64 sum is exact where float32 would overflow)
    spatial = (2, 5, 200)
    seg, values = _segmentation(rng, 'planes', 6, spatial)
    x = np.zeros((2,) + spatial, np.float32)
    x[0] = rng.choice(np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, 3e38, -3e38, 1.0], np.float32), spatial)
    x[1] = -0.0
    dev = _check(seg, values, x)
    assert np.signbit(dev['min'][0, 1]) and np.signbit(dev['max'][0, 1]) and not np.signbit(dev['sum'][0, 1])
    lone = np.zeros((1,) + spatial, np.uint8)
    lone[0, 1, 3, 130] = 1
    _check(lone, None, x)


def test_a_non_finite_intensity_is_a_status_and_the_statement_answers():
    rng = np.random.default_rng(2804)
    spatial = (2, 9, 100)
    seg, _ = _segmentation(rng, 'planes', 4, spatial)
    seg[1, 1, 4, 77] = 1
    lib = _lib.load()
    for bad in (np.nan, np.inf, -np.inf):
        x = _intensities(rng, 2, spatial)
        x[1, 1, 4, 77] = bad
        assert S._device_statistics(seg, None, spatial, x, (1.0, 1.0, 1.0), 0) is None
        out_int = np.full((4, _lib.STATS_INTS), -77, np.int64)
        out_f64 = np.full((4, 2, _lib.STATS_F64S), -77.5, np.float64)
        status = ctypes.c_int(0)
        rc = lib.ts2d_label_statistics(0, seg.ctypes.data, _lib.STATS_PLANES, None, 4, 2, 9, 100, x.ctypes.data, 2, 0, out_int.ctypes.data,
                                       out_f64.ctypes.data, ctypes.byref(status))
        assert rc == 0 and status.value == _lib.STATS_NONFINITE and (out_int == -77).all() and (out_f64 == -77.5).all()      # outputs untouched
        img = nrrd.Image(np.moveaxis(seg, 0, -1), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).reshape(-1)), 4, {}, None)
        from totalsegmentator2d_amd import image
        image.set_annotation_meta(img, {i + 1: f'l{i}' for i in range(4)})
        with np.errstate(all='ignore'):
            dev = S.label_statistics(img, {'a': x[0], 'b': x[1]}, device=0)
            host = S.label_statistics(img, {'a': x[0], 'b': x[1]})
        assert json.dumps(dev, sort_keys=True) == json.dumps(host, sort_keys=True) and not np.isfinite(dev['l1']['intensity']['b']['mean'])
        x[1, 1, 4, 77] = 1.0
        seg2 = seg.copy()
        x[0][seg2.max(axis=0) == 0] = bad                                        # non-finite under NO label: of no consequence
        if (seg2.max(axis=0) == 0).any():
            assert S._device_statistics(seg2, None, spatial, x, (1.0, 1.0, 1.0), 0) is not None
    # refusals by name, outputs untouched
    out_int = np.full((4, _lib.STATS_INTS), -77, np.int64)
    status = ctypes.c_int(0)
    for args in ((seg.ctypes.data, 2, None, 4, 2, 9, 100, None, 0), (seg.ctypes.data, 0, None, 256, 2, 9, 100, None, 0),
                 (seg.ctypes.data, 0, None, 4, 2, 9, 100, None, 1), (seg.ctypes.data, 1, None, 4, 2, 9, 100, None, 0),
                 (seg.ctypes.data, 0, None, 4, 65536, 65536, 1, None, 0)):
        assert lib.ts2d_label_statistics(0, *args, 0, out_int.ctypes.data, None, ctypes.byref(status)) != 0 and (out_int == -77).all()


def test_result_statistics_on_the_device_equal_the_host_route(tmp_path, monkeypatch):
    ids = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_ribs')
    models = {m: synthetic_model(m, 3 + i, 31 + i, patch=(64, 64), mirror=False)[0] for i, m in enumerate(ids)}
    calls = []
    orig = engine.label_statistics
    monkeypatch.setattr(engine, 'label_statistics', lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    with TS2D(models=models) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device == 0
        seg = res.get_segmentation()
        before = seg.array.tobytes()
        dev = res.statistics()
        dev_files = res.save_statistics(str(tmp_path / 'dev'), 'case', models='all')
        n_dev = len(calls)
        res.device = None
        host = res.statistics()
        host_files = res.save_statistics(str(tmp_path / 'host'), 'case', models='all')
        assert n_dev == 4 and len(calls) == n_dev                                # the device served every call; the host route made none
        assert dev == host and len(dev) == 7 and any(e['exists'] for e in dev.values())
        assert all(sorted(e['intensity']) == ['max', 'mean'] for e in dev.values())
        assert [os.path.basename(f) for f in dev_files] == [os.path.basename(f) for f in host_files] == \
            ['case.statistics.json', 'case-cardiac.statistics.json', 'case-ribs.statistics.json']
        for a, b in zip(dev_files, host_files):
            with open(a, 'rb') as fa, open(b, 'rb') as fb:
                assert fa.read() == fb.read()
        assert seg.array.tobytes() == before


def test_a_label_map_stack_from_apply(tmp_path):
    from tests.test_gpu_labelmap import _write_model_folder
    from totalsegmentator2d_amd.model import HIPModel
    arch = cases.unet(3, (32, 32, 64), 6)
    _write_model_folder(str(tmp_path), 'labelmap', arch, [71], (64, 64))
    m = HIPModel({'root': str(tmp_path), 'model': 'ts2d-v2-ep4000b2_labelmap', 'revision': 1, 'folds': (0,), 'param': {'nnu.configuration': '2d'}})
    a = prng.normal_f32(63, 0, (16, 128, 128, 2)) * 40 + 10
    vol = nrrd.Image(a, (1.5, 1.5, 3.0), (1.0, 2.0, 3.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), 2, {}, 'left-posterior-superior')
    m.start()
    try:
        seg = m.apply(vol)
    finally:
        m.stop()
    assert seg.components == 1 and seg.array.shape == (16, 128, 128) and seg.array.dtype == np.uint8
    before = seg.array.tobytes()
    ch0 = np.ascontiguousarray(a[..., 0])
    dev = S.label_statistics(seg, {'ch0': ch0}, device=0)
    host = S.label_statistics(seg, {'ch0': ch0})
    assert dev == host and len(dev) >= 2 and all(e['exists'] for e in dev.values()) and seg.array.tobytes() == before
    assert sum(e['count'] for e in dev.values()) == int((seg.array > 0).sum())
