"""Crop box, z-score and resample of a native 2-D input on the MI355X: the ts2d_planes handle (csrc/kernels_prep.h) against the numpy statement of
its arithmetic (preprocess.zscore_f32_statement / crop_box_statement, which tests/test_prep_cpu.py pins to numpy) - every bit of every float32
result, the box, the statistics and the clip bounds - and the product surface (HIPModel.apply / apply_batch, TS2D.predict / predict_many) with
the switch ``device_input_normalize`` on and off."""
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, nrrd
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu
A = os.path.join(GOLDEN, 'assets')


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _statement(data):
    """(box, normalised planes [C, 1, h, w], stats [C, 2]) of the host statement."""
    box = P.crop_box_statement(data)
    (_, _), (r0, r1), (c0, c1) = box
    planes = [np.ascontiguousarray(data[c, 0, r0:r1, c0:c1]) for c in range(data.shape[0])]
    stats = np.array([P.zscore_stats_f32_statement(p)[:2] for p in planes], np.float32)
    return box, np.stack([P.zscore_f32_statement(p) for p in planes])[:, None], stats


def _check(data, out_hw=None):
    box, want, stats = _statement(data)
    with P.DevicePlanes(data, 0) as p:
        assert p.shape == data.shape
        assert p.crop_zscore() == box and p.shape == want.shape
        assert np.array_equal(_bits(p.stats), _bits(stats)), (data.shape, p.stats, stats)
        got = p.download()
        diff = _bits(got) != _bits(want)
        assert not diff.any(), (data.shape, box, int(diff.sum()))
        if out_hw is not None:                       # the clip bounds the handle kept are the planes' minimum and maximum: the resample shows them
            res = P.resample_planes_cubic_device(p, out_hw, 0)
            assert res.shape == (data.shape[0], 1) + tuple(out_hw) and p.shape == res.shape
            for c in range(data.shape[0]):
                assert np.array_equal(_bits(res[c, 0]), _bits(P.resize_cubic_f64(want[c, 0], out_hw))), (data.shape, out_hw, c)
    return got


def _data(seed, c, h, w, kind='normal', border=(0, 0, 0, 0)):
    rng = np.random.default_rng(seed)
    t, b, l, r = border
    hh, ww = h - t - b, w - l - r
    if kind == 'normal':
        core = rng.standard_normal((c, 1, hh, ww)) * 200 + 50
    elif kind == 'ints':
        core = rng.integers(-1000, 3000, (c, 1, hh, ww))
    else:
        core = rng.standard_normal((c, 1, hh, ww)) * 10.0 ** rng.uniform(-6, 6, (c, 1, hh, ww))
    data = np.zeros((c, 1, h, w), np.float32)
    data[:, :, t:h - b, l:w - r] = core.astype(np.float32)
    return data


@pytest.mark.parametrize('c,h,w,border', [(1, 3, 5, (0, 0, 0, 0)), (2, 9, 7, (1, 0, 0, 2)), (3, 64, 128, (0, 0, 0, 0)), (2, 90, 77, (0, 5, 3, 0)), (1, 91, 91, (0, 0, 0, 0)),
                                          (2, 644, 337, (7, 9, 11, 13)), (3, 129, 131, (0, 1, 0, 0)), (1, 1000, 1111, (100, 0, 0, 100)), (2, 2000, 1500, (0, 0, 0, 0)),
                                          (1, 3000, 2500, (3, 0, 0, 1))])
def test_handle_equals_the_statement_bit_for_bit(c, h, w, border):
    for kind in ('normal', 'ints', 'hdr'):
        _check(_data(h + w, c, h, w, kind, border))


def test_planes_with_different_zero_patterns_share_one_box():
    data = np.zeros((3, 1, 70, 50), np.float32)
    rng = np.random.default_rng(3)
    data[0, 0, 10:20, 5:9] = rng.standard_normal((10, 4))
    data[1, 0, 40:61, 30:31] = 5.0                      # a single column lower down
    data[2, 0, 33, 2:49] = rng.standard_normal(47)      # a single row that widens the box
    got = _check(data)
    assert got.shape == (3, 1, 51, 47)
    single = np.zeros((2, 1, 40, 300), np.float32)
    single[0, 0, 17, 20:280] = rng.standard_normal(260)             # single-row box
    assert _check(single).shape == (2, 1, 1, 260)


def test_constant_and_all_zero_planes():
    zero = np.zeros((2, 1, 33, 47), np.float32)
    assert not _check(zero).any()                                     # the whole extent stays, std 0: divided by 1e-8
    const = np.full((2, 1, 120, 90), np.float32(-3.25), np.float32)
    const[1] = 7.5
    _check(const)
    neg = np.full((1, 1, 12, 700), -0.0, np.float32)                  # the sum starts from +0: the mean is +0 and every sample stays -0
    got = _check(neg)
    assert np.signbit(got).all()
    mixed = _data(5, 2, 200, 300)
    mixed[1] = 1e-3                                                   # one constant plane beside a varying one
    _check(mixed, (133, 301))


@pytest.mark.parametrize('hw,out', [((600, 512), (400, 273)), ((400, 512), (667, 256)), ((90, 77), (150, 103)), ((33, 47), (80, 21))])
def test_resample_up_and_down_on_the_handle_equals_the_statement(hw, out):
    _check(_data(hw[0], 2, hw[0] + 9, hw[1] + 4, border=(4, 5, 1, 3)), out)


def test_two_runs_give_the_same_bytes():
    data = _data(11, 2, 1500, 1100, border=(0, 10, 10, 0))
    runs = []
    for _ in range(2):
        with P.DevicePlanes(data, 0) as p:
            p.crop_zscore()
            runs.append((p.download().tobytes(), p.resample((700, 333)).download().tobytes()))
    assert runs[0] == runs[1]


def test_a_nan_sample_sets_nonfinite_and_the_entries_refuse_by_name():
    for bad in (np.nan, np.inf, -np.inf):
        data = _data(12, 2, 100, 90)
        data[1, 0, 50, 50] = bad
        with P.DevicePlanes(data, 0) as p:
            assert p.crop_zscore() is None
    with P.DevicePlanes(_data(13, 1, 20, 20), 0) as p:
        with pytest.raises(RuntimeError, match='ts2d_planes_resample_cubic: the planes carry no clip bounds'):
            p.resample((10, 10))
        p.crop_zscore()
        with pytest.raises(RuntimeError, match='ts2d_planes_resample_cubic: extents 20 x 20 -> 1 x 10'):
            p.resample((1, 10))
        assert p.resample((10, 10)).shape == (1, 1, 10, 10)
        with pytest.raises(RuntimeError, match='clip bounds'):       # a resample uses them up
            p.resample((20, 20))
    assert _lib.load().ts2d_planes_download(None, None) == -1 and 'ts2d_planes_download: null' in _lib.last_error()


# ------------------------------------------------------------------------------------------------ surface
def _image(seed, hw, spacing, channels=2, border=0):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(hw + (channels,)) * 200 + 50).astype(np.float32)
    if border:
        a[:border] = 0; a[:, -border:] = 0
    if channels == 1:
        a = a[..., 0]
    return nrrd.Image(a, spacing, (3.0, -7.0), (1.0, 0.0, 0.0, 1.0), channels, {}, None)


class _Witness:
    """Counts the handles the product creates."""
    def __init__(self, monkeypatch):
        self.shapes = []
        orig = P.DevicePlanes.__init__

        def init(planes, data, device, lib=None):
            self.shapes.append(tuple(data.shape))
            orig(planes, data, device, lib)
        monkeypatch.setattr(P.DevicePlanes, '__init__', init)


def _both(model, imgs, witness):
    """apply and apply_batch with the switch on and off -> the results, after checking the witness."""
    out = {}
    for on in (True, False):
        model.device_input_normalize = on
        del witness.shapes[:]
        pre = {n: model._preprocess_input(i) for n, i in imgs.items()}
        assert len(witness.shapes) == (len(imgs) if on else 0)
        out[on] = (pre, {n: model.apply(i) for n, i in imgs.items()}, model.apply_batch(dict(imgs)))
        assert len(witness.shapes) == (3 * len(imgs) if on else 0)
    model.device_input_normalize = True
    return out


def _assert_equal(out, imgs):
    keys = ('shape_before_cropping', 'bbox_used_for_cropping', 'shape_after_cropping_and_before_resampling')
    for n in imgs:
        (_, d_on, p_on), (_, d_off, p_off) = out[True][0][n], out[False][0][n]
        assert d_on.shape == d_off.shape and np.array_equal(_bits(d_on), _bits(d_off)), n
        assert all(p_on[k] == p_off[k] for k in keys) and 'device_normalize' not in p_on, n
        for k in (1, 2):
            assert np.array_equal(out[True][k][n].array, out[False][k][n].array) and out[True][k][n].meta == out[False][k][n].meta, n
        assert out[True][1][n].array.any(), n


def test_apply_and_apply_batch_are_byte_identical_with_the_switch_on_and_off(monkeypatch):
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    witness = _Witness(monkeypatch)
    model = synthetic_model('ts2d-v2-ep4000b2_cardiac', 3, 41, patch=(64, 64), mirror=True)[0]
    model.start()
    try:
        assert model.device_input_normalize is True and model._normalize_device() == 0
        s0332 = nrrd.read(os.path.join(A, 'sample_s0332.nrrd'))
        imgs = {'s0616': nrrd.read(os.path.join(A, 'sample_s0616.nrrd')),
                's0332': nrrd.Image(np.ascontiguousarray(s0332.array[:, 0]), (s0332.spacing[0], s0332.spacing[2]), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None),
                'off_spacing_zero_border': _image(1, (150, 131), (0.9, 1.2), border=9), 'up': _image(2, (90, 77), (2.5, 2.0)),
                'plan': _image(3, (80, 80), (1.5, 1.5), border=3)}
        out = _both(model, imgs, witness)
        _assert_equal(out, imgs)
        assert out[True][0]['off_spacing_zero_border'][2]['bbox_used_for_cropping'] == [[0, 1], [9, 150], [0, 122]]
        model.device_input_resample = False                  # z-score on the device, resample on the host: the same bytes again
        d = model._preprocess_input(imgs['up'])[1]
        assert np.array_equal(_bits(d), _bits(out[False][0]['up'][1]))
    finally:
        model.stop()


def test_a_one_channel_model_on_an_x_ray_image(monkeypatch):
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    witness = _Witness(monkeypatch)
    model = synthetic_model('tsxr-v1_lung', 2, 43, channels=('xray',), patch=(64, 64), mirror=True)[0]
    model.start()
    try:
        chex = nrrd.read(os.path.join(A, 'sample_chexpert.nrrd'))
        imgs = {'chexpert': chex, 'big': _image(4, (700, 500), (0.7, 0.8), channels=1, border=20)}
        out = _both(model, imgs, witness)
        _assert_equal(out, imgs)
    finally:
        model.stop()


def test_below_the_threshold_the_host_route_stays(monkeypatch):
    witness = _Witness(monkeypatch)
    model = synthetic_model('ts2d-v2-ep4000b2_cardiac', 3, 41, patch=(64, 64), mirror=True)[0]
    model.start()
    try:
        img = _image(5, (80, 80), (1.5, 1.5))
        monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 2 * 80 * 80 + 1)
        model._preprocess_input(img)
        assert witness.shapes == []
        monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 2 * 80 * 80)
        model._preprocess_input(img)
        assert witness.shapes == [(2, 1, 80, 80)]
    finally:
        model.stop()


def test_predict_and_predict_many_on_a_2d_asset(monkeypatch):
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    witness = _Witness(monkeypatch)
    ids = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_muscles')
    models = {m: synthetic_model(m, 3 + 2 * i, 41 + i, patch=(64, 64), mirror=True)[0] for i, m in enumerate(ids)}
    paths = [os.path.join(A, 'sample_s0616.nrrd'), os.path.join(A, 'sample_s0332.nrrd')]
    with TS2D(models=models) as ts:
        res = {}
        for on in (True, False):
            for m in models.values():
                m.device_input_normalize = on
            del witness.shapes[:]
            res[on] = ([ts.predict(p) for p in paths], ts.predict_many(paths))
            assert bool(witness.shapes) == on
        for k in (0, 1):
            for a, b in zip(res[True][k], res[False][k]):
                assert a.models == b.models == sorted(ids)
                for m in [None] + list(ids):
                    sa, sb = a.get_segmentation(m), b.get_segmentation(m)
                    assert np.array_equal(sa.array, sb.array) and sa.meta == sb.meta and sa.size == sb.size, (k, m)
                assert a.get_segmentation().array.any()
