"""The device input resample on the MI355X: ts2d_resample_cubic (csrc/kernels_resample_in.h) against the numpy statement of its arithmetic
(preprocess.resize_cubic_f64, which tests/test_resample_cubic_cpu.py pins to scipy) - every bit of every float32 result - and the
product surface (HIPModel.apply / apply_batch) on cases off the plan spacing with the switch ``device_input_resample`` on and off."""
import numpy as np
import pytest

from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, nrrd
from totalsegmentator2d_amd import preprocess as P

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device(planes, out_hw):
    planes = np.ascontiguousarray(planes, np.float32)
    out = P.resample_planes_cubic_device(planes[:, None], out_hw, 0)
    assert out is not None and out.dtype == np.float32 and out.shape == (planes.shape[0], 1) + tuple(out_hw)
    return out[:, 0]


def _check(planes, out_hw):
    got = _device(planes, out_hw)
    for p, pl in enumerate(planes):
        want = P.resize_cubic_f64(pl, out_hw)
        diff = _bits(got[p]) != _bits(want)
        assert not diff.any(), (planes.shape, out_hw, p, int(diff.sum()), float(np.abs(got[p] - want).max()))
    return got


def _zscored(seed, n, hw):
    rng = np.random.default_rng(seed)
    return np.stack([P.zscore((rng.standard_normal(hw) * 200 + 50).astype(np.float32)) for _ in range(n)])


# the three geometries of profiles/r09_resampled_case.txt: original extent -> network extent at 1.5 mm
@pytest.mark.parametrize('hw,out', [((600, 512), (400, 273)), ((400, 512), (667, 256)), ((1000, 512), (400, 239))])
def test_case_geometries_equal_the_statement_bit_for_bit(hw, out):
    _check(_zscored(hw[0], 2, hw), out)


@pytest.mark.parametrize('n', [1, 2, 3])
def test_plane_counts_and_widths_that_are_no_multiple_of_four(n):
    for hw, out in (((33, 47), (80, 21)), ((64, 52), (27, 66)), ((9, 31), (50, 77)), ((40, 40), (40, 91)), ((57, 40), (30, 40)), ((2, 2), (5, 7))):
        _check(_zscored(n + hw[1], n, hw), out)


def test_special_planes():
    rng = np.random.default_rng(8)
    hw, out = (90, 70), (131, 52)
    const = np.full(hw, np.float32(-3.25), np.float32)
    hdr = (rng.standard_normal(hw) * 10.0 ** rng.uniform(-6, 6, hw)).astype(np.float32)
    at_bounds = np.where(rng.random(hw) < 0.5, np.float32(-2.0), np.float32(5.0)).astype(np.float32)     # overshoot everywhere: the clip decides
    zero_bg = np.zeros(hw, np.float32); zero_bg[30:40, 20:30] = 700.0                                    # -0.0 at the lower bound keeps its sign
    got = _check(np.stack([const, hdr, at_bounds, zero_bg]), out)
    assert (got[0] == np.float32(-3.25)).all()
    assert got[2].min() == -2.0 and got[2].max() == 5.0 and ((got[2] == -2.0) | (got[2] == 5.0)).mean() > 0.2
    ints = rng.integers(-1000, 3000, (3,) + hw).astype(np.float32)
    _check(ints, out)
    _check(ints[:, :50, :33], (50, 70))             # identity-sized along one axis
    _check(ints[:, :50, :33], (20, 33))


def test_two_calls_give_the_same_bytes():
    planes = _zscored(4, 2, (200, 150))
    a, b = _device(planes, (133, 301)), _device(planes, (133, 301))
    assert a.tobytes() == b.tobytes()


def test_bad_arguments_are_refused_by_name_and_a_good_call_follows():
    lib = _lib.load()
    src = _zscored(1, 1, (16, 16)); dst = np.zeros((1, 9, 9), np.float32)
    lh = np.array([[src.min(), src.max()]], np.float32)
    assert lib.ts2d_resample_cubic(0, None, 1, 16, 16, 9, 9, lh.ctypes.data, dst.ctypes.data) == -1 and 'ts2d_resample_cubic: null' in _lib.last_error()
    assert lib.ts2d_resample_cubic(0, src.ctypes.data, 1, 16, 1, 9, 9, lh.ctypes.data, dst.ctypes.data) == -1 and 'extents' in _lib.last_error()
    inv = lh[:, ::-1].copy()
    assert lib.ts2d_resample_cubic(0, src.ctypes.data, 1, 16, 16, 9, 9, inv.ctypes.data, dst.ctypes.data) == -1 and 'clip bounds' in _lib.last_error()
    assert lib.ts2d_resample_cubic(0, src.ctypes.data, 1, 16, 16, 9, 9, lh.ctypes.data, dst.ctypes.data) == 0
    assert np.array_equal(_bits(dst[0]), _bits(P.resize_cubic_f64(src[0], (9, 9))))
    bad = src.copy(); bad[0, 3, 3] = np.nan                                                               # the Python wrapper keeps such a plane on the host
    assert P.resample_planes_cubic_device(bad[:, None], (9, 9), 0) is None


# ------------------------------------------------------------------------------------------------ surface
def _image(seed, hw, spacing):
    rng = np.random.default_rng(seed)
    return nrrd.Image((rng.standard_normal(hw + (2,)) * 200 + 50).astype(np.float32), spacing, (3.0, -7.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


def test_apply_and_apply_batch_equal_the_host_resample(monkeypatch):
    """Off-spacing cases through HIPModel.apply / apply_batch with the device input resample on and off: the statement is bit for bit scipy,
    so the preprocessed planes and the masks are equal byte for byte.  A witness counts the entry's calls: one per case, none when off."""
    model = synthetic_model('ts2d-v2-ep4000b2_cardiac', 3, 41, patch=(64, 64), mirror=True)[0]
    model.start()
    calls = []
    orig = P.resample_planes_cubic_device
    monkeypatch.setattr(P, 'resample_planes_cubic_device', lambda d, hw, dev: (calls.append(d.shape), orig(d, hw, dev))[1])
    try:
        imgs = {'up': _image(1, (90, 77), (2.5, 2.0)), 'down': _image(2, (150, 131), (0.9, 1.2)), 'plan': _image(3, (80, 80), (1.5, 1.5))}
        assert model.device_input_resample is True and model._resample_device() == 0
        pre_dev = {n: model._preprocess_input(i)[1] for n, i in imgs.items()}
        assert calls == [(2, 1, 90, 77), (2, 1, 150, 131)]
        del calls[:]
        dev_one = {n: model.apply(i) for n, i in imgs.items()}
        dev_many = model.apply_batch(dict(imgs))
        assert len(calls) == 4
        del calls[:]
        model.device_input_resample = False
        pre_host = {n: model._preprocess_input(i)[1] for n, i in imgs.items()}
        host_one = {n: model.apply(i) for n, i in imgs.items()}
        host_many = model.apply_batch(dict(imgs))
        assert calls == []
        for n in imgs:
            assert pre_dev[n].shape == pre_host[n].shape and np.array_equal(_bits(pre_dev[n]), _bits(pre_host[n])), n
            assert np.array_equal(dev_one[n].array, host_one[n].array) and dev_one[n].meta == host_one[n].meta, n
            assert np.array_equal(dev_many[n].array, host_many[n].array) and dev_many[n].meta == host_many[n].meta, n
            assert dev_one[n].array.any(), n
    finally:
        model.stop()
