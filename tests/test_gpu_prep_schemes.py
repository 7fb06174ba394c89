"""Every nnU-Net normalisation scheme on the device-resident planes of the MI355X: ts2d_planes_crop_normalize (csrc/kernels_prep_schemes.h) against
the numpy statements of its arithmetic (preprocess.ct_f32_statement, rescale01_f32_statement, rgb01_f32_statement, masked_zscore_f32_statement, which
tests/test_prep_schemes_cpu.py pins to numpy) - every bit of every float32 result, the box, the statistics, the clip bounds through the resample, the
status bits - and the product surface (HIPModel.apply / apply_batch) with the switch ``device_input_normalize_schemes`` on and off."""
import numpy as np
import pytest

from tests import cases
from tests.prep_schemes_util import CT_PROPS, bits, case_statement
from totalsegmentator2d_amd import nrrd, weights
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.model import HIPModel

pytestmark = pytest.mark.gpu
FIP = {str(c): dict(CT_PROPS, mean=5.0 + c, std=20.0 - 3 * c) for c in range(3)}
Z, CT, RS, RGB, NO = P.NORM_SCHEME_IDS
# per case: the schemes of up to three channels (cycled) and whether the z-score channels are masked
KINDS = {'ct': ([CT], False), 'rescale': ([RS], False), 'rgb': ([RGB], False), 'none': ([NO], False), 'masked': ([Z], True),
         'ct + z-score + rescale': ([CT, Z, RS], False), 'masked + none + ct': ([Z, NO, CT], True)}


def _data(seed, c, h, w, kind, border=(0, 0, 0, 0), keep=0.8):
    """Planes for `kind`: inside the border N(7, 30) (integers 0 ... 255 for RGB) with values on and beyond the CT bounds, signed zeros and
    denormals sprinkled in, and zeros in the interior - single pixels (a fraction 1 - keep) and a whole row."""
    rng = np.random.default_rng(seed)
    t, b, l, r = border
    hh, ww = h - t - b, w - l - r
    if 'rgb' in kind:
        core = rng.integers(0, 256, (c, 1, hh, ww)).astype(np.float32)
    else:
        core = (rng.standard_normal((c, 1, hh, ww)) * 30 + 7).astype(np.float32)
        special = np.array([-50.0, 60.0, -50.000004, 60.000004, -0.0, 1e-45, -1e-45, 1e-39], np.float32)
        hit = rng.random(core.shape) < 0.05
        core[hit] = rng.choice(special, int(hit.sum()))
    core[:, :, rng.random((hh, ww)) >= keep] = 0
    core[rng.random(core.shape) < 0.05] = 0                           # ... and zeros of one channel alone: the mask is "non-zero in ANY channel"
    if hh > 4:
        core[:, :, hh // 2] = 0
    core[:, :, 0, 0] = 1.0; core[:, :, -1, -1] = 2.0                  # the box is the border's
    data = np.zeros((c, 1, h, w), np.float32)
    data[:, :, t:h - b, l:w - r] = core
    return data


def _setup(kind, c):
    ids, masked = KINDS[kind]
    return [ids[i % len(ids)] for i in range(c)], [masked] * c


def _check(data, kind, out_hw=None):
    schemes, use_mask = _setup(kind, data.shape[0])
    box, want, status = case_statement(data, schemes, use_mask, FIP)
    assert status == 0, (kind, status)
    with P.DevicePlanes(data, 0) as p:
        assert p.crop_normalize(schemes, use_mask, FIP) == box and p.status == 0 and p.shape == want.shape
        got = p.download()
        diff = bits(got) != bits(want)
        assert not diff.any(), (kind, data.shape, box, int(diff.sum()), np.argwhere(diff)[:4])
        for c, s in enumerate(schemes):
            plane = np.ascontiguousarray(data[c, 0, box[1][0]:box[1][1], box[2][0]:box[2][1]])
            if s == Z:
                sel = plane[np.any(data[:, 0, box[1][0]:box[1][1], box[2][0]:box[2][1]] != 0, axis=0)] if use_mask[c] else plane
                assert np.array_equal(bits(p.stats[c]), bits(np.array(P.zscore_stats_f32_statement(sel)[:2]))), (kind, c)
            elif s == CT:
                assert np.array_equal(bits(p.stats[c]), bits(P.ct_f32_parameters(FIP[str(c)])[:2]))
            elif s == RS:
                assert bits(p.stats[c, 0]) == bits(plane.min()) and bits(p.stats[c, 1]) == bits(max(np.float32(plane.max() - plane.min()), np.float32(1e-8)))
            else:
                assert p.stats[c].tolist() == ([0.0, 255.0] if s == RGB else [0.0, 1.0])
        if out_hw is not None:                       # the clip bounds the handle kept are the planes' minimum and maximum: the resample shows them
            res = P.resample_planes_cubic_device(p, out_hw, 0)
            assert res.shape == (data.shape[0], 1) + tuple(out_hw)
            for c in range(data.shape[0]):
                assert np.array_equal(bits(res[c, 0]), bits(P.resize_cubic_f64(want[c, 0], out_hw))), (kind, out_hw, c)
    return got


# (2, 130, 127): more than two chunks of 8192; with keep = 0.55 / 0.45 the masked count lies above / below one chunk
@pytest.mark.parametrize('c,h,w,border,keep', [(1, 3, 5, (0, 0, 0, 0), 0.8), (2, 9, 7, (1, 0, 0, 2), 0.8), (1, 91, 91, (0, 0, 0, 0), 0.8), (3, 64, 128, (0, 0, 0, 0), 0.8),
                                               (2, 130, 127, (0, 0, 0, 0), 0.55), (2, 130, 127, (3, 1, 0, 2), 0.45), (2, 40, 33, (0, 0, 0, 0), 0.004)])
def test_handle_equals_the_statements_bit_for_bit(c, h, w, border, keep):
    for kind in KINDS:
        data = _data(h * w + c, c, h, w, kind, border, keep)
        if kind == 'masked':
            n_m = int(np.any(data != 0, axis=0).sum())
            assert (n_m > 8192) == (keep == 0.55) and (n_m < 8) == (keep < 0.01), n_m
        _check(data, kind)


@pytest.mark.parametrize('hw,out', [((90, 77), (150, 103)), ((33, 47), (80, 21))])
def test_resample_up_and_down_on_the_handle_equals_the_statement_after_each_scheme(hw, out):
    for kind in KINDS:
        _check(_data(hw[0], 2, hw[0] + 9, hw[1] + 4, kind, border=(4, 5, 1, 3)), kind, out)


def test_clip_edges_signed_zeros_and_a_constant_plane():
    edge = np.array([-0.0, 0.0, -1e-45, 1e-45, -1.0, 5.0, 3.0, -3.0, 1e30, -1e30, 2.9999998, 0.5], np.float32)
    data = np.tile(edge, 30).reshape(1, 1, 20, 18)
    for lo, hi in ((0.0, 3.0), (-0.0, 3.0), (-3.0, 0.0), (-3.0, -0.0), (0, 3), (3.0, -3.0)):
        fip = {'0': {'percentile_00_5': lo, 'percentile_99_5': hi, 'mean': 0.0, 'std': 1.0}}
        want = P.ct_f32_statement(data[0, 0], fip['0'])
        with P.DevicePlanes(data, 0) as p:
            assert p.crop_normalize([CT], [False], fip) is not None
            assert np.array_equal(bits(p.download()[0, 0]), bits(want)), (lo, hi)
    const = np.full((2, 1, 70, 90), np.float32(-3.25), np.float32)
    got = _check(const, 'rescale')
    assert not got.any() and not np.signbit(got).any()
    _check(np.abs(_data(3, 2, 70, 90, 'ct')) + np.float32(1e-3), 'rescale')          # no zero at all: the minimum is positive


def test_two_runs_give_the_same_bytes():
    for kind in ('masked', 'ct + z-score + rescale'):
        data = _data(11, 3, 300, 260, kind, border=(0, 10, 10, 0), keep=0.6)
        schemes, use_mask = _setup(kind, 3)
        runs = []
        for _ in range(2):
            with P.DevicePlanes(data, 0) as p:
                assert p.crop_normalize(schemes, use_mask, FIP) is not None
                runs.append((p.download().tobytes(), p.stats.tobytes(), p.resample((170, 333)).download().tobytes()))
        assert runs[0] == runs[1]


def test_each_status_is_set_and_nothing_faults():
    def status(data, schemes, use_mask=None):
        with P.DevicePlanes(data, 0) as p:
            assert p.crop_normalize(schemes, use_mask or [False] * len(schemes), FIP) is None
            with pytest.raises(RuntimeError, match='clip bounds'):          # nothing usable stays on the handle
                p.resample((10, 10))
            return p.status
    for kind, (ids, masked) in KINDS.items():
        data = _data(12, 2, 50, 40, kind)
        data[1, 0, 20, 20] = np.nan
        assert status(data, *_setup(kind, 2)) & P.PLANES_NONFINITE, kind
    rgb = _data(13, 2, 50, 40, 'rgb')
    rgb[1, 0, 49, 39] = 256
    assert status(rgb, [RGB, RGB]) == P.PLANES_RGB_RANGE
    rgb[1, 0, 49, 39] = -1e-45
    assert status(rgb, [RGB, RGB]) == P.PLANES_RGB_RANGE
    assert status(np.zeros((2, 1, 33, 47), np.float32), [Z, Z], [True, True]) == P.PLANES_EMPTY_MASK
    neg = np.abs(_data(14, 1, 30, 30, 'ct')); neg[0, 0, 3, 3] = -0.0
    assert status(neg, [RS]) == P.PLANES_ZERO_SIGN
    assert status(np.full((1, 1, 8, 8), 3e38, np.float32) * np.array([1, -1] * 4, np.float32), [RS]) == P.PLANES_NONFINITE      # max - min overflows
    from totalsegmentator2d_amd import _lib
    with P.DevicePlanes(rgb, 0) as p:
        ids, par, msk, st = np.array([0, 7], np.int32), np.zeros((2, 4), np.float32), np.zeros(2, np.uint8), np.zeros((2, 2), np.float32)
        import ctypes
        box, code = (ctypes.c_int32 * 4)(), ctypes.c_int()
        assert p._lib.ts2d_planes_crop_normalize(p._h, ids.ctypes.data, par.ctypes.data, msk.ctypes.data, ctypes.byref(box), st.ctypes.data, ctypes.byref(code)) == -1
        assert 'ts2d_planes_crop_normalize: plane 1 has the unknown scheme 7' in _lib.last_error()
        ids[1], par[1, 2] = 1, np.inf
        assert p._lib.ts2d_planes_crop_normalize(p._h, ids.ctypes.data, par.ctypes.data, msk.ctypes.data, ctypes.byref(box), st.ctypes.data, ctypes.byref(code)) == -1
        assert 'non-finite CT parameter' in _lib.last_error()


# ------------------------------------------------------------------------------------------------ surface
def _model(mid, heads, seed, multilabel):
    arch = cases.unet(3, (32, 32, 64), heads, cin=2)
    blob = weights.pack_blob(arch, weights.synthetic_state_dict(arch, seed))
    n_labels = heads if multilabel else heads - 1                      # a label-map model has a head for the background
    ds = {'channel_names': {'0': 'mean', '1': 'max'}, 'labels': {'background': 0, **{f'l{i + 1}': i + 1 for i in range(n_labels)}}, 'file_ending': '.nrrd'}
    if multilabel:
        ds['multilabel'] = True
    return HIPModel({'model': mid, 'revision': 1, 'param': {'nnu.predict.augment': True},
                     'synthetic': {'arch': arch, 'blobs': [blob], 'patch_size': (64, 64), 'dataset_json': ds}})


def _image(seed, hw, spacing, border):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(hw + (2,)) * 200 + 50).astype(np.float32)
    a[rng.random(hw) < 0.1] = 0                                       # zeros in the interior: the mask is not the box
    a[:border] = 0; a[:, -border:] = 0
    return nrrd.Image(a, spacing, (3.0, -7.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


@pytest.mark.parametrize('which', ['ct label map', 'masked z-score multilabel'])
def test_apply_and_apply_batch_are_byte_identical_with_the_switch_on_and_off(monkeypatch, which):
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    entered = []
    orig = P.DevicePlanes.crop_normalize
    monkeypatch.setattr(P.DevicePlanes, 'crop_normalize', lambda self, *a: (entered.append(self.shape), orig(self, *a))[1])
    model = _model('ts2d-test_' + which.split()[0], 4, 51, multilabel='multilabel' in which)
    model.start()
    try:
        p = model._predictor
        if which.startswith('ct'):
            p.configuration_manager.normalization_schemes = [CT, CT]
            p.plans_manager.plans = {'foreground_intensity_properties_per_channel': {'0': {'percentile_00_5': -300.0, 'percentile_99_5': 420.5, 'mean': 48.0, 'std': 190.0},
                                                                                     '1': {'percentile_00_5': -250, 'percentile_99_5': 400, 'mean': 52.5, 'std': 201.25}}}
        else:
            p.configuration_manager.use_mask_for_norm = [True, True]
        assert model.device_input_normalize_schemes is True and model.multilabel == ('multilabel' in which)
        imgs = {'plan': _image(1, (90, 80), (1.5, 1.5), 3), 'off': _image(2, (110, 97), (0.9, 1.2), 5)}      # on and off the plan spacing
        out = {}
        for on in (True, False):
            model.device_input_normalize_schemes = on
            del entered[:]
            pre = {n: model._preprocess_input(i) for n, i in imgs.items()}
            out[on] = (pre, {n: model.apply(i) for n, i in imgs.items()}, model.apply_batch(dict(imgs)))
            assert len(entered) == (3 * len(imgs) if on else 0)
        for n in imgs:
            (_, d_on, p_on), (_, d_off, p_off) = out[True][0][n], out[False][0][n]
            assert d_on.shape == d_off.shape and np.array_equal(bits(d_on), bits(d_off)) and p_on == p_off and 'device_normalize_schemes' not in p_on, n
            for k in (1, 2):
                assert np.array_equal(out[True][k][n].array, out[False][k][n].array) and out[True][k][n].meta == out[False][k][n].meta, n
            assert out[True][1][n].array.any(), n
    finally:
        model.stop()
