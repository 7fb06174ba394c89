"""Slice stacks (a 3-D volume through a 2-D model) as far as they go without a GPU: the numpy statements behind ts2d_planes_crop_normalize_stack - the
box over three axes, every unmasked scheme over the flattened channel - pinned to ``crop_to_nonzero`` and ``normalize_channel``, the C-ABI of the two
new entries, the routing of ``DefaultPreprocessor.run_case_npy`` under the key ``device_normalize_stack`` with a stand-in for the handle, and the
routing of ``HIPModel._run`` to the predictor's stack methods with a host double."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests.prep_schemes_util import CT_PROPS, bits
from tests.stack_util import StackStandInLib, stack_case, stack_statement, volume_statement
from tests.test_prep_cpu import _same
from totalsegmentator2d_amd import _lib, nrrd
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.model import HIPModel

UNMASKED = ('ZScoreNormalization', 'CTNormalization', 'RescaleTo01Normalization', 'RGBTo01Normalization', 'NoNormalization')


# ------------------------------------------------------------------------------------------------ statements
def _box_equals_upstream(data):
    box = P.crop_box3_statement(data)
    assert box == P.crop_to_nonzero(data)[1] and all(type(v) is int for b in box for v in b), box
    return box


def test_crop_box3_statement_is_crop_to_nonzero():
    shape = (2, 9, 20, 17)
    rng = np.random.default_rng(3)
    data = np.zeros(shape, np.float32)
    data[1, 2:7, 3:15, 4:11] = rng.standard_normal((5, 12, 7))                      # content in one channel only
    data[1, 3:5, 6:9, 6:9] = 0                                                       # ... with a hole the upstream mask fills
    assert _box_equals_upstream(data) == [[2, 7], [3, 15], [4, 11]]
    for ax in range(3):                                                              # a lone voxel sets each of the six bounds
        for far in (False, True):
            d = data.copy()
            at = [4, 8, 7]
            at[ax] = shape[1 + ax] - 1 if far else 0
            d[(0,) + tuple(at)] = 1e-45
            want = [[2, 7], [3, 15], [4, 11]]
            want[ax] = [want[ax][0], shape[1 + ax]] if far else [0, want[ax][1]]
            assert _box_equals_upstream(d) == want, (ax, far)
    d = data.copy(); d[0, 8, 19, 16] = np.nan                                        # a NaN counts
    assert _box_equals_upstream(d) == [[2, 9], [3, 20], [4, 17]]
    d = data.copy(); d[0, 0, 0, 0] = -0.0; d[1, 8, 19, 16] = -0.0                    # -0.0 does not
    assert _box_equals_upstream(d) == [[2, 7], [3, 15], [4, 11]]
    zeros = np.zeros(shape, np.float32); zeros[0, 1, 1, 1] = -0.0                    # all zeros: the whole extent
    assert _box_equals_upstream(zeros) == [[0, 9], [0, 20], [0, 17]]
    with pytest.raises(ValueError, match='crop_box3_statement'):
        P.crop_box3_statement(np.zeros((2, 3, 4), np.float32))


@pytest.mark.parametrize('shape', [(3, 61, 47), (7, 131, 97)])      # 8601 samples: one full chunk + a tail, the chunk boundary inside the last slice; 88 942
@pytest.mark.parametrize('scheme', UNMASKED)
def test_flattened_statements_are_normalize_channel_on_the_cropped_view(shape, scheme):
    z, h, w = shape
    assert shape != (3, 61, 47) or 2 * h * w < P.SUM_CHUNK < z * h * w < 2 * P.SUM_CHUNK
    full = stack_case(sum(shape), 1, z + 2, h + 5, w + 3, (1, 1, 2, 3, 3, 0), rgb=scheme == 'RGBTo01Normalization')
    view = full[0, 1:z + 1, 2:h + 2, 3:]                                             # cropped and non-contiguous, as crop_to_nonzero hands it on
    assert view.shape == shape and not view.flags.c_contiguous
    with np.errstate(all='ignore'):
        want = P.normalize_channel(view, scheme, False, None, CT_PROPS)
    got = volume_statement(view, scheme, CT_PROPS)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(bits(got), bits(want))
    if scheme == 'ZScoreNormalization':                                              # ... and NOT the per-slice statement
        assert not np.array_equal(bits(got[0]), bits(P.zscore_f32_statement(view[0])))
        assert np.array_equal(bits(P.zscore_stats_f32_statement(np.ascontiguousarray(view).reshape(1, -1))[0]), bits(np.ascontiguousarray(view).mean()))


# ------------------------------------------------------------------------------------------------ C-ABI
def test_the_entries_are_declared_exported_bound_and_optional_and_the_abi_is_still_9():
    hdr = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r'int\s+ts2d_planes_create_stack\s*\(([^)]*)\)\s*;', hdr)
    assert m and [' '.join(p.split()) for p in m.group(1).split(',')] == ['int device', 'const float* src', 'int channels', 'int slices', 'int h', 'int w', 'ts2d_planes** out']
    m = re.search(r'int\s+ts2d_planes_crop_normalize_stack\s*\(([^)]*)\)\s*;', hdr)
    assert m and [' '.join(p.split()) for p in m.group(1).split(',')] == ['ts2d_planes* p', 'const int32_t* schemes', 'const float* params', 'const uint8_t* use_mask',
                                                                         'int32_t box[6]', 'float* stats', 'int* status']
    assert {'ts2d_planes_create_stack', 'ts2d_planes_crop_normalize_stack'} <= _lib.OPTIONAL and _lib.ABI_VERSION == 9
    lib = _lib.load()
    c = ctypes
    assert lib.ts2d_abi_version() == 9
    assert lib.ts2d_planes_crop_normalize_stack.argtypes == [c.c_void_p] * 4 + [c.POINTER(c.c_int32 * 6), c.c_void_p, c.POINTER(c.c_int)]
    # refused before any device work: no GPU is needed
    a = np.zeros(8, np.float32)
    h = c.c_void_p(0x1234)
    for args, word in (((0, None, 1, 2, 2, 2, c.byref(h)), 'ts2d_planes_create_stack: null argument'),
                       ((0, a.ctypes.data, 1, 0, 2, 2, c.byref(h)), 'ts2d_planes_create_stack: 1 channels of 0 slices outside 1 ... 65535 planes'),
                       ((0, a.ctypes.data, 0, 2, 2, 2, c.byref(h)), 'ts2d_planes_create_stack: 0 channels of 2 slices outside'),
                       ((0, a.ctypes.data, 256, 256, 2, 2, c.byref(h)), '256 channels of 256 slices outside 1 ... 65535 planes'),
                       ((0, a.ctypes.data, 1, 2, 2, 8193, c.byref(h)), 'ts2d_planes_create_stack: extents 2 x 8193 outside 1 ... 8192'),
                       ((0, a.ctypes.data, 1, 1025, 512, 512, c.byref(h)), 'ts2d_planes_create_stack: 1025 planes of 512 x 512 are more than one handle takes (2^28 samples)')):
        h.value = 0x1234
        assert lib.ts2d_planes_create_stack(*args) == -1 and word in _lib.last_error(), (_lib.last_error(), word)
        assert h.value is None                                                       # the handle is cleared, nothing else is written
    box, status = (c.c_int32 * 6)(*[7] * 6), c.c_int(7)
    assert lib.ts2d_planes_crop_normalize_stack(None, a.ctypes.data, a.ctypes.data, a.ctypes.data, c.byref(box), a.ctypes.data, c.byref(status)) == -1
    assert 'ts2d_planes_crop_normalize_stack: null argument' in _lib.last_error() and list(box) == [7] * 6 and status.value == 7


# ------------------------------------------------------------------------------------------------ routing of run_case_npy
FIP = {'0': CT_PROPS, '1': dict(CT_PROPS, mean=-3, std=11.5)}
ON = {'device_normalize_stack': 2}


def _stand(monkeypatch, **kw):
    stand = StackStandInLib(fip=FIP, **kw)
    monkeypatch.setattr(P, 'planes_device_entries', lambda: stand)
    monkeypatch.setattr(P, 'cubic_device_entry', lambda: None)
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    return stand


def _run(data, spacing, props_extra, schemes=None, use_mask=None, tf=(0, 1, 2), plans=None):
    """run_case_npy of a stack: a 3-D image spacing (z, y, x) and a 2-D plan of 1.5 x 1.5 mm."""
    pm = SimpleNamespace(transpose_forward=list(tf), plans=plans or {})
    cm = SimpleNamespace(spacing=[1.5, 1.5], normalization_schemes=schemes or ['ZScoreNormalization'] * data.shape[0],
                         use_mask_for_norm=use_mask or [False] * data.shape[0])
    props = dict({'spacing': (2.5,) + tuple(spacing)}, **props_extra)
    with np.errstate(all='ignore'):
        out, _, props = P.DefaultPreprocessor(verbose=False).run_case_npy(data.copy(), None, props, pm, cm, {})
    return out, props


CASES = [('z-score', {}, False), ('CT + z-score', dict(schemes=['CTNormalization', 'ZScoreNormalization']), False),
         ('rescale + none', dict(schemes=['RescaleTo01Normalization', 'NoNormalization']), False), ('rgb', dict(schemes=['RGBTo01Normalization'] * 2), True)]


@pytest.mark.parametrize('name,kw,rgb', CASES, ids=[c[0] for c in CASES])
def test_run_case_npy_takes_the_stack_key_and_returns_the_same_bytes_and_properties(monkeypatch, name, kw, rgb):
    stand = _stand(monkeypatch)
    kw = dict(kw, plans={'foreground_intensity_properties_per_channel': FIP})
    data = stack_case(41, 2, 4, 10, 30, (1, 0, 2, 0, 3, 4), rgb=rgb)
    data[:, 2, 4:6] = 0                                                              # zeros in the interior of the box
    host = _run(data, (1.5, 1.5), {}, **kw)
    assert stand.calls == []
    dev = _run(data, (1.5, 1.5), ON, **kw)
    assert stand.calls == [('create_stack', 2, 2, 4, 10, 30), ('crop_normalize_stack',), ('download',), ('destroy',)]
    assert _same(dev, host) and 'device_normalize_stack' not in dev[1] and dev[1]['bbox_used_for_cropping'] == [[1, 4], [2, 10], [3, 26]]
    assert dev[1]['shape_after_cropping_and_before_resampling'] == (3, 8, 23) and dev[0].shape == (2, 3, 8, 23)
    # off the plan spacing: the resample happens on the handle, every slice clipped to its own bounds
    del stand.calls[:]
    host = _run(data, (1.0, 0.8), {}, **kw)
    dev = _run(data, (1.0, 0.8), dict(ON, device_resample=2, device_normalize=2, device_normalize_schemes=2), **kw)     # (the old keys beside it: their predicates refuse a stack)
    assert stand.calls == [('create_stack', 2, 2, 4, 10, 30), ('crop_normalize_stack',), ('resample', 5, 12), ('download',), ('destroy',)] and _same(dev, host)
    assert dev[0].shape == (2, 3, 5, 12) and not stand.planes


def test_without_the_key_or_eligibility_no_call_is_made(monkeypatch):
    stand = _stand(monkeypatch)
    plans = {'foreground_intensity_properties_per_channel': FIP}
    data = stack_case(42, 2, 4, 10, 30, (0, 1, 1, 1, 2, 2))

    def quiet(d, on, **kw):
        assert _same(_run(d, (1.5, 1.5), on, **kw), _run(d, (1.5, 1.5), {}, **kw)) and stand.calls == [], kw
    quiet(data, {})
    quiet(data, {'device_normalize': 0, 'device_normalize_schemes': 0, 'device_resample': 0})       # the old keys alone still make no call for Z > 1
    quiet(data, ON, use_mask=[False, True])                                                           # a masked scheme: the 3-D hole filling stays on the host
    quiet(data, ON, schemes=['CTNormalization', 'ZScoreNormalization'], use_mask=[True, True], plans=plans)
    quiet(data, ON, tf=(0, 2, 1))                                                                     # a transposed plan
    quiet(data, ON, tf=(1, 0, 2))
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', data.size + 1)                            # below the size gate
    quiet(data, ON)
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    for bad in (dict(CT_PROPS, percentile_99_5=1e40), dict(CT_PROPS, percentile_00_5=np.nan)):
        with np.errstate(all='ignore'):
            quiet(data, ON, schemes=['CTNormalization', 'ZScoreNormalization'], plans={'foreground_intensity_properties_per_channel': {'0': bad}})
    with pytest.raises(NotImplementedError, match='FancyNormalization'):
        _run(data, (1.5, 1.5), ON, schemes=['FancyNormalization'] * 2)
    assert stand.calls == []
    # a single slice is no stack: the key makes no call there, and a masked CT channel (use_mask is ignored for CT) is no masked scheme
    quiet(data[:, :1], ON)
    assert _same(_run(data, (1.5, 1.5), ON, schemes=['CTNormalization'] * 2, use_mask=[True, True], plans=plans),
                 _run(data, (1.5, 1.5), {}, schemes=['CTNormalization'] * 2, use_mask=[True, True], plans=plans)) and len(stand.calls) == 4
    del stand.calls[:]

    class Old:                                                                       # a library built before the entries
        def __getattr__(self, name):
            if name.endswith('_stack'):
                raise AttributeError(name)
            return getattr(stand, name)
    monkeypatch.setattr(P, 'planes_device_entries', lambda: Old())
    quiet(data, ON)
    monkeypatch.setattr(P, 'planes_device_entries', lambda: None)
    quiet(data, ON)


def test_every_status_bit_falls_back_to_the_host_route_and_destroys_the_handle(monkeypatch):
    stand = _stand(monkeypatch)
    three = [('create_stack', 2, 2, 4, 10, 30), ('crop_normalize_stack',), ('destroy',)]
    data = stack_case(43, 2, 4, 10, 30, (0, 0, 0, 2, 0, 0))
    nan = data.copy(); nan[1, 2, 5, 7] = np.nan
    dev, host = _run(nan, (1.5, 1.5), ON), _run(nan, (1.5, 1.5), {})
    assert np.array_equal(dev[0], host[0], equal_nan=True) and dev[1] == host[1] and stand.calls == three and not stand.planes
    del stand.calls[:]
    rgb = stack_case(44, 2, 4, 10, 30, rgb=True); rgb[0, 3, 5, 5] = 256             # an RGB sample of 256: the host route raises upstream's message
    with pytest.raises(RuntimeError, match=r'RGB images are uint 8, for whatever reason I found pixel values outside \[0, 255\]'):
        _run(rgb, (1.5, 1.5), ON, schemes=['RGBTo01Normalization'] * 2)
    assert stand.calls == [('create_stack', 2, 2, 4, 10, 30), ('crop_normalize_stack',), ('destroy',)] and not stand.planes
    del stand.calls[:]
    neg = np.abs(data); neg[0, 1, 4, 4] = -0.0                                       # a Rescale channel whose minimum is -0.0
    kw = dict(schemes=['RescaleTo01Normalization'] * 2)
    assert _same(_run(neg, (1.5, 1.5), ON, **kw), _run(neg, (1.5, 1.5), {}, **kw)) and stand.calls == three
    assert stack_statement(neg, kw['schemes'])[2] == P.PLANES_ZERO_SIGN
    for bit in (P.PLANES_NONFINITE, P.PLANES_RGB_RANGE, P.PLANES_ZERO_SIGN):         # every bit alone, whatever raised it
        forced = _stand(monkeypatch, force_status=bit)
        assert _same(_run(data, (1.5, 1.5), ON), _run(data, (1.5, 1.5), {})) and forced.calls == three and not forced.planes


def test_the_switches_exist_and_the_preprocess_key_tells_the_stack_key():
    m = HIPModel.__new__(HIPModel)
    m._discover = lambda: None
    HIPModel.__init__(m, {'param': {}})
    assert m.device_input_stack is True and m.device_stack is True
    p = SimpleNamespace(configuration_manager=SimpleNamespace(spacing=[1.5, 1.5]), plans_manager=SimpleNamespace(), dataset_json={})
    key = HIPModel._preprocess_key
    assert key(p, {}) != key(p, {'device_normalize_stack': 0}) != key(p, {'device_normalize_stack': 1}) != key(p, {'device_normalize_schemes': 1})


# ------------------------------------------------------------------------------------------------ routing of HIPModel._run
def _stack_image(seed, z=3, h=38, w=34):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((z, h, w, 2)) * 40 + 10).astype(np.float32)
    return nrrd.Image(a, (1.5, 1.5, 2.5), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), 2, {}, 'left-posterior-superior')


@pytest.mark.parametrize('spacing', [(1.5, 1.5, 2.5), (1.2, 1.7, 2.5)], ids=['on the plan spacing', 'off it'])
def test_run_routes_a_stack_to_the_stack_methods_of_a_predictor_that_has_them(spacing):
    """A host double WITH the stack methods (they decide the map from the double's own logits, as the export's host route does) receives the
    Z = 3 case in `apply` and `apply_batch`; a double whose methods are missing keeps the logits route; the image is the same."""
    from tests.batch_util import synthetic_batch_model
    from totalsegmentator2d_amd.export import SIGMOID_HALF_THRESHOLD
    img = _stack_image(5)
    img = nrrd.Image(img.array, spacing, img.origin, img.direction, img.components, {}, img.space)
    m, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_stack', 3, 77, feats=(8, 16), patch=(32, 32), mirror=False)
    m.start(wait=False)
    try:
        p = m._predictor
        cls = type(p)
        seen = []

        def single(data, out_shape=None):
            data = np.asarray(data)
            assert data.shape[1] == 3 and (out_shape is None or out_shape[0] == 3)
            lg = np.asarray(p.predict_logits_from_preprocessed_data(data)).astype(np.float32)
            if out_shape is not None and tuple(out_shape) != lg.shape[1:]:
                lg = P.resample_data_to_shape(lg, out_shape, order=1)
            seen.append((data.shape, None if out_shape is None else tuple(out_shape)))
            return (lg > SIGMOID_HALF_THRESHOLD).astype(np.uint8)

        class With(cls):
            def predict_stack_from_preprocessed_data(self, data, out_shape=None):
                return single(data, out_shape)

            def predict_stack_from_preprocessed_data_batch(self, datas, out_shapes=None):
                return [single(d, s) for d, s in zip(datas, out_shapes or [None] * len(datas))]

        class Without(cls):
            predict_stack_from_preprocessed_data = None
            predict_stack_from_preprocessed_data_batch = None

        p.__class__ = Without
        want, want_many = m.apply(img), m.apply_batch({'a': img})['a']
        assert not seen
        p.__class__ = cls                                    # the product's own methods answer None without engines: the logits route again
        assert np.array_equal(m.apply(img).array, want.array) and not seen
        p.__class__ = With
        got, got_many = m.apply(img), m.apply_batch({'a': img})['a']
        assert len(seen) == 2 and seen[0] == seen[1] and seen[0][0][:2] == (2, 3) and seen[0][1] == (3, 38, 34)
        for a, b in ((got, want), (got_many, want_many)):
            assert a.array.dtype == np.uint8 and a.array.shape == (3, 38, 34, 3) and np.array_equal(a.array, b.array) and a.meta == b.meta and a.spacing == b.spacing
        assert want.array.any() and not want.array.all()
        m.device_stack = False                               # the switch, and the convention's own switch, keep the logits route
        assert np.array_equal(m.apply(img).array, want.array) and len(seen) == 2
        m.device_stack, m.device_threshold = True, False
        assert np.array_equal(m.apply(img).array, want.array) and len(seen) == 2
    finally:
        m.stop()
