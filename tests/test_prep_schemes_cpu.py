"""Every nnU-Net normalisation scheme on the device-resident planes (csrc/kernels_prep_schemes.h) as far as it goes without a GPU: the numpy
statements of the arithmetic (preprocess.ct_f32_statement, rescale01_f32_statement, rgb01_f32_statement, masked_zscore_f32_statement) pinned bit for
bit to preprocess.normalize_channel, the C-ABI of ts2d_planes_crop_normalize (header, export, binding, validation before any device work) and the
routing of ``DefaultPreprocessor.run_case_npy`` with a stand-in for the handle."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests.prep_schemes_util import CT_PROPS, SchemesStandInLib, bits, case_statement, planes_of_every_kind
from tests.test_prep_cpu import _case, _run, _same
from totalsegmentator2d_amd import _lib
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.model import HIPModel

SHAPES = [(1, 1), (1, 7), (3, 5), (7, 11), (13, 127), (64, 128), (129, 131), (90, 77), (600, 512)]


def _host(plane, scheme, props=None, mask=None):
    with np.errstate(all='ignore'):
        return P.normalize_channel(plane[None], scheme, mask is not None, None if mask is None else mask[None], props)[0]


def _equal(got, ref, what):
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    diff = bits(got) != bits(ref)
    assert not diff.any(), (what, int(diff.sum()))


# ------------------------------------------------------------------------------------------------ statements
def test_ct_statement_is_normalize_channel_bit_for_bit():
    rng = np.random.default_rng(21)
    props = [CT_PROPS, dict(CT_PROPS, percentile_00_5=-50, percentile_99_5=60, mean=5, std=20),            # bounds (and moments) given as ints
             dict(CT_PROPS, percentile_00_5=0.0, percentile_99_5=0.1), dict(CT_PROPS, percentile_00_5=-0.0, percentile_99_5=1e-40),
             dict(CT_PROPS, percentile_00_5=-1e-3, percentile_99_5=0.0), dict(CT_PROPS, std=0.0), dict(CT_PROPS, std=1e-9, mean=0.1),
             {'percentile_00_5': -1003.7, 'percentile_99_5': 1546.25, 'mean': 101.3307, 'std': 76.9153},
             dict(CT_PROPS, percentile_00_5=60.0, percentile_99_5=-50.0)]                                  # bounds in the wrong order: the upper one everywhere
    for h, w in SHAPES:
        for name, a in planes_of_every_kind(rng, h, w):
            for pr in props:
                _equal(P.ct_f32_statement(a, pr), _host(a, 'CTNormalization', pr), (h, w, name, pr))
    # what clip does at the edges, written down in the statement's docstring
    edge = np.array([np.nan, -0.0, 0.0, -1e-45, 1e-45, -1.0, 5.0, np.inf, -np.inf], np.float32)
    flat = dict(CT_PROPS, mean=0.0, std=1.0)
    got = P.ct_f32_statement(edge, dict(flat, percentile_00_5=0.0, percentile_99_5=3.0))
    assert np.array_equal(bits(got), bits(np.array([np.nan, -0.0, 0.0, 0.0, 1e-45, 0.0, 3.0, 3.0, 0.0], np.float32)))
    _equal(got, _host(edge, 'CTNormalization', dict(flat, percentile_00_5=0.0, percentile_99_5=3.0)), 'edge')
    got = P.ct_f32_statement(edge, dict(flat, percentile_00_5=-3.0, percentile_99_5=-0.0))
    assert np.array_equal(bits(got), bits(np.array([np.nan, -0.0, 0.0, -1e-45, -0.0, -1.0, -0.0, -0.0, -3.0], np.float32)))
    # a bound that is not finite in float32: an infinity clips nothing, a NaN makes every sample NaN - numpy's, and not the device's business
    for lo, hi in ((-1e40, 1e40), (-np.inf, 3.0), (np.nan, 3.0), (-3.0, np.nan)):
        pr = dict(flat, percentile_00_5=lo, percentile_99_5=hi)
        _equal(P.ct_f32_statement(edge, pr), _host(edge, 'CTNormalization', pr), (lo, hi))
        assert not np.isfinite(P.ct_f32_parameters(pr)).all()
    assert np.isnan(P.ct_f32_statement(edge, dict(flat, percentile_00_5=np.nan, percentile_99_5=3.0))).all()
    par = P.ct_f32_parameters(dict(CT_PROPS, std=1e-9))
    assert par.dtype == np.float32 and bits(par[1]) == bits(np.float32(1e-8)) and bits(P.ct_f32_parameters(CT_PROPS)[1]) == bits(np.float32(20.0))


def test_rescale_and_rgb_and_none_statements_are_normalize_channel_bit_for_bit():
    rng = np.random.default_rng(22)
    for h, w in SHAPES:
        for name, a in planes_of_every_kind(rng, h, w):
            got = P.rescale01_f32_statement(a)
            _equal(got, _host(a, 'RescaleTo01Normalization'), (h, w, name))
            if name in ('constant', 'zero', 'negative zero'):
                assert not got.any(), name                                         # a constant plane gives zeros
            with np.errstate(all='ignore'):                                        # the divisor from the two bounds of the plane: what the device derives
                d = np.float32(a.max() - a.min())
                assert bits((a - a.min()).max()) == bits(d) or d == 0, (h, w, name)
            if a.min() < 0 or a.max() > 255:
                for fn in (lambda: P.rgb01_f32_statement(a), lambda: _host(a, 'RGBTo01Normalization')):
                    with pytest.raises(RuntimeError, match=r'outside \[0, 255\]'):
                        fn()
            else:
                _equal(P.rgb01_f32_statement(a), _host(a, 'RGBTo01Normalization'), (h, w, name))
    nan = np.array([[1.0, np.nan, 3.0]], np.float32)                               # a NaN passes upstream's range check and comes out a NaN
    _equal(P.rgb01_f32_statement(nan), _host(nan, 'RGBTo01Normalization'), 'nan')
    _equal(P.rescale01_f32_statement(nan), _host(nan, 'RescaleTo01Normalization'), 'nan')
    edge = np.array([[0.0, -0.0, 255.0, 1e-45, 254.99998]], np.float32)
    _equal(P.rgb01_f32_statement(edge), _host(edge, 'RGBTo01Normalization'), 'edge')


# masked counts on both sides of every branch of the pairwise sum: < 8 sequential, one leaf, the first split, one chunk, chunks and a tail
MASKED_COUNTS = (1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 8192 + 129, 2 * 8192 + 5)


@pytest.mark.parametrize('n_m', MASKED_COUNTS)
def test_masked_zscore_statement_is_normalize_channel_bit_for_bit(n_m):
    rng = np.random.default_rng(n_m)
    w = 131
    h = -(-n_m // w) * 2 + 7                                   # room for zeros in the interior and for whole zero rows inside the box
    for name, a in planes_of_every_kind(rng, h, w):
        if name in ('zero', 'negative zero'):
            continue
        mask = np.zeros(h * w, bool)
        mask[rng.choice(np.arange(w, h * w - w), n_m - min(n_m, 2), replace=False)] = True
        mask = mask.reshape(h, w)
        mask[0, 0] = True
        mask[h - 1, w - 1] = n_m > 1                            # the box is the whole plane
        mask[3] = False; mask[h // 2] = False                   # whole zero rows inside it
        short = n_m - int(mask.sum())
        free = np.flatnonzero(~mask.reshape(-1))
        free = free[(free // w != 3) & (free // w != h // 2) & (free > 0) & (free < h * w - 1)]
        mask.reshape(-1)[free[:short]] = True
        assert int(mask.sum()) == n_m and not mask[3].any()
        a = np.where(a == 0, np.float32(1.0), a)                # (the mask is the plane's own non-zero pattern)
        plane = np.where(mask, a, np.float32(0.0))
        got = P.masked_zscore_f32_statement(plane, mask)
        _equal(got, _host(plane, 'ZScoreNormalization', mask=mask), (n_m, name))
        assert not got[~mask].any() and np.array_equal(bits(P.zscore_stats_f32_statement(plane[mask])[0]), bits(plane[mask].mean()))
    with pytest.raises(ValueError, match='mask is empty'):
        P.masked_zscore_f32_statement(np.zeros((3, 3), np.float32), np.zeros((3, 3), bool))


# ------------------------------------------------------------------------------------------------ C-ABI
def test_the_entry_is_declared_exported_bound_and_optional_and_the_abi_is_still_9():
    hdr = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r'int\s+ts2d_planes_crop_normalize\s*\(([^)]*)\)\s*;', hdr)
    assert m and [' '.join(p.split()) for p in m.group(1).split(',')] == ['ts2d_planes* p', 'const int32_t* schemes', 'const float* params', 'const uint8_t* use_mask',
                                                                         'int32_t box[4]', 'float* stats', 'int* status']
    for name, value in (('TS2D_NORM_ZSCORE', 0), ('TS2D_NORM_CT', 1), ('TS2D_NORM_RESCALE01', 2), ('TS2D_NORM_RGB01', 3), ('TS2D_NORM_NONE', 4),
                        ('TS2D_PLANES_NONFINITE', P.PLANES_NONFINITE), ('TS2D_PLANES_RGB_RANGE', P.PLANES_RGB_RANGE), ('TS2D_PLANES_EMPTY_MASK', P.PLANES_EMPTY_MASK),
                        ('TS2D_PLANES_ZERO_SIGN', P.PLANES_ZERO_SIGN)):
        assert re.search(rf'#define {name} {value}\b', hdr), name
    assert [P.NORM_SCHEME_IDS[s] for s in ('ZScoreNormalization', 'CTNormalization', 'RescaleTo01Normalization', 'RGBTo01Normalization', 'NoNormalization')] == [0, 1, 2, 3, 4]
    assert 'ts2d_planes_crop_normalize' in _lib.OPTIONAL and _lib.ABI_VERSION == 9
    raw = open(_lib.HEADER_PATH).read()
    doc = raw[:raw.index('int ts2d_planes_crop_normalize(')]
    assert 'prediction_worker.py:194-199' in doc[doc.rindex('/* crop_to_nonzero'):]
    lib = _lib.load()
    c = ctypes
    fn = lib.ts2d_planes_crop_normalize
    assert fn.restype is c.c_int and fn.argtypes == [c.c_void_p] * 4 + [c.POINTER(c.c_int32 * 4), c.c_void_p, c.POINTER(c.c_int)] and lib.ts2d_abi_version() == 9
    box, status = (c.c_int32 * 4)(), c.c_int()
    a = np.zeros(8, np.float32)
    assert fn(None, a.ctypes.data, a.ctypes.data, a.ctypes.data, c.byref(box), a.ctypes.data, c.byref(status)) == -1       # no GPU is needed: refused before any device work
    assert 'ts2d_planes_crop_normalize: null' in _lib.last_error()


# ------------------------------------------------------------------------------------------------ routing
FIP = {'0': CT_PROPS, '1': dict(CT_PROPS, mean=-3, std=11.5)}
ON = {'device_normalize_schemes': 2}


def _stand(monkeypatch, **kw):
    stand = SchemesStandInLib(fip=FIP, **kw)
    monkeypatch.setattr(P, 'planes_device_entries', lambda: stand)
    monkeypatch.setattr(P, 'cubic_device_entry', lambda: None)
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    return stand


def _rgb_case(seed, c, h, w, border):
    d = _case(seed, c, h, w, border)
    return np.where(d != 0, np.abs(d) % 256, d).astype(np.float32)


CASES = [('CT', dict(schemes=['CTNormalization'] * 2), _case),
         ('CT + z-score', dict(schemes=['CTNormalization', 'ZScoreNormalization']), _case),
         ('masked z-score', dict(use_mask=[True, True]), _case),
         ('masked + plain z-score', dict(use_mask=[False, True]), _case),
         ('rescale', dict(schemes=['RescaleTo01Normalization'] * 2), _case),
         ('rgb', dict(schemes=['RGBTo01Normalization'] * 2), _rgb_case),
         ('none + rescale', dict(schemes=['NoNormalization', 'RescaleTo01Normalization']), _case),
         ('none', dict(schemes=['NoNormalization'] * 2), _case)]


@pytest.mark.parametrize('name,kw,make', CASES, ids=[c[0] for c in CASES])
def test_run_case_npy_takes_the_new_key_and_returns_the_same_bytes_and_properties(monkeypatch, name, kw, make):
    stand = _stand(monkeypatch)
    kw = dict(kw, plans={'foreground_intensity_properties_per_channel': FIP})
    data = make(31, 2, 60, 45, border=(3, 0, 5, 2))
    data[:, 0, 20:23] = 0; data[:, 0, 30, 7:19] = 0                  # zeros in the interior of the box, whole zero rows among them
    host = _run(data, (1.5, 1.5), {}, **kw)
    assert stand.calls == []
    dev = _run(data, (1.5, 1.5), ON, **kw)
    assert stand.calls == [('create', 2, 2, 60, 45), ('crop_normalize',), ('download',), ('destroy',)]
    assert _same(dev, host) and 'device_normalize_schemes' not in dev[1] and dev[1]['bbox_used_for_cropping'] == [[0, 1], [3, 60], [5, 43]]
    # off the plan spacing: the resample happens on the handle
    del stand.calls[:]
    host = _run(data, (1.0, 0.8), {}, **kw)
    dev = _run(data, (1.0, 0.8), dict(ON, device_resample=2, device_normalize=2), **kw)     # (the old key beside it: its predicate refuses these cases)
    assert stand.calls == [('create', 2, 2, 60, 45), ('crop_normalize',), ('resample', 38, 20), ('download',), ('destroy',)] and _same(dev, host)
    # a z-score from the projection that can never apply does not bar the route
    del stand.calls[:]
    dz = {'shape': (60, 45), 'order': (0, 1), 'box': (0, 59, 0, 44), 'norm': np.zeros((2, 60, 45), np.float32)}
    assert _same(_run(data, (1.5, 1.5), dict(ON, device_zscore=dz), **kw), _run(data, (1.5, 1.5), {}, **kw)) and len(stand.calls) == 4
    assert not stand.planes


@pytest.mark.filterwarnings('ignore:Mean of empty slice', 'ignore:Degrees of freedom')        # (numpy's words for the image of zeros below)
def test_each_status_falls_back_to_the_host_route_and_destroys_the_handle(monkeypatch):
    stand = _stand(monkeypatch)
    plans = {'foreground_intensity_properties_per_channel': FIP}
    three = [('create', 2, 2, 40, 30), ('crop_normalize',), ('destroy',)]
    data = _case(32, 2, 40, 30, border=(0, 3, 0, 0))
    nan = data.copy(); nan[1, 0, 7, 7] = np.nan
    for kw in (dict(schemes=['CTNormalization'] * 2, plans=plans), dict(use_mask=[True, True]), dict(schemes=['NoNormalization', 'RescaleTo01Normalization'])):
        dev, host = _run(nan, (1.5, 1.5), ON, **kw), _run(nan, (1.5, 1.5), {}, **kw)
        assert np.array_equal(dev[0], host[0], equal_nan=True) and dev[1] == host[1] and stand.calls == three and not stand.planes, kw
        del stand.calls[:]
    # an RGB sample of 256: the host route raises upstream's message
    rgb = _rgb_case(33, 2, 40, 30, (0, 3, 0, 0)); rgb[0, 0, 5, 5] = 256
    with pytest.raises(RuntimeError, match=r'RGB images are uint 8, for whatever reason I found pixel values outside \[0, 255\]'):
        _run(rgb, (1.5, 1.5), ON, schemes=['RGBTo01Normalization'] * 2)
    assert stand.calls == three and not stand.planes
    del stand.calls[:]
    # an image of zeros under a masked scheme: numpy's NaN of an empty mean, not the device's
    zero = np.zeros((2, 1, 40, 30), np.float32)
    dev, host = _run(zero, (1.5, 1.5), ON, use_mask=[True, True]), _run(zero, (1.5, 1.5), {}, use_mask=[True, True])
    assert np.array_equal(dev[0], host[0], equal_nan=True) and dev[1] == host[1] and stand.calls == three
    del stand.calls[:]
    # a Rescale plane whose minimum is -0.0
    neg = np.abs(data); neg[0, 0, 4, 4] = -0.0
    kw = dict(schemes=['RescaleTo01Normalization'] * 2)
    assert _same(_run(neg, (1.5, 1.5), ON, **kw), _run(neg, (1.5, 1.5), {}, **kw)) and stand.calls == three
    assert case_statement(neg, kw['schemes'], [0, 0], None)[2] == P.PLANES_ZERO_SIGN
    # every bit alone, whatever raised it
    for bit in (P.PLANES_NONFINITE, P.PLANES_RGB_RANGE, P.PLANES_EMPTY_MASK, P.PLANES_ZERO_SIGN):
        forced = _stand(monkeypatch, force_status=bit)
        kw = dict(schemes=['CTNormalization'] * 2, plans=plans)
        assert _same(_run(data, (1.5, 1.5), ON, **kw), _run(data, (1.5, 1.5), {}, **kw)) and forced.calls == three and not forced.planes


def test_without_the_key_or_the_symbol_or_eligibility_no_call_is_made(monkeypatch):
    stand = _stand(monkeypatch)
    plans = {'foreground_intensity_properties_per_channel': FIP}
    data = _case(34, 2, 40, 30, border=(2, 2, 2, 2))
    ct = dict(schemes=['CTNormalization', 'ZScoreNormalization'], plans=plans)

    def quiet(d, on, **kw):
        assert _same(_run(d, (1.5, 1.5), on, **kw), _run(d, (1.5, 1.5), {}, **kw)) and stand.calls == [], kw
    quiet(data, {}, **ct)
    quiet(data, {'device_normalize': 0}, **ct)                                    # the old key alone keeps these cases on the host
    quiet(data, ON, tf=(0, 2, 1), **ct)
    quiet(_case(5, 2, 40, 30)[:, 0].reshape(2, 4, 10, 30), ON, **ct)              # Z > 1
    with pytest.raises(RuntimeError, match='CTNormalization needs'):              # no intensity properties for channel 1: the host route says so
        _run(data, (1.5, 1.5), ON, schemes=['CTNormalization'] * 2, plans={'foreground_intensity_properties_per_channel': {'0': CT_PROPS}})
    assert stand.calls == []
    for bad in (dict(CT_PROPS, percentile_99_5=1e40), dict(CT_PROPS, mean=np.float64(5.0)), dict(CT_PROPS, percentile_00_5=np.nan)):
        with np.errstate(all='ignore'):
            quiet(data, ON, schemes=['CTNormalization', 'ZScoreNormalization'], plans={'foreground_intensity_properties_per_channel': {'0': bad}})
    wide = np.ones((1, 1, 1, P.CUBIC_MAX_EXTENT + 1), np.float32); wide[0, 0, 0, ::2] = 3
    quiet(wide, ON, schemes=['NoNormalization'])
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', data.size + 1)
    quiet(data, ON, **ct)
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    # a plain z-score case belongs to the old key: the new one alone makes no call, both make the old route's calls
    quiet(data, ON)
    assert _same(_run(data, (1.5, 1.5), dict(ON, device_normalize=0)), _run(data, (1.5, 1.5), {}))
    assert stand.calls == [('create', 0, 2, 40, 30), ('crop_zscore',), ('download',), ('destroy',)]
    del stand.calls[:]
    # a scheme the table does not know: the host route raises as before
    with pytest.raises(NotImplementedError, match='FancyNormalization'):
        _run(data, (1.5, 1.5), ON, schemes=['FancyNormalization'] * 2)
    assert stand.calls == []
    # a library built before the entry
    class Old:
        def __getattr__(self, name):
            if name == 'ts2d_planes_crop_normalize':
                raise AttributeError(name)
            return getattr(stand, name)
    monkeypatch.setattr(P, 'planes_device_entries', lambda: Old())
    quiet(data, ON, **ct)
    monkeypatch.setattr(P, 'planes_device_entries', lambda: None)
    quiet(data, ON, **ct)


# ------------------------------------------------------------------------------------------------ the switch
def test_the_switch_sets_its_own_key_and_the_preprocess_key_tells_it():
    m = HIPModel.__new__(HIPModel)
    m._discover = lambda: None
    HIPModel.__init__(m, {'param': {}})
    assert m.device_input_normalize_schemes is True and m.device_input_normalize is True
    p = SimpleNamespace(configuration_manager=SimpleNamespace(spacing=[1.5, 1.5]), plans_manager=SimpleNamespace(), dataset_json={})
    key = HIPModel._preprocess_key
    assert key(p, {}) != key(p, {'device_normalize_schemes': 0}) != key(p, {'device_normalize': 0})
    assert key(p, {'device_normalize_schemes': 0}) == key(p, {'device_normalize_schemes': 0}) != key(p, {'device_normalize_schemes': 1})
