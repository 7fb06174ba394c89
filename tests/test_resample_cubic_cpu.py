"""The device input resample (order 3, csrc/kernels_resample_in.h) as far as it goes without a GPU: the numpy statement of its arithmetic
(preprocess.resize_cubic_f64) pinned to scipy bit for bit, its limits, the C-ABI of ts2d_resample_cubic (header, export, binding,
validation before any device work), the emitted instruction stream of the three kernels (no fused multiply-add, no scratch, no
spills) and the routing of an off-spacing case through ``DefaultPreprocessor.run_case_npy`` with a stand-in for the entry."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests.conftest import ROOT
from totalsegmentator2d_amd import _lib
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.model import HIPModel

HIPCC = '/opt/rocm/bin/hipcc'


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _planes(rng, h, w):
    """N(0,1), integer-valued, high-dynamic-range, constant, and a zero background around a blob (results of -0.0 at the clip bound)."""
    yield rng.standard_normal((h, w)).astype(np.float32)
    yield rng.integers(-1000, 3000, (h, w)).astype(np.float32)
    yield (rng.standard_normal((h, w)) * 10.0 ** rng.uniform(-6, 6, (h, w))).astype(np.float32)
    yield np.full((h, w), np.float32(rng.standard_normal()), np.float32)
    a = np.zeros((h, w), np.float32)
    a[h // 3:h // 3 + max(1, h // 8), w // 3:w // 3 + max(1, w // 8)] = np.float32(700.0)
    yield a


def _shapes(seed, n):
    rng = np.random.default_rng(seed)
    s = [(8, 8, 8, 13), (8, 8, 3, 2), (2, 2, 5, 7), (3, 9, 40, 2), (9, 31, 9, 77), (600, 512, 400, 273), (400, 512, 667, 256), (1000, 512, 400, 239)]
    while len(s) < n:
        s.append(tuple(int(v) for v in rng.integers(8, 300, 4)))
    return s


def test_resize_cubic_f64_is_scipy_bit_for_bit():
    rng = np.random.default_rng(20)
    total = 0
    for h, w, oh, ow in _shapes(21, 30):
        for a in _planes(rng, h, w):
            ref = P.resize_like_skimage(a, (oh, ow), 3)
            got = P.resize_cubic_f64(a, (oh, ow))
            assert got.dtype == np.float32 and got.shape == ref.shape == (oh, ow)
            diff = _bits(got) != _bits(ref)
            assert not diff.any(), ((h, w, oh, ow), int(diff.sum()), float(np.abs(got - ref).max()))
            total += ref.size
    assert total > 3_000_000
    assert _switch_default() is True                      # the statement is bit-exact to scipy, so the switch ships on


def _switch_default():
    m = HIPModel.__new__(HIPModel)
    m._discover = lambda: None
    HIPModel.__init__(m, {'param': {}})
    return m.device_input_resample


def test_coefficients_are_scipys_spline_filter_bit_for_bit():
    from scipy import ndimage as ndi
    rng = np.random.default_rng(3)
    for h, w in ((2, 2), (2, 9), (5, 3), (40, 61), (300, 7)):
        a = (rng.standard_normal((h, w)) * 10.0 ** rng.uniform(-3, 3, (h, w))).astype(np.float32)
        ref = ndi.spline_filter(np.pad(a, P.CUBIC_PAD, mode='edge'), 3, output=np.float64, mode='nearest')
        assert np.array_equal(P.cubic_coefficients_f64(a).view(np.uint64), ref.view(np.uint64)), (h, w)


def test_cubic_axis_taps_against_a_direct_evaluation():
    for n_in, n_out in ((2, 2), (2, 7), (600, 400), (512, 273), (400, 667), (1000, 239), (9, 8192), (8192, 2)):
        start, w = P.cubic_axis_taps(n_in, n_out)
        assert start.shape == (n_out,) and w.shape == (n_out, 4)
        assert start.min() >= 0 and start.max() + 3 <= n_in + 2 * P.CUBIC_PAD - 1
        for o in {0, 1, n_out // 2, n_out - 1}:
            cc = (np.float64(o) + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5 + 12.0
            f = np.floor(cc)
            y = cc - f
            t = 1.0 - y
            want = [t * t * t / 6.0, (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0, (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0]
            want.append(1.0 - want[0] - want[1] - want[2])
            assert start[o] == int(f) - 1 and w[o].tolist() == want, (n_in, n_out, o)
        assert np.allclose(w.sum(1), 1.0, atol=1e-15)


def test_the_limits_raise_by_name():
    a = np.ones((8, 8), np.float32)
    for shape, new in (((1, 8), (4, 4)), ((8, 8), (1, 4)), ((8, 8), (4, P.CUBIC_MAX_EXTENT + 1))):
        with pytest.raises(P.CubicResampleLimit, match='extent'):
            P.resize_cubic_f64(np.ones(shape, np.float32), new)
    for bad in (np.inf, -np.inf, np.nan):
        b = a.copy(); b[3, 4] = bad
        with pytest.raises(P.CubicResampleLimit, match='non-finite'):
            P.resize_cubic_f64(b, (5, 5))
    with pytest.raises(P.CubicResampleLimit, match='2-D'):
        P.resize_cubic_f64(np.ones((2, 8, 8), np.float32), (5, 5))


# ------------------------------------------------------------------------------------------------ C-ABI
def test_entry_is_declared_exported_and_bound_and_the_abi_is_still_9():
    hdr = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r'int\s+ts2d_resample_cubic\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'ts2d_resample_cubic is not declared in include/ts2d_engine.h'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    assert params == ['int device', 'const float* src', 'int n_planes', 'int in_h', 'int in_w', 'int out_h', 'int out_w', 'const float* lo_hi', 'float* dst']
    assert 'ts2d_resample_cubic' in _lib.SYMBOLS and _lib.ABI_VERSION == 9
    lib = _lib.load()
    assert lib.ts2d_abi_version() == 9
    c = ctypes
    assert lib.ts2d_resample_cubic.restype is c.c_int
    assert lib.ts2d_resample_cubic.argtypes == [c.c_int, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p]
    assert P.cubic_device_entry() is not None


def test_entry_refuses_bad_arguments_by_name_before_any_device_work():
    lib = _lib.load()
    src = np.zeros((1, 8, 8), np.float32); dst = np.zeros((1, 5, 5), np.float32); lh = np.array([[0.0, 1.0]], np.float32)
    good = dict(src=src.ctypes.data, n=1, ih=8, iw=8, oh=5, ow=5, lh=lh.ctypes.data, dst=dst.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.ts2d_resample_cubic(0, a['src'], a['n'], a['ih'], a['iw'], a['oh'], a['ow'], a['lh'], a['dst'])
        return rc, _lib.last_error()

    for kw, word in ((dict(src=None), 'null'), (dict(lh=None), 'null'), (dict(dst=None), 'null'), (dict(n=0), 'planes'), (dict(ih=1), 'extents'),
                     (dict(ow=1), 'extents'), (dict(oh=8193), 'extents')):
        rc, msg = call(**kw)
        assert rc == -1 and 'ts2d_resample_cubic' in msg and word in msg, (kw, rc, msg)
    for bounds in ((np.nan, 1.0), (0.0, np.inf), (2.0, 1.0)):
        bad = np.array([bounds], np.float32)
        rc, msg = call(lh=bad.ctypes.data)
        assert rc == -1 and 'ts2d_resample_cubic' in msg and 'clip bounds' in msg, (bounds, rc, msg)
    # every refusal of the input-side entries that is reached before the device is selected, word for word (the strings were
    # recorded from the library as it was before the entries moved to their own unit and shared one extent / size check)
    for entry, args, want in _input_side_refusals():
        rc = getattr(lib, entry)(*args)
        assert (rc, _lib.last_error()) == (-1, want), (entry, args, rc, _lib.last_error())
    handle = ctypes.c_void_p(1234)                        # a refused ts2d_planes_create leaves no handle behind
    assert lib.ts2d_planes_create(0, src.ctypes.data, 0, 8, 8, ctypes.byref(handle)) == -1 and handle.value is None


_SMALL = np.zeros(64, np.float32)


def _input_side_refusals():
    """(entry, arguments, message) - the buffers are small: every call is refused before it reads one."""
    p = _SMALL.ctypes.data
    out = ctypes.pointer(ctypes.c_void_p())
    R, C, J = 'ts2d_resample_cubic', 'ts2d_planes_create', 'ts2d_project_coronal'
    ext = 'ts2d_resample_cubic: extents %d x %d -> %d x %d outside 2 ... 8192'
    big = 'ts2d_resample_cubic: %d planes of %d x %d -> %d x %d are more than one call takes (2^28 samples)'
    view = 'ts2d_project_coronal: the strided view leaves the buffer'
    return [
        (R, (0, None, 1, 8, 8, 5, 5, p, p), 'ts2d_resample_cubic: null argument'),
        (R, (0, p, 1, 8, 8, 5, 5, None, p), 'ts2d_resample_cubic: null argument'),
        (R, (0, p, 1, 8, 8, 5, 5, p, None), 'ts2d_resample_cubic: null argument'),
        (R, (0, p, 0, 8, 8, 5, 5, p, p), 'ts2d_resample_cubic: 0 planes'),
        (R, (0, p, -3, 8, 8, 5, 5, p, p), 'ts2d_resample_cubic: -3 planes'),
        (R, (0, p, 1, 1, 8, 5, 5, p, p), ext % (1, 8, 5, 5)),
        (R, (0, p, 1, 8, 1, 5, 5, p, p), ext % (8, 1, 5, 5)),
        (R, (0, p, 1, 8, 8, 1, 5, p, p), ext % (8, 8, 1, 5)),
        (R, (0, p, 1, 8, 8, 5, 1, p, p), ext % (8, 8, 5, 1)),
        (R, (0, p, 1, 8193, 8, 5, 5, p, p), ext % (8193, 8, 5, 5)),
        (R, (0, p, 1, 8, 8193, 5, 5, p, p), ext % (8, 8193, 5, 5)),
        (R, (0, p, 1, 8, 8, 8193, 5, p, p), ext % (8, 8, 8193, 5)),
        (R, (0, p, 1, 8, 8, 5, 8193, p, p), ext % (8, 8, 5, 8193)),
        (R, (0, p, 1, 0, -4, 5, 5, p, p), ext % (0, -4, 5, 5)),
        (R, (0, p, 4, 8192, 8192, 5, 5, p, p), big % (4, 8192, 8192, 5, 5)),                  # 4 x 8216 x 8216 padded samples in
        (R, (0, p, 5, 8, 8, 8192, 8192, p, p), big % (5, 8, 8, 8192, 8192)),                  # 5 x 8192 x 8192 samples out
        (C, (0, None, 1, 8, 8, out), 'ts2d_planes_create: null argument'),
        (C, (0, p, 1, 8, 8, None), 'ts2d_planes_create: null argument'),
        (C, (0, p, 0, 8, 8, out), 'ts2d_planes_create: 0 planes outside 1 ... 65535'),
        (C, (0, p, 65536, 8, 8, out), 'ts2d_planes_create: 65536 planes outside 1 ... 65535'),
        (C, (0, p, 1, 0, 8, out), 'ts2d_planes_create: extents 0 x 8 outside 1 ... 8192'),
        (C, (0, p, 1, 8, 0, out), 'ts2d_planes_create: extents 8 x 0 outside 1 ... 8192'),
        (C, (0, p, 1, 8193, 8, out), 'ts2d_planes_create: extents 8193 x 8 outside 1 ... 8192'),
        (C, (0, p, 1, 8, 8193, out), 'ts2d_planes_create: extents 8 x 8193 outside 1 ... 8192'),
        (C, (0, p, 5, 8192, 8192, out), 'ts2d_planes_create: 5 planes of 8192 x 8192 are more than one handle takes (2^28 samples)'),
        (J, (0, None, 64, 2, 4, 4, 4, 16, 4, 1, 0, p, p), 'ts2d_project_coronal: null argument'),
        (J, (0, p, 64, 2, 4, 4, 4, 16, 4, 1, 0, None, p), 'ts2d_project_coronal: null argument'),
        (J, (0, p, 64, 2, 4, 4, 4, 16, 4, 1, 0, p, None), 'ts2d_project_coronal: null argument'),
        (J, (0, p, 64, -1, 4, 4, 4, 16, 4, 1, 0, p, p), 'ts2d_project_coronal: bad dtype / extents'),
        (J, (0, p, 64, 5, 4, 4, 4, 16, 4, 1, 0, p, p), 'ts2d_project_coronal: bad dtype / extents'),
        (J, (0, p, 64, 2, 0, 4, 4, 16, 4, 1, 0, p, p), 'ts2d_project_coronal: bad dtype / extents'),
        (J, (0, p, 64, 2, 4, 4, 0, 16, 4, 1, 0, p, p), 'ts2d_project_coronal: bad dtype / extents'),
        (J, (0, p, 63, 2, 4, 4, 4, 16, 4, 1, 0, p, p), view),                                 # the last element is number 63
        (J, (0, p, 64, 2, 4, 4, 4, 16, 4, 1, 1, p, p), view),                                 # ... shifted past the end by the base
        (J, (0, p, 64, 2, 4, 4, 4, 16, 4, 1, -1, p, p), view),                                # a base in front of the buffer
        (J, (0, p, 64, 2, 4, 4, 4, 16, 4, -1, 2, p, p), view),                                # a negative stride that walks in front of it
        (J, (0, p, 0, 2, 1, 1, 1, 0, 0, 0, 0, p, p), view),                                   # an empty buffer
    ]


# ------------------------------------------------------------------------------------------------ emitted code
@pytest.fixture(scope='module')
def resample_in_asm(tmp_path_factory):
    """kernels_resample_in.h alone, compiled to gfx950 assembly with the device flags of the shipped build (csrc/Makefile DEVFLAGS)."""
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    d = tmp_path_factory.mktemp('resample_in_isa')
    csrc = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
    tu = d / 'resample_in.hip'
    tu.write_text(f'#include "{os.path.join(csrc, "kernels_resample_in.h")}"\n')
    devflags = subprocess.check_output(['make', '-s', '-C', csrc, 'flags'], text=True).split()
    subprocess.check_call([HIPCC, '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S', *devflags, '-o', str(d / 'resample_in.s'), str(tu)],
                          stderr=subprocess.DEVNULL)
    return open(d / 'resample_in.s').read()


@pytest.mark.parametrize('kernel,n_mul,n_add', [('rsin_prefilter_cols', 40, 30), ('rsin_prefilter_rows', 40, 30), ('rsin_interp_clip', 128, 64)])
def test_kernels_have_no_fused_multiply_add_no_scratch_and_no_spills(resample_in_asm, kernel, n_mul, n_add):
    m = re.search(rf'^(_ZN4ts2d\d+{kernel}\w*):', resample_in_asm, re.M)
    assert m, f'{kernel} not found in the assembly'
    body = resample_in_asm[m.end():resample_in_asm.index('.Lfunc_end', m.end())]
    ops = [ln.split()[0] for ln in body.split('\n') if ln.strip() and not ln.strip().startswith((';', '.'))]
    fused = [o for o in ops if 'f64' in o and ('fma' in o or 'mad' in o)]          # v_fma_f64, v_fmac_f64, ...
    assert not fused, f'a float64 product was fused into its sum ({fused[0]}): bit-identity with the host statement is gone'
    assert sum(o == 'v_mul_f64' for o in ops) >= n_mul and sum(o == 'v_add_f64' for o in ops) >= n_add
    assert not [o for o in ops if o.startswith('scratch_')], f'{kernel} spills registers'
    assert not [o for o in ops if o in ('v_rcp_f64_e32', 'v_div_scale_f64', 'v_floor_f64_e32')], f'{kernel} divides or floors on the device'
    meta = resample_in_asm[resample_in_asm.index('amdhsa.kernels:'):]
    blk = next(b for b in re.split(r'\n  - \.', meta)[1:] if kernel in b)
    assert re.search(r'private_segment_fixed_size:\s*0\b', blk) and re.search(r'vgpr_spill_count:\s*0\b', blk) and re.search(r'sgpr_spill_count:\s*0\b', blk)


# ------------------------------------------------------------------------------------------------ routing
class _StandIn:
    """ts2d_resample_cubic computed by the numpy statement, counting its calls."""
    def __init__(self):
        self.calls = []

    def __call__(self, device, src, n, ih, iw, oh, ow, lo_hi, dst):
        self.calls.append((device, n, ih, iw, oh, ow))
        s = np.ctypeslib.as_array(ctypes.cast(src, ctypes.POINTER(ctypes.c_float)), (n, ih, iw))
        lh = np.ctypeslib.as_array(ctypes.cast(lo_hi, ctypes.POINTER(ctypes.c_float)), (n, 2))
        d = np.ctypeslib.as_array(ctypes.cast(dst, ctypes.POINTER(ctypes.c_float)), (n, oh, ow))
        for p in range(n):
            assert lh[p, 0] == s[p].min() and lh[p, 1] == s[p].max()
            d[p] = P.resize_cubic_f64(s[p], (oh, ow))
        return 0


def _run(data, spacing, props_extra):
    pm = SimpleNamespace(transpose_forward=[0, 1, 2], plans={})
    cm = SimpleNamespace(spacing=[1.5, 1.5], normalization_schemes=['NoNormalization'] * data.shape[0], use_mask_for_norm=[False] * data.shape[0])
    props = dict({'spacing': (999.0,) + spacing}, **props_extra)
    out, _, props = P.DefaultPreprocessor(verbose=False).run_case_npy(data.copy(), None, props, pm, cm, {})
    return out, props


def test_run_case_npy_routes_an_off_spacing_case_to_the_entry_when_asked(monkeypatch):
    rng = np.random.default_rng(5)
    data = (rng.standard_normal((2, 1, 60, 45)) * 30 + 7).astype(np.float32)
    stand = _StandIn()
    monkeypatch.setattr(P, 'cubic_device_entry', lambda: stand)
    host, props = _run(data, (1.0, 0.8), {})
    assert stand.calls == [] and host.shape == (2, 1, 40, 24)
    dev, props = _run(data, (1.0, 0.8), {'device_resample': 3})
    assert stand.calls == [(3, 2, 60, 45, 40, 24)] and 'device_resample' not in props           # ONE call for all planes
    assert np.array_equal(_bits(dev), _bits(host))
    same, _ = _run(data, (1.5, 1.5), {'device_resample': 3})                                     # on the plan spacing: nothing to resample
    assert len(stand.calls) == 1 and np.array_equal(same, data)
    bad = data.copy(); bad[1, 0, 5, 5] = np.inf                                                  # a non-finite plane: scipy, as before
    with np.errstate(all='ignore'):
        a, _ = _run(bad, (1.0, 0.8), {'device_resample': 3})
        b, _ = _run(bad, (1.0, 0.8), {})
    assert len(stand.calls) == 1 and np.array_equal(a, b, equal_nan=True)
    thin = data[:, :, :, :1]                                                                      # an extent below 2: scipy
    a, _ = _run(thin, (1.0, 1.5), {'device_resample': 3})
    b, _ = _run(thin, (1.0, 1.5), {})
    assert len(stand.calls) == 1 and np.array_equal(_bits(a), _bits(b))
    monkeypatch.setattr(P, 'cubic_device_entry', lambda: None)                                    # a library without the symbol: scipy, silently
    c, _ = _run(data, (1.0, 0.8), {'device_resample': 3})
    assert np.array_equal(_bits(c), _bits(host))


def test_the_preprocess_key_tells_the_two_settings_apart():
    p = SimpleNamespace(configuration_manager=SimpleNamespace(spacing=[1.5, 1.5]), plans_manager=SimpleNamespace(), dataset_json={})
    assert HIPModel._preprocess_key(p, {}) != HIPModel._preprocess_key(p, {'device_resample': 0})
    assert HIPModel._preprocess_key(p, {'device_resample': 0}) == HIPModel._preprocess_key(p, {'device_resample': 0})


def test_a_model_without_engines_of_this_library_keeps_the_host_route():
    m = HIPModel.__new__(HIPModel)
    m.device_input_resample = True
    m._predictor = SimpleNamespace(engines=[SimpleNamespace(close=lambda: None)])
    assert m._resample_device() is None
    m._predictor = SimpleNamespace(engines=[])
    assert m._resample_device() is None
