"""The projection modes as far as they go without a GPU: ``image.project`` for median, std, first / depth, slice:* and min against spelled-out
per-ray Python loops, the refusals, and the selection of the device kernels (csrc/ray_select.h) compiled for the host against ``np.sort``."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from totalsegmentator2d_amd import image, nrrd

CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
EYE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
DTYPES = ('int16', 'uint8', 'uint16', 'int32', 'float32')
AXES = ('sagittal', 'coronal', 'axial')          # sitk axes 0, 1, 2 = numpy axes 2, 1, 0


def _img(arr):
    return nrrd.Image(np.ascontiguousarray(arr), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), EYE, 1, {}, None)


def _extremes(dtype):
    if dtype == 'float32':
        fi = np.finfo(np.float32)
        return np.array([fi.min, fi.max, -fi.tiny, fi.tiny, -1e-45, 1e-45, 0.0, -0.0, -1.5, 1.5], np.float32)
    ii = np.iinfo(dtype)
    return np.array([ii.min, ii.max, 0, 1, ii.max - 1, ii.min + 1], dtype)


def _volume(dtype, n, axis, rng):
    """A small volume whose rays along sitk ``axis`` have length n: random rays, rays of ties, all-equal rays, all-zero rays, extreme values."""
    shape = [3, 4, 6]
    shape[2 - axis] = n
    if dtype == 'float32':
        a = rng.normal(0, 50, shape).astype(np.float32)
    else:
        ii = np.iinfo(dtype)
        a = rng.integers(max(ii.min, -2000), min(ii.max, 3000) + 1, shape).astype(dtype)
    moved = np.moveaxis(a, 2 - axis, -1)
    rays = moved.reshape(-1, n).copy()
    ex = _extremes(dtype)
    rays[0] = 0                                                 # all zero
    rays[1] = ex[1]                                             # all equal
    rays[2] = rng.choice(ex[:2], n)                             # ties of the extremes
    rays[3] = rng.choice(np.array([0, 1, 1, 3], a.dtype), n)   # ties around zero
    rays[4, : n - 1] = 0                                        # first non-zero sample is the last one
    rays[5] = rng.choice(ex, n)
    rays[6, 0] = 0                                              # a leading zero before the first sample
    return np.ascontiguousarray(np.moveaxis(rays.reshape(moved.shape), -1, 2 - axis))


def _rays(a, axis):
    """(rays [m, n] as Python lists in index order, the shape of the result with the projected axis kept)"""
    npax = 2 - axis
    moved = np.moveaxis(a, npax, -1)
    shape = list(a.shape)
    shape[npax] = 1
    return moved.reshape(-1, a.shape[npax]), moved.shape[:-1], shape, npax


def _expect(a, axis, fn, dtype):
    rays, lead, shape, npax = _rays(a, axis)
    flat = np.array([fn(r) for r in rays], dtype)
    return np.expand_dims(flat.reshape(lead), npax)


def _std_loop(ray):
    n = len(ray)
    if isinstance(ray[0], (int, np.integer)):
        mean = float(sum(int(v) for v in ray)) / float(n)         # exact integer sum, one division
    else:
        s = 0.0
        for v in ray:
            s += float(v)
        mean = s / float(n)
    sq = 0.0
    for v in ray:
        d = float(v) - mean
        sq += d * d
    return math.sqrt(sq / float(n - 1))


def _first_loop(ray):
    for v in ray:
        if v != 0:
            return v
    return ray[0]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [2, 3, 4, 5])
def test_project_modes_against_per_ray_loops(dtype, n):
    rng = np.random.default_rng(100 + n)
    for axis, axname in enumerate(AXES):
        a = _volume(dtype, n, axis, rng)
        img = _img(a)
        nat = a.dtype

        def got(mode):
            r = image.project(img, mode, axname)
            assert list(r.array.shape) == _rays(a, axis)[2]
            return r.array

        med = got('median')
        assert med.dtype == nat and np.array_equal(med, _expect(a, axis, lambda r: sorted(r.tolist())[n // 2], nat)), (axname, 'median')
        std = got('std')
        assert std.dtype == np.float64
        want = _expect(a, axis, lambda r: _std_loop(r.tolist()), np.float64)
        assert np.array_equal(std, want), (axname, 'std')
        for name in ('first', 'depth', ' First '):
            f = got(name)
            assert f.dtype == nat and np.array_equal(f, _expect(a, axis, lambda r: _first_loop(r.tolist()), nat)), (axname, name)
        mn = got('min')
        assert mn.dtype == nat and np.array_equal(mn, _expect(a, axis, lambda r: min(r.tolist()), nat)), (axname, 'min')
        for pos, idx in (('first', 0), ('middle', int(np.round(n * 0.5))), ('0.25', int(np.round(n * 0.25)))):
            s = got(f'slice:{pos}')
            assert s.dtype == nat and np.array_equal(s, np.take(a, [idx], axis=2 - axis)), (axname, pos)
        with pytest.raises(RuntimeError, match=rf'range \[0, {n}\)'):
            got('slice:last')


def test_float_std_of_a_float_volume_uses_the_index_order_mean():
    """float32 rays whose float64 sum depends on the order: the statement adds in index order (ITK's accumulator), not pairwise."""
    rng = np.random.default_rng(7)
    a = (rng.normal(0, 1, (2, 301, 3)) * np.float32(10.0) ** rng.integers(-6, 7, (2, 301, 3))).astype(np.float32)
    got = image.project(_img(a), 'std', 'coronal').array
    want = _expect(a, 1, lambda r: _std_loop(r.tolist()), np.float64)
    assert np.array_equal(got, want)


def test_slice_positions_round_half_to_even():
    for n, idx in ((5, 2), (7, 4)):                              # 2.5 -> 2, 3.5 -> 4
        a = np.arange(2 * n * 3, dtype=np.int16).reshape(2, n, 3)
        s = image.project(_img(a), 'slice:0.5', 'coronal').array
        assert np.array_equal(s, a[:, idx:idx + 1, :]), n
        assert image.slice_projection_index('0.5', n) == idx
    assert image.slice_projection_index('middle', 4) == 2 and image.slice_projection_index('first', 4) == 0
    assert image.slice_projection_index('-3', 4) == 0            # clipped below
    for bad in ('last', '1', '7.5'):
        with pytest.raises(RuntimeError, match=r'range \[0, 4\)'):
            image.slice_projection_index(bad, 4)
    for bad in ('abc', '', None, 'nan'):
        with pytest.raises(RuntimeError, match='slice position'):
            image.slice_projection_index(bad, 4)
    with pytest.raises(RuntimeError, match='slice position'):
        image.project(_img(np.zeros((2, 3, 4), np.int16)), 'slice:abc', 'coronal')


def test_modes_that_stay_unsupported():
    img = _img(np.zeros((2, 3, 4), np.int16))
    for mode in ('multiclass:3', 'foo', 'xr', 'median:2', 'multiclass'):
        with pytest.raises(RuntimeError, match='Unsupported filter mode'):
            image.project(img, mode, 'coronal')
        assert image.device_projection_mode(mode, 3) is None
    assert image.parse_projection_mode(' Slice:Middle ') == ('slice', 'middle') and image.parse_projection_mode('MIP') == ('mip', None)
    from totalsegmentator2d_amd import _lib
    codes = {m: image.device_projection_mode(m, 8) for m in ('max', 'mip', 'min', 'mean', 'avg', 'median', 'std', 'first', 'depth', 'slice:middle')}
    assert codes == {'max': (0, 0), 'mip': (0, 0), 'min': (1, 0), 'mean': (2, 0), 'avg': (2, 0), 'median': (3, 0), 'std': (4, 0), 'first': (5, 0),
                     'depth': (5, 0), 'slice:middle': (6, 4)}
    assert set(_lib.PROJECT_MODES.values()) == set(range(7))
    assert image.device_projection_mode('slice:last', 8) is None and image.device_projection_mode('std', 1) is None


# ------------------------------------------------------------------------------------------------ the selection of the kernels on the host
KEY_TYPES = {'int16': ('int16_t', np.uint16), 'uint8': ('uint8_t', np.uint8), 'uint16': ('uint16_t', np.uint16), 'int32': ('int32_t', np.uint32),
             'float32': ('float', np.uint32)}


@pytest.fixture(scope='module')
def host_select(tmp_path_factory):
    """csrc/ray_select.h compiled as plain C++: per sample type the keys, their inverse, the k-th smallest over staged keys (the LDS kernel's
    arithmetic) and over samples (the variant that re-reads the ray)."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    d = tmp_path_factory.mktemp('ray_select')
    body = [f'#include "{os.path.join(CSRC, "ray_select.h")}"', 'using namespace ts2d;']
    for name, (ct, _) in KEY_TYPES.items():
        body.append(f'''
extern "C" void keys_{name}(const {ct}* v, int n, RsKey<{ct}>::type* k, {ct}* back) {{
    for (int i = 0; i < n; ++i) {{ k[i] = rs_key(v[i]); back[i] = rs_unkey<{ct}>(k[i]); }}
}}
extern "C" void kth_{name}(const {ct}* ray, int n, long long stride, int k, {ct}* from_keys, {ct}* from_samples) {{
    RsKey<{ct}>::type* keys = new RsKey<{ct}>::type[n];
    for (int i = 0; i < n; ++i) keys[i] = rs_key(ray[i * stride]);
    *from_keys = rs_unkey<{ct}>(rs_select_kth<RsKey<{ct}>::type, RsKey<{ct}>::bits>(keys, n, 1, k));
    *from_samples = rs_select_kth_samples<{ct}>(ray, n, stride, k);
    delete[] keys;
}}''')
    src = d / 'rs.cpp'
    src.write_text('\n'.join(body) + '\n')
    so = d / 'rs.so'
    subprocess.check_call([cxx, '-x', 'c++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', str(so), str(src)])
    return ctypes.CDLL(str(so))


def _bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _kth(lib, name, ray, k, stride=1):
    ray = np.ascontiguousarray(ray)
    a, b = np.zeros(1, ray.dtype), np.zeros(1, ray.dtype)
    fn = getattr(lib, f'kth_{name}')
    fn.restype, fn.argtypes = None, [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    fn(ray.ctypes.data, (len(ray) + stride - 1) // stride, stride, k, a.ctypes.data, b.ctypes.data)
    return a[0], b[0]


def _keys(lib, name, v):
    v = np.ascontiguousarray(v)
    k = np.zeros(len(v), KEY_TYPES[name][1]); back = np.zeros_like(v)
    fn = getattr(lib, f'keys_{name}')
    fn.restype, fn.argtypes = None, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    fn(v.ctypes.data, len(v), k.ctypes.data, back.ctypes.data)
    return k, back


def test_key_round_trip_and_order(host_select):
    for name in ('int16', 'uint16'):                              # all 65 536 values
        v = np.arange(65536, dtype=np.uint16).view(name)
        k, back = _keys(host_select, name, v)
        assert np.array_equal(back, v)
        order = np.argsort(v, kind='stable')
        assert np.array_equal(k[order], np.arange(65536, dtype=np.uint16))      # a bijection that keeps the order
    v = np.arange(256, dtype=np.uint8)
    k, back = _keys(host_select, 'uint8', v)
    assert np.array_equal(k, v) and np.array_equal(back, v)
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 4096), [-2 ** 31, 2 ** 31 - 1, 0, -1, 1]]).astype(np.int32)
    k, back = _keys(host_select, 'int32', v)
    assert np.array_equal(back, v) and np.array_equal(np.argsort(k, kind='stable'), np.argsort(v, kind='stable'))
    fi = np.finfo(np.float32)
    f = np.concatenate([rng.integers(0, 2 ** 32, 8192).astype(np.uint32).view(np.float32),
                        np.array([fi.min, fi.max, -fi.tiny, fi.tiny, -1e-45, 1e-45, 1e-40, -1e-40, 0.0, -0.0, np.inf, -np.inf], np.float32)])
    f = f[~np.isnan(f)]
    k, back = _keys(host_select, 'float32', f)
    assert np.array_equal(_bits(back), _bits(f))                  # bit for bit, the sign of a zero included
    o = np.argsort(k, kind='stable')
    assert np.all(np.diff(f[o].astype(np.float64)) >= 0)          # ascending keys = ascending values
    kz, _ = _keys(host_select, 'float32', np.array([-0.0, 0.0], np.float32))
    assert kz[0] + 1 == kz[1]                                      # -0.0 right below +0.0


@pytest.mark.parametrize('name', list(KEY_TYPES))
def test_selection_against_sort(host_select, name):
    rng = np.random.default_rng(11)
    ex = _extremes(name)
    if name == 'float32':
        ex = np.concatenate([ex, np.array([1e-40, -1e-40, -3e38, 3e38], np.float32)])      # subnormals, large negatives
    for n in (1, 2, 3, 64, 65, 257):
        if name == 'float32':
            rays = [rng.normal(0, 100, n).astype(np.float32), -np.abs(rng.normal(0, 1e-3, n)).astype(np.float32),
                    rng.integers(0, 2 ** 23, n).astype(np.uint32).view(np.float32) * rng.choice(np.array([-1, 1], np.float32), n)]
        else:
            ii = np.iinfo(name)
            rays = [rng.integers(ii.min, ii.max + 1, n).astype(name), rng.integers(0, 4, n).astype(name)]
        rays += [rng.choice(ex, n), np.full(n, ex[0]), np.full(n, ex[1]), np.zeros(n, ex.dtype)]
        for ray in rays:
            ray = np.asarray(ray, dtype=name)
            want = np.sort(ray)
            for k in sorted({n // 2, 0, n - 1}):
                a, b = _kth(host_select, name, ray, k)
                assert a == want[k] and b == want[k], (n, k)
    # a strided ray: every third sample
    ray = np.asarray(rng.choice(ex, 3 * 65), dtype=name)
    a, b = _kth(host_select, name, ray, 65 // 2, stride=3)
    assert a == np.sort(ray[::3])[65 // 2] == b
