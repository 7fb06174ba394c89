"""PNG visuals without a GPU: the statement of totalsegmentator2d_amd/visual.py (create_visual of the reference, ts2d/core/util/image.py:383-453),
the PNG writer, the host tables of csrc/visual_plan.cpp against the statement, the C-ABI declarations, and the surface (Result.save, ts2d_run)."""
import ctypes
import os
import random
import re
import shutil
import struct
import subprocess
import warnings
import zlib

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, image, nrrd, png
from totalsegmentator2d_amd import visual as V
from totalsegmentator2d_amd.main import ts2d_entry_point, ts2d_run
from totalsegmentator2d_amd.tool import TS2D

A = os.path.join(GOLDEN, 'assets')
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
EYE2 = (1.0, 0.0, 0.0, 1.0)


def _img(arr, spacing_hw=(1.0, 1.0), components=1, meta=None):
    return nrrd.Image(arr, (spacing_hw[1], spacing_hw[0]), (0.0, 0.0), EYE2, components, dict(meta or {}), None)


# ------------------------------------------------------------------------------------------------ statement: flatten, palette
def test_flatten_takes_the_last_nonzero_plane():
    planes = np.zeros((5, 3, 4), np.uint8)
    planes[0, 0, 0] = 1
    planes[1, 0, 1] = 7; planes[3, 0, 1] = 1                 # the later plane wins
    planes[4, 1, :] = 255; planes[2, 1, :] = 1
    got = V.flatten_index(planes)
    want = np.zeros((3, 4), np.uint8); want[0, 0] = 1; want[0, 1] = 4; want[1, :] = 5
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(V.flatten_index(np.ones((255, 2, 2), np.uint8)), np.full((2, 2), 255, np.uint8))
    with pytest.raises(ValueError, match='256 components'):
        V.flatten_index(np.zeros((256, 2, 2), np.uint8))
    with pytest.raises(ValueError, match='256 components'):
        image.create_visual(_img(np.zeros((2, 2, 256), np.uint8), components=256), labels=True)


def test_palette_and_default_colours():
    assert [V.default_color(i) for i in range(6)] == [(255, 0, 0), (0, 128, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    for i in (6, 7):
        r = random.Random(i)
        assert V.default_color(i) == (r.randint(32, 200), r.randint(32, 200), r.randint(32, 200))
    pal = V.to_palette({2: (0.5, 1.5, -1.0), 4: (1, 2, 300)})
    assert pal == [(255, 255, 255), V.default_color(1), (127, 255, 0), V.default_color(3), (1, 2, 255)]
    assert V.to_palette({}) == [(255, 255, 255)] and V.to_palette(['#9370DB', 'green']) == [(147, 112, 219), (0, 128, 0)]
    # modulo, background black
    idx = np.array([[0, 1, 2, 3, 4, 5, 200]], np.uint8)
    rgb = V.label_rgb(idx, [(9, 9, 9), (1, 0, 0), (0, 2, 0)])
    assert rgb.shape == (1, 7, 3) and rgb.dtype == np.uint8
    assert rgb[0].tolist() == [[0, 0, 0], [1, 0, 0], [0, 2, 0], [9, 9, 9], [1, 0, 0], [0, 2, 0], [0, 2, 0]]      # 200 % 3 = 2; 3 % 3 = 0: entry 0, not black
    src = open(V.__file__).read()
    assert not re.search(r'^\s*(import|from)\s+(matplotlib|seaborn)', src, flags=re.M)


# ------------------------------------------------------------------------------------------------ statement: geometry
def _scan_outside(ratio_s, ratio_m):
    first, last = [], []
    for N in range(5, 41):
        t = V.axis_table(N, ratio_s, ratio_m)
        if not t['inside'][0]:
            first.append(N)
        if not t['inside'][-1]:
            last.append(N)
    return first, last


def test_geometry_extent_centre_and_outside_rows():
    t = V.axis_table(37, 2.5, 0.8)
    assert t['M'] == int(0.5 + 37 * 2.5 / 0.8) == 116
    j = np.arange(116)
    assert np.array_equal(t['x'], np.float64(18) + (j - 58).astype(np.float64) * (np.float64(0.8) / np.float64(2.5)))
    assert np.array_equal(t['inside'], (t['x'] >= -0.5) & (t['x'] < 36.5))
    found_first, found_last = False, False
    for s, m in ((2.5, 0.8), (3.0, 1.0)):
        first, last = _scan_outside(s, m)
        found_first |= bool(first); found_last |= bool(last)
        for N in first + last:
            t = V.axis_table(N, s, m)
            out = ~t['inside']
            assert np.array_equal(t['nearest'][out], np.full(out.sum(), -1)) and not t['w'][out].any() and not t['idx'][out].any()
            ins = t['inside']
            k = np.flatnonzero(ins)
            assert 1 <= out.sum() <= 3 and ins[k[0]:k[-1] + 1].all()       # outside only at the ends: the step m/s is below 1
            assert t['nearest'][ins].min() >= 0 and t['nearest'][ins].max() <= N - 1 and t['idx'].min() >= 0 and t['idx'].max() <= N - 1
    assert found_first and found_last, 'the scan must produce an outside first row and an outside last row'
    # an outside row is black in the label visual and 0 before the window in the grey one
    s, m = next((s, m) for s, m in ((2.5, 0.8), (3.0, 1.0)) if _scan_outside(s, m)[0])
    N = _scan_outside(s, m)[0][0]
    lab = np.full((N, 4), 1, np.uint8)
    vis = image.create_visual(_img(lab, (s, m)), labels=True, palette=[(0, 0, 0), (10, 20, 30)])
    assert vis.array.shape == (V.uniform_extent(N, s, m), 4, 3) and vis.components == 3 and vis.spacing == (m, m)
    ins = V.axis_table(N, s, m)['inside']
    assert not ins[0] and not vis.array[~ins].any() and (vis.array[ins] == (10, 20, 30)).all()
    grey = image.create_visual(_img(np.full((N, 4), 7, np.int16), (s, m)), labels=False)
    assert grey.array.dtype == np.uint8 and not grey.array[~ins].any() and (grey.array[ins] > 200).all()      # the outside zeros widen the window to 0 ... 7 (a truncated 6.99 is 6: 218)


def test_nearest_rounds_half_up():
    t = V.axis_table(8, 2.0, 1.0)                           # ratio 0.5: every odd output index is a tie
    assert t['M'] == 16 and np.array_equal(t['x'], 4.0 + (np.arange(16) - 8) * 0.5)
    ins = t['inside']
    assert ins[:-1].all() and not ins[-1] and t['x'][-1] == 7.5      # 7.5 is not below N - 0.5
    assert np.array_equal(t['nearest'][ins], np.floor(t['x'] + 0.5).astype(np.int64)[ins]) and t['nearest'][-1] == -1
    assert t['nearest'][1] == 1 and t['x'][1] == 0.5 and t['nearest'][3] == 2 and t['x'][3] == 1.5      # .5 goes up, never to even
    plane = np.arange(8, dtype=np.uint8)[:, None] * np.ones((1, 2), np.uint8) + 1
    vis = image.create_visual(_img(plane, (2.0, 1.0)), labels=True, palette=[(0, 0, 0)] + [(k, 0, 0) for k in range(1, 9)])
    assert vis.array[:, 0, 0].tolist() == (t['nearest'] + 1).tolist()      # (the outside row: -1 + 1 = 0, black)


def test_isotropic_plane_passes_through():
    rng = np.random.default_rng(1)
    p = rng.integers(-500, 1500, (9, 11)).astype(np.int16)
    vis = image.create_visual(_img(p, (1.5, 1.5 + 1e-9)), labels=False)
    assert vis.array.shape == p.shape and vis.spacing == (1.5 + 1e-9, 1.5)
    assert np.array_equal(vis.array, V.window_u8(p, float(p.min()), float(p.max())))
    lab = rng.integers(0, 4, (9, 11)).astype(np.uint8)
    got = image.create_visual(_img(lab, (0.7, 0.7)), labels=True, palette={1: (255, 0, 0), 3: (0, 0, 255)})
    assert np.array_equal(got.array, V.label_rgb(lab, [(255, 255, 255), (255, 0, 0), V.default_color(2), (0, 0, 255)]))


# ------------------------------------------------------------------------------------------------ statement: cubic B-spline
def test_explicit_bspline_against_scipy():
    """The explicit prefilter and 16-tap sum against ``map_coordinates(spline_filter(mode='mirror'), order=3, mode='mirror', prefilter=False)`` in
    float64.  The two differ by the order of a 16-term sum (and the last bits of the coefficients), bound 64 * 2^-53 * max|coefficient|.
    Measured maximum over the cases below: 1.16 * 2^-53 * max|coefficient| (4.5e-13 absolute on samples of N(0, 300^2))."""
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(7)
    worst = 0.0
    for (H, W), (sh, sw) in (((37, 53), (0.8, 2.5)), ((16, 16), (3.0, 1.0)), ((5, 33), (1.0, 2.0)), ((17, 2), (2.5, 0.8)), ((600, 8), (1.0, 3.0))):
        p = (rng.normal(size=(H, W)) * 300).astype(np.float32)
        m = min(sh, sw)
        ty, tx = V.axis_table(H, sh, m), V.axis_table(W, sw, m)
        c = V.spline_coefficients(p)
        cs = ndi.spline_filter(p.astype(np.float64), order=3, output=np.float64, mode='mirror')
        bound = 64 * 2.0 ** -53 * np.abs(cs).max()
        assert np.abs(c - cs).max() <= bound
        r = np.zeros((ty['M'], tx['M']))
        for a in range(4):
            for b in range(4):
                r = r + (c[ty['idx'][:, a]][:, tx['idx'][:, b]] * ty['w'][:, a, None]) * tx['w'][None, :, b]
        yy, xx = np.meshgrid(ty['x'], tx['x'], indexing='ij')
        ref = ndi.map_coordinates(cs, [yy, xx], order=3, mode='mirror', prefilter=False)
        ins = ty['inside'][:, None] & tx['inside'][None, :]
        err = np.abs(r - ref)[ins].max()
        worst = max(worst, err / (2.0 ** -53 * np.abs(cs).max()))
        print(f'{H} x {W}: max|explicit - scipy| = {err:.3e}, bound {bound:.3e}')
        assert err <= bound
        got = V.resample_cubic(p, ty, tx)
        assert got.dtype == np.float32 and np.array_equal(got[ins], r.astype(np.float32)[ins]) and not got[~ins].any()
    print(f'worst = {worst:.2f} * 2^-53 * max|coefficient|')


def test_integer_results_are_clamped_then_truncated():
    r = np.array([-40000.7, -1.9, -0.5, 0.99, 1.5, 32767.2, 70000.0])
    assert V.cast_to_pixel_type(r, np.int16).tolist() == [-32768, -1, 0, 0, 1, 32767, 32767]
    assert V.cast_to_pixel_type(r, np.uint16).tolist() == [0, 0, 0, 0, 1, 32767, 65535]
    assert V.cast_to_pixel_type(np.array([0.1]), np.float32)[0] == np.float32(0.1)
    # a step edge overshoots: the int16 resample clamps where the float one does not
    p = np.zeros((8, 8), np.int16); p[:, 4:] = 32767
    ty, tx = V.axis_table(8, 1.0, 0.5), V.axis_table(8, 1.0, 0.5)
    got = V.resample_cubic(p, ty, tx)
    assert got.dtype == np.int16 and got.max() == 32767 and got.min() < 0
    assert V.resample_cubic(p.astype(np.float32), ty, tx).max() > 32767


# ------------------------------------------------------------------------------------------------ statement: window
def test_window_cases():
    p = np.array([[-10, 0, 10, 20, 30]], np.int16)
    assert V.window_u8(p, -10.0, 30.0).tolist() == [[0, 63, 127, 191, 255]]                     # auto: truncation, not rounding
    assert np.array_equal(image.create_visual(_img(p), labels=False).array, V.window_u8(p, -10.0, 30.0))
    assert image.create_visual(_img(p), labels=False, window=(0, 20)).array.tolist() == [[0, 0, 127, 255, 255]]
    assert image.create_visual(_img(p), labels=False, window=(None, 10)).array.tolist() == [[0, 127, 255, 255, 255]]
    assert image.create_visual(_img(p), labels=False, window='minmax').array.tolist() == [[0, 63, 127, 191, 255]]
    assert not image.create_visual(_img(np.full((3, 3), 5, np.int16)), labels=False).array.any()      # hi == lo: all zero
    assert not V.window_u8(p, 4.0, 4.0).any()
    lo, hi = np.percentile(p, (5, 95))
    assert np.array_equal(image.create_visual(_img(p), labels=False, window='pc5').array, V.window_u8(p, lo, hi)) and (lo, hi) == (-8.0, 28.0)
    assert np.array_equal(image.create_visual(_img(p), labels=False, window='pc10-50').array, V.window_u8(p, *np.percentile(p, (10, 50))))
    with pytest.raises(RuntimeError, match='windowing method'):
        image.create_visual(_img(p), labels=False, window='otsu')
    f = np.array([[0.0, 0.1, 0.2, 0.3]], np.float32)
    x = f.astype(np.float64)
    scale = 255.0 / (float(f.max()) - 0.0)
    assert np.array_equal(V.window_u8(f, 0.0, float(f.max()))[0], np.trunc((x * scale + -0.0 * scale).astype(np.float32).astype(np.float64))[0].astype(np.uint8))
    with pytest.raises(ValueError, match='multi-component'):
        image.create_visual(_img(np.zeros((4, 4, 2), np.float32), components=2), labels=False)


def test_labels_default_follows_the_metadata_and_a_uint8_grey_takes_nearest():
    seg = _img((np.arange(12).reshape(3, 4) % 3).astype(np.uint8), (1.0, 2.0))
    image.set_annotation_meta(seg, {1: 'a', 2: 'b'}, {'a': (255, 0, 0), 'b': '#00FF00'})
    vis = image.create_visual(seg)                           # labels=None: Segment* keys -> labels, palette from the metadata
    assert vis.components == 3 and vis.array.shape == (3, 8, 3)
    assert set(map(tuple, vis.array.reshape(-1, 3).tolist())) == {(0, 0, 0), (255, 0, 0), (0, 255, 0)}
    plain = _img(seg.array, (1.0, 2.0))
    with pytest.warns(UserWarning, match='nearest neighbour'):
        grey = image.create_visual(plain)                    # no metadata, no palette: grey; uint8 -> nearest
    tx = V.axis_table(4, 2.0, 1.0)
    want = seg.array[:, np.clip(tx['nearest'], 0, None)] * tx['inside'].astype(np.uint8)[None, :]
    assert grey.components == 1 and np.array_equal(grey.array, V.window_u8(want, 0.0, 2.0))
    vol = nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))    # 3-D: reoriented, projected along the coronal axis, collapsed
    v = image.create_visual(vol, labels=False, axis='coronal')
    mx = image.reduce_dimensions(image.project(image.reorient_image(vol), 'max', 'coronal'))
    assert v.array.shape == (133, 53) and np.array_equal(v.array, V.window_u8(mx.array, float(mx.array.min()), float(mx.array.max())))


# ------------------------------------------------------------------------------------------------ PNG
def _walk_chunks(data):
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data)
    return chunks


@pytest.mark.parametrize('shape', [(1, 1), (3, 5, 3), (257, 2)])
def test_png_writer(tmp_path, shape):
    rng = np.random.default_rng(len(shape))
    a = rng.integers(0, 256, shape).astype(np.uint8)
    path = str(tmp_path / 'a.png')
    png.write(_img(a, components=3 if len(shape) == 3 else 1), path)
    data = open(path, 'rb').read()
    chunks = _walk_chunks(data)
    assert [k for k, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    w, h, depth, ctype, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (w, h, depth, ctype, comp, filt, lace) == (shape[1], shape[0], 8, 2 if len(shape) == 3 else 0, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(shape[0], -1)
    assert not raw[:, 0].any() and np.array_equal(raw[:, 1:].reshape(shape), a)          # filter type 0 on every scanline
    with pytest.raises(ValueError):
        png.encode(a.astype(np.int16))
    PIL = pytest.importorskip('PIL.Image')
    with PIL.open(path) as im:
        assert im.mode == ('RGB' if len(shape) == 3 else 'L') and np.array_equal(np.asarray(im), a)


# ------------------------------------------------------------------------------------------------ host tables of csrc/visual_plan.cpp
@pytest.fixture(scope='module')
def host_plan(tmp_path_factory):
    """csrc/visual_plan.cpp compiled as plain C++ behind a C shim."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    d = tmp_path_factory.mktemp('visual_plan')
    shim = d / 'shim.cpp'
    shim.write_text(f'''#include "{os.path.join(CSRC, "visual_plan.h")}"
using namespace ts2d;
extern "C" {{
int vp_extent(int N, double s, double m) {{ return visual_axis_extent(N, s, m); }}
void vp_table(int N, double s, double m, int M, VisTap* t) {{ visual_axis_table(N, s, m, M, t); }}
void vp_constants(int n, double* out) {{ const VisAxis a = visual_axis_constants(n); out[0] = a.z; out[1] = a.gain; out[2] = a.zn1; out[3] = a.k0; out[4] = a.k1; }}
void vp_zpow(int n, double* z) {{ visual_zpow(n, z); }}
void vp_window(double lo, double hi, double* out) {{ const VisWindow w = visual_window(lo, hi); out[0] = w.scale; out[1] = w.shift; }}
void vp_lut(const uint8_t* pal, int n, uint32_t* lut) {{ visual_color_lut(pal, n, lut); }}
}}
''')
    so = d / 'vp.so'
    subprocess.check_call([cxx, '-x', 'c++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', str(so), str(shim), os.path.join(CSRC, 'visual_plan.cpp')])
    lib = ctypes.CDLL(str(so))
    lib.vp_extent.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double]
    lib.vp_table.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]
    lib.vp_constants.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.vp_zpow.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.vp_window.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    lib.vp_lut.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return lib


TAP = np.dtype([('w', np.float64, 4), ('idx', np.int32, 4), ('nearest', np.int32), ('inside', np.int32)])


def test_host_tables_equal_the_statement(host_plan):
    assert TAP.itemsize == 56
    for N in list(range(1, 41)) + [337, 600, 644, 8192]:
        for s, m in ((2.5, 0.8), (3.0, 1.0), (1.0, 1.0), (2.0, 1.0), (1.0, 0.3), (0.7, 0.7)):
            t = V.axis_table(N, s, m)
            assert host_plan.vp_extent(N, s, m) == t['M'], (N, s, m)
            tab = np.zeros(t['M'], TAP)
            host_plan.vp_table(N, s, m, t['M'], tab.ctypes.data)
            assert np.array_equal(tab['inside'] != 0, t['inside']) and np.array_equal(tab['nearest'], t['nearest']), (N, s, m)
            assert np.array_equal(tab['idx'], t['idx']) and np.array_equal(tab['w'].view(np.uint64), t['w'].view(np.uint64)), (N, s, m)
    assert host_plan.vp_extent(8192, 1000.0, 0.001) == -1 and host_plan.vp_extent(1, 1.0, 3.0) == -1      # too many samples; none
    for n in (2, 5, 16, 17, 33, 600, 8192):
        c = np.zeros(5)
        host_plan.vp_constants(n, c.ctypes.data)
        import math
        zn1 = math.pow(V.POLE, float(n - 1))
        assert c.tolist() == [V.POLE, V.GAIN, zn1, 1.0 / (1.0 - zn1 * zn1), V.POLE / (V.POLE * V.POLE - 1.0)]
    z = np.zeros(600)
    host_plan.vp_zpow(600, z.ctypes.data)
    want, zi = [1.0], V.POLE
    for _ in range(599):
        want.append(zi); zi = zi * V.POLE
    assert z.tolist() == want and ((np.abs(z) > 0) & (np.abs(z) < 2.2250738585072014e-308)).any() and z[-1] == 0      # through denormals to 0
    w = np.zeros(2)
    host_plan.vp_window(-12.5, 300.25, w.ctypes.data)
    assert w.tolist() == [255.0 / (300.25 - -12.5), 12.5 * (255.0 / (300.25 - -12.5))]
    pal = np.array([(255, 255, 255), (1, 2, 3), (4, 5, 6)], np.uint8)
    lut = np.zeros(256, np.uint32)
    host_plan.vp_lut(pal.ctypes.data, 3, lut.ctypes.data)
    want = V.color_lut(pal).astype(np.uint32)
    assert np.array_equal(lut, want[:, 0] | (want[:, 1] << 8) | (want[:, 2] << 16)) and lut[0] == 0 and lut[3] == 0xFFFFFF


# ------------------------------------------------------------------------------------------------ C-ABI
def test_entries_are_declared_bound_and_optional():
    hdr = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER_PATH).read(), flags=re.S)
    want = {'ts2d_visual_labels': ['int device', 'const uint8_t* planes', 'int K', 'int H', 'int W', 'double spacing_h', 'double spacing_w',
                                   'const uint8_t* palette', 'int n_palette', 'int out_h', 'int out_w', 'uint8_t* rgb'],
            'ts2d_visual_grey': ['int device', 'const void* plane', 'int dtype', 'int H', 'int W', 'double spacing_h', 'double spacing_w', 'int cubic',
                                 'double lo', 'double hi', 'int auto_lo', 'int auto_hi', 'int out_h', 'int out_w', 'uint8_t* grey',
                                 'double* window_used', 'int* status']}
    c = ctypes
    kinds = {'int': c.c_int, 'double': c.c_double}
    lib = _lib.load()
    for name, params in want.items():
        m = re.search(rf'int\s+{name}\s*\(([^)]*)\)\s*;', hdr)
        assert m, f'{name} is not declared in include/ts2d_engine.h'
        assert [' '.join(p.split()) for p in m.group(1).split(',')] == params
        assert name in _lib.SYMBOLS and name in _lib.OPTIONAL and hasattr(lib, name)
        argtypes = [kinds.get(p.rsplit(' ', 1)[0], c.c_void_p) for p in params]
        argtypes[-1] = c.POINTER(c.c_int) if name == 'ts2d_visual_grey' else argtypes[-1]
        assert getattr(lib, name).restype is c.c_int and getattr(lib, name).argtypes == argtypes, name
    assert '#define TS2D_VISUAL_NONFINITE 1' in hdr and _lib.VISUAL_NONFINITE == V.VISUAL_NONFINITE == 1 and _lib.ABI_VERSION == 9
    assert V.DEVICE_DTYPES == image._GPU_DTYPES


def test_bad_arguments_are_refused_by_name_before_any_device_work():
    """No GPU is needed: every check below runs before the first HIP call."""
    lib = _lib.load()
    planes = np.ones((2, 4, 4), np.uint8); pal = np.zeros((2, 3), np.uint8); rgb = np.zeros((4, 4, 3), np.uint8)
    grey = np.zeros((4, 4), np.uint8); used = np.zeros(2); st = ctypes.c_int(7)
    P = lambda a: a.ctypes.data                               # noqa: E731

    def refused(rc, *words):
        msg = _lib.last_error()
        return rc == -1 and all(w in msg for w in words)
    L = lib.ts2d_visual_labels
    assert refused(L(0, None, 2, 4, 4, 1.0, 1.0, P(pal), 2, 4, 4, P(rgb)), 'ts2d_visual_labels', 'null')
    assert refused(L(0, P(planes), 2, 4, 4, 1.0, 1.0, None, 2, 4, 4, P(rgb)), 'ts2d_visual_labels', 'null')
    assert refused(L(0, P(planes), 2, 4, 4, 1.0, 1.0, P(pal), 2, 4, 4, None), 'ts2d_visual_labels', 'null')
    assert refused(L(0, P(planes), 0, 4, 4, 1.0, 1.0, P(pal), 2, 4, 4, P(rgb)), 'K = 0')
    assert refused(L(0, P(planes), 256, 4, 4, 1.0, 1.0, P(pal), 2, 4, 4, P(rgb)), 'K = 256')
    assert refused(L(0, P(planes), 2, 4, 4, 1.0, 1.0, P(pal), 0, 4, 4, P(rgb)), 'n_palette = 0')
    assert refused(L(0, P(planes), 2, 0, 4, 1.0, 1.0, P(pal), 2, 4, 4, P(rgb)), 'extents 0 x 4')
    assert refused(L(0, P(planes), 2, 4, 9000, 1.0, 1.0, P(pal), 2, 4, 4, P(rgb)), 'extents 4 x 9000')
    assert refused(L(0, P(planes), 2, 4, 4, 0.0, 1.0, P(pal), 2, 4, 4, P(rgb)), 'spacing')
    assert refused(L(0, P(planes), 2, 4, 4, float('nan'), 1.0, P(pal), 2, 4, 4, P(rgb)), 'spacing')
    assert refused(L(0, P(planes), 2, 4, 4, 2.0, 1.0, P(pal), 2, 4, 4, P(rgb)), 'out_h x out_w = 4 x 4', '8 x 4')
    assert refused(L(0, P(planes), 2, 4, 4, 1e6, 1.0, P(pal), 2, 4, 4, P(rgb)), 'resamples to more')
    G = lib.ts2d_visual_grey
    src = np.ones((4, 4), np.float32)
    ok_tail = (4, 4, P(grey), P(used), ctypes.byref(st))
    assert refused(G(0, None, 2, 4, 4, 1.0, 1.0, 0, 0.0, 1.0, 0, 0, *ok_tail), 'ts2d_visual_grey', 'null')
    assert refused(G(0, P(src), 2, 4, 4, 1.0, 1.0, 0, 0.0, 1.0, 0, 0, 4, 4, None, P(used), ctypes.byref(st)), 'null')
    assert refused(G(0, P(src), 2, 4, 4, 1.0, 1.0, 0, 0.0, 1.0, 0, 0, 4, 4, P(grey), None, ctypes.byref(st)), 'null')
    assert refused(G(0, P(src), 2, 4, 4, 1.0, 1.0, 0, 0.0, 1.0, 0, 0, 4, 4, P(grey), P(used), None), 'null')
    assert refused(G(0, P(src), 5, 4, 4, 1.0, 1.0, 0, 0.0, 1.0, 0, 0, *ok_tail), 'dtype 5') and st.value == 0
    assert refused(G(0, P(src), -1, 4, 4, 1.0, 1.0, 0, 0.0, 1.0, 0, 0, *ok_tail), 'dtype -1')
    assert refused(G(0, P(src), 2, 4, 4, 1.0, 1.0, 2, 0.0, 1.0, 0, 0, *ok_tail), 'cubic = 2')
    assert refused(G(0, P(src), 1, 4, 4, 1.0, 1.0, 1, 0.0, 1.0, 0, 0, *ok_tail), 'uint8', 'nearest')
    assert refused(G(0, P(src), 2, 4, 4, 1.0, 1.0, 0, float('nan'), 1.0, 0, 0, *ok_tail), 'window')
    assert refused(G(0, P(src), 2, 4, 4, 1.0, 1.0, 0, 0.0, float('inf'), 1, 0, *ok_tail), 'window')
    assert refused(G(0, P(src), 2, 1, 4, 1.0, 1.0, 1, 0.0, 1.0, 0, 0, 1, 4, P(grey), P(used), ctypes.byref(st)), 'at least 2', '1 x 4')
    assert refused(G(0, P(src), 2, 4, 4, 1.0, 2.0, 1, 0.0, 1.0, 0, 0, *ok_tail), 'out_h x out_w = 4 x 4', '4 x 8')
    assert not grey.any() and not used.any()


# ------------------------------------------------------------------------------------------------ surface
@pytest.fixture(scope='module')
def two_models():
    m1, _, _ = synthetic_model('ts2d-v2-ep4000b2_cardiac', 3, 31, network=True, mirror=False, feats=(32, 32))
    m2, _, _ = synthetic_model('ts2d-v2-ep4000b2_ribs', 4, 32, network=True, mirror=False, feats=(32, 32))
    return {'ts2d-v2-ep4000b2_cardiac': m1, 'ts2d-v2-ep4000b2_ribs': m2}


def _decode(path):
    chunks = _walk_chunks(open(path, 'rb').read())
    w, h, _, ctype = struct.unpack('>IIBB', chunks[0][1][:10])
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, -1)[:, 1:]
    return raw.reshape(h, w, 3) if ctype == 2 else raw


def test_save_writes_every_file_and_its_png_twin(tmp_path, two_models):
    """Counterpart of the reference's test_022: content='all' (the default) writes a .png beside every .nrrd, without a warning."""
    with TS2D(models=dict(two_models)) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device is None                             # no engines behind these models: the statement renders
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            files = res.save(dest=str(tmp_path), name='test', models='all', targets='all', content='all')
        names = sorted(os.path.basename(f) for f in files)
        nrrds = ['test-cardiac.nrrd', 'test-cardiac.seg.nrrd', 'test-ribs.nrrd', 'test-ribs.seg.nrrd', 'test.nrrd', 'test.seg.nrrd',
                 'test_max.nrrd', 'test_mean.nrrd']
        pngs = ['test-cardiac-ch0.png', 'test-cardiac-ch1.png', 'test-cardiac.seg.png', 'test-ribs-ch0.png', 'test-ribs-ch1.png',
                'test-ribs.seg.png', 'test.png', 'test.seg.png', 'test_max.png', 'test_mean.png']
        assert names == sorted(nrrds + pngs) and sorted(os.listdir(tmp_path)) == names
        seg = _decode(str(tmp_path / 'test.seg.png'))
        want = image.create_visual(res.get_segmentation(), labels=True, axis='coronal')
        assert seg.shape == (133, 53, 3) and np.array_equal(seg, want.array)
        mx = _decode(str(tmp_path / 'test_max.png'))
        assert mx.shape == (133, 53) and np.array_equal(mx, image.create_visual(res.get_projection('max')).array) and mx.max() == 255
        assert np.array_equal(_decode(str(tmp_path / 'test.png')), image.create_visual(res.get_input(), labels=False, axis='coronal').array)
        only = res.save(dest=str(tmp_path / 'v'), name='t', models='final', targets='segmentation', content='visual')
        assert [os.path.basename(f) for f in only] == ['t.seg.png'] and os.listdir(tmp_path / 'v') == ['t.seg.png']
        plain = res.save(dest=str(tmp_path / 'f'), name='t', models='all', targets='all', content='file')
        assert sorted(os.path.basename(f) for f in plain) == sorted(n.replace('test', 't') for n in nrrds)


def test_cli_visualize_writes_the_png_twins(tmp_path, two_models, capsys):
    """Counterpart of the reference's test_030 with --visualize."""
    src = tmp_path / 'in'
    os.makedirs(src)
    shutil.copy(os.path.join(A, 'sample_s0521.nrrd'), src / 'sample_s0521.nrrd')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ts2d_run(str(src), str(tmp_path / 'out'), models=dict(two_models), visualize=True, save_all=True, silent=True)
    out = sorted(os.listdir(tmp_path / 'out'))
    stems = ['sample_s0521-cardiac.seg', 'sample_s0521-ribs.seg', 'sample_s0521.seg', 'sample_s0521_max', 'sample_s0521_mean']
    assert out == sorted([s + '.nrrd' for s in stems] + [s + '.png' for s in stems])
    with pytest.raises(SystemExit):
        ts2d_entry_point(['--help'])
    text = capsys.readouterr().out
    assert '--visualize' in text and 'not implemented' not in text


# ------------------------------------------------------------------------------------------------ emitted instruction stream
@pytest.fixture(scope='module')
def visual_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    d = tmp_path_factory.mktemp('visual_isa')
    devflags = subprocess.check_output(['make', '-s', '-C', CSRC, 'flags'], text=True).split()
    subprocess.check_call([HIPCC, '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S', *devflags, '-o', str(d / 'visual.s'),
                           os.path.join(CSRC, 'visual.hip')], stderr=subprocess.DEVNULL)
    return open(d / 'visual.s').read()


@pytest.mark.parametrize('kernel,n_inst,n_mul,n_add', [('visual_flatten', 1, 0, 0), ('visual_label_rgb', 1, 0, 0), ('visual_prefilter_cols', 5, 40, 30),
                                                       ('visual_prefilter_rows', 1, 40, 30), ('visual_interp_cast', 5, 32, 16),
                                                       ('visual_gather_nearest', 5, 0, 0), ('visual_window', 1, 4, 4)])
def test_kernels_fuse_nothing_divide_nowhere_and_spill_nothing(visual_asm, kernel, n_inst, n_mul, n_add):
    """Every instantiation: no fused float64 multiply-add (bit identity with the statement), no division, reciprocal or floor (those are the
    host's: visual_plan.cpp), no scratch, no spills."""
    names = re.findall(rf'^(_ZN4ts2d\d+{kernel}\w*):', visual_asm, re.M)
    assert len(names) == n_inst, names
    meta = visual_asm[visual_asm.index('amdhsa.kernels:'):]
    for name in names:
        start = visual_asm.index(f'\n{name}:')
        body = visual_asm[start:visual_asm.index('.Lfunc_end', start)]
        ops = [ln.split()[0] for ln in body.split('\n') if ln.strip() and not ln.strip().startswith((';', '.'))]
        fused = [o for o in ops if 'f64' in o and ('fma' in o or 'mad' in o)]
        assert not fused, f'{name}: a float64 product was fused into its sum ({fused[0]})'
        assert sum(o == 'v_mul_f64' for o in ops) >= n_mul and sum(o == 'v_add_f64' for o in ops) >= n_add, name
        assert not [o for o in ops if o.startswith('scratch_')], f'{name} spills registers'
        assert not [o for o in ops if o.startswith(('v_rcp_', 'v_div_', 'v_floor_', 'v_exp_', 'v_log_'))], f'{name} divides, floors or takes a power on the device'
        blk = next(b for b in re.split(r'\n  - \.', meta)[1:] if name in b)
        assert re.search(r'private_segment_fixed_size:\s*0\b', blk) and re.search(r'vgpr_spill_count:\s*0\b', blk) and re.search(r'sgpr_spill_count:\s*0\b', blk), name
