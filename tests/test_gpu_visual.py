"""PNG visuals on the MI355X: the entries ts2d_visual_labels / ts2d_visual_grey (csrc/kernels_visual.h, csrc/visual.hip) against the numpy
float64 statement of totalsegmentator2d_amd/visual.py - every output byte for byte -, their refusals, and create_visual(device=0) end to end."""
import ctypes
import warnings

import numpy as np
import pytest

from totalsegmentator2d_amd import _lib, engine, image, nrrd
from totalsegmentator2d_amd import visual as V

pytestmark = pytest.mark.gpu
SPACINGS = ((1.0, 1.0), (0.8, 2.5), (3.0, 1.0), (1.0, 2.0))      # (spacing of axis 0, of axis 1); (3, 1) has an outside last row at H = 16 and 600
EYE2 = (1.0, 0.0, 0.0, 1.0)


def _geo(shape, sp):
    m = min(sp)
    return V.uniform_extent(shape[0], sp[0], m), V.uniform_extent(shape[1], sp[1], m)


def _planes(seed, K, H, W, offset=0):
    """Sparse uint8 planes [K, H, W] (a label map with values up to 200 for K = 1) in a buffer whose base is `offset` bytes off its allocation."""
    rng = np.random.default_rng(seed)
    buf = np.zeros(K * H * W + offset, np.uint8)
    p = buf[offset:].reshape(K, H, W)
    if K == 1:
        p[0] = (rng.random((H, W)) < 0.7) * rng.integers(1, 201, (H, W))
    else:
        p[:] = (rng.random((K, H, W)) < min(0.5, 2.0 / K)) * rng.integers(1, 256, (K, H, W))
        p[:, 0, 0] = 0                                           # one pixel with no plane set, one with the last, one with the first only
        p[K - 1, 0, 1] = 1
        p[:, 1, 0] = 0; p[0, 1, 0] = 9
    return p


def test_the_entries_are_there():
    lib = _lib.load()
    assert hasattr(lib, 'ts2d_visual_labels') and hasattr(lib, 'ts2d_visual_grey') and V._device_entries() is lib


@pytest.mark.parametrize('shape', [(37, 53), (16, 16)])
@pytest.mark.parametrize('K', [1, 3, 117, 255])
def test_labels_equal_the_statement(K, shape):
    """37 x 53 = 1961 pixels: no multiple of 16, so every plane but the first starts off a 16-byte boundary in the caller's buffer and the last lane
    of the flatten takes the byte path; 16 x 16 is all vector lanes.  The palette (5 colours) is shorter than the largest label."""
    pal = [(255, 255, 255), (255, 0, 0), (0, 128, 0), (1, 2, 3), (200, 100, 50)]
    for offset in (0, 1):
        planes = _planes(K * 100 + shape[0] + offset, K, *shape, offset=offset)
        assert int(planes.max()) > len(pal) or K > 1
        for sp in SPACINGS:
            want = V._labels_statement(planes, sp, pal)
            geo = V._device_geometry(shape, sp)
            assert geo is not None and geo[1] == want.shape[:2] == _geo(shape, sp)
            got = engine.visual_labels(planes, geo[0], np.asarray(pal, np.uint8), geo[1], 0)
            assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (K, shape, sp, offset, int((got != want).sum()))
        if K > 1:
            idx = V.flatten_index(planes)
            assert idx[0, 0] == 0 and idx[0, 1] == K and idx[1, 0] == 1
    assert any(not (V.axis_table(shape[0], sp[0], min(sp))['inside'].all() and V.axis_table(shape[1], sp[1], min(sp))['inside'].all())
               for sp in SPACINGS)                               # an outside row or column was among the cases (37 x 53: column 0 at (0.8, 2.5); 16 x 16: row 47 at (3, 1))


@pytest.mark.parametrize('shape', [(5, 16), (16, 17), (17, 33), (33, 5), (600, 8)])
@pytest.mark.parametrize('dtype', ['uint8', 'int16', 'float32'])
def test_grey_equals_the_statement(dtype, shape):
    """Line lengths 5, 16, 17 and 33 sit either side of the 16-sample batches of the line filter; on the 600-sample columns the powers of the pole
    pass through denormals to 0.  uint8 takes the nearest path, the others the cubic one (and the nearest one at spacing (1, 1))."""
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    if dtype == 'float32':
        planes = [(rng.normal(size=shape) * 300).astype(np.float32), np.full(shape, -2.5, np.float32)]
    elif dtype == 'int16':
        planes = [rng.integers(-1024, 3000, shape).astype(np.int16), np.full(shape, 32767, np.int16)]
        planes[0][0, :2] = (-32768, 32767)                       # an overshoot next to the type's bounds is clamped
    else:
        planes = [rng.integers(0, 256, shape).astype(np.uint8), np.full(shape, 7, np.uint8)]
    for plane in planes:
        for sp in SPACINGS:
            cubic = not V.is_uniform(sp) and dtype != 'uint8'
            geo = V._device_geometry(shape, sp)
            for window in (None, (float(plane.min()) + 3.0, float(plane.max()) - 1.5), (None, 100.0)):
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    want = V._grey_statement(plane, sp, window)
                lo, hi = (None, None) if window is None else window
                got = engine.visual_grey(plane, geo[0], cubic, lo, hi, geo[1], 0)
                assert got is not None
                out, used = got
                assert out.dtype == np.uint8 and out.shape == want.shape == _geo(shape, sp)
                assert np.array_equal(out, want), (dtype, shape, sp, window, int((out != want).sum()), int(np.abs(out.astype(int) - want).max()))
                if cubic:
                    m = min(sp)
                    res = V.resample_cubic(plane, V.axis_table(shape[0], sp[0], m), V.axis_table(shape[1], sp[1], m))
                    assert used == V.resolve_window(res, window)     # the window is that of the RESAMPLED plane, outside zeros included


def test_a_constant_plane_and_an_equal_window_give_zeros():
    plane = np.full((9, 9), 5, np.int16)
    out, used = engine.visual_grey(plane, (1.0, 1.0), False, None, None, (9, 9), 0)
    assert used == (5.0, 5.0) and not out.any() and np.array_equal(out, V._grey_statement(plane, (1.0, 1.0), None))
    out, used = engine.visual_grey(plane, (1.0, 1.0), False, 2.0, 2.0, (9, 9), 0)
    assert used == (2.0, 2.0) and not out.any()


def test_a_nan_sample_sets_the_status_bit_and_create_visual_takes_the_statement():
    rng = np.random.default_rng(5)
    plane = rng.normal(size=(20, 24)).astype(np.float32)
    plane[7, 9] = np.nan
    for sp, cubic in (((1.0, 1.0), False), ((1.0, 2.0), True)):
        geo = V._device_geometry(plane.shape, sp)
        assert engine.visual_grey(plane, geo[0], cubic, None, None, geo[1], 0) is None
        status = ctypes.c_int(0)
        out = np.full(geo[1], 77, np.uint8); used = np.full(2, -1.0)
        rc = _lib.load().ts2d_visual_grey(0, plane.ctypes.data, 2, 20, 24, geo[0][0], geo[0][1], int(cubic), 0.0, 0.0, 1, 1, geo[1][0], geo[1][1],
                                          out.ctypes.data, used.ctypes.data, ctypes.byref(status))
        assert rc == 0 and status.value == _lib.VISUAL_NONFINITE and (out == 77).all() and (used == -1.0).all()
        img = nrrd.Image(plane, (sp[1], sp[0]), (0.0, 0.0), EYE2, 1, {}, None)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                      # (numpy warns about the NaN on its way through the statement)
            a, b = image.create_visual(img, labels=False, window=(-1.0, 1.0), device=0), image.create_visual(img, labels=False, window=(-1.0, 1.0))
        assert np.array_equal(a.array, b.array)
    plane[7, 9] = np.inf
    assert engine.visual_grey(plane, (1.0, 1.0), False, None, None, plane.shape, 0) is None


def test_bad_arguments_are_refused_on_the_gpu_box_too():
    lib = _lib.load()
    planes = np.ones((2, 4, 4), np.uint8); pal = np.zeros((2, 3), np.uint8); rgb = np.zeros((4, 4, 3), np.uint8)
    grey = np.zeros((4, 4), np.uint8); used = np.zeros(2); st = ctypes.c_int(0)
    src = np.ones((4, 4), np.float32)

    def refused(rc, *words):
        return rc == -1 and all(w in _lib.last_error() for w in words)
    assert refused(lib.ts2d_visual_labels(0, None, 2, 4, 4, 1.0, 1.0, pal.ctypes.data, 2, 4, 4, rgb.ctypes.data), 'ts2d_visual_labels', 'null')
    assert refused(lib.ts2d_visual_labels(0, planes.ctypes.data, 0, 4, 4, 1.0, 1.0, pal.ctypes.data, 2, 4, 4, rgb.ctypes.data), 'K = 0')
    assert refused(lib.ts2d_visual_labels(0, planes.ctypes.data, 256, 4, 4, 1.0, 1.0, pal.ctypes.data, 2, 4, 4, rgb.ctypes.data), 'K = 256')
    assert refused(lib.ts2d_visual_grey(0, None, 2, 4, 4, 1.0, 1.0, 0, 0.0, 1.0, 0, 0, 4, 4, grey.ctypes.data, used.ctypes.data, ctypes.byref(st)),
                   'ts2d_visual_grey', 'null')
    assert refused(lib.ts2d_visual_grey(0, src.ctypes.data, 9, 4, 4, 1.0, 1.0, 0, 0.0, 1.0, 0, 0, 4, 4, grey.ctypes.data, used.ctypes.data,
                                        ctypes.byref(st)), 'dtype 9')
    assert not rgb.any() and not grey.any()
    with pytest.raises(RuntimeError, match='out_h x out_w'):
        engine.visual_labels(planes, (1.0, 2.0), pal, (4, 4), 0)


def test_create_visual_of_a_combined_segmentation_end_to_end(monkeypatch):
    """A 117-channel multilabel segmentation as combine_segmentations hands it out (plane-major memory behind the interleaved view), colours from
    its Segment* metadata: device=0 goes through ts2d_visual_labels and equals device=None; so does a float32 projection through ts2d_visual_grey."""
    rng = np.random.default_rng(11)
    K, H, W = 117, 140, 130                                     # 2.1 M plane samples: above visual.LABELS_DEVICE_MIN
    planes = (rng.random((K, H, W)) < 0.02).astype(np.uint8)
    seg = nrrd.Image(np.moveaxis(planes, 0, -1), (2.5, 0.8), (0.0, 0.0), EYE2, K, {}, None)
    image.set_annotation_meta(seg, {i + 1: f'label{i}' for i in range(K)}, {f'label{i}': tuple(int(v) for v in rng.integers(0, 256, 3)) for i in range(0, K, 2)})
    calls = []
    real_labels, real_grey = engine.visual_labels, engine.visual_grey
    monkeypatch.setattr(engine, 'visual_labels', lambda *a, **k: (calls.append('labels'), real_labels(*a, **k))[1])
    monkeypatch.setattr(engine, 'visual_grey', lambda *a, **k: (calls.append('grey'), real_grey(*a, **k))[1])
    dev = image.create_visual(seg, labels=True, axis='coronal', device=0)
    host = image.create_visual(seg, labels=True, axis='coronal')
    assert calls == ['labels'] and dev.components == 3 and K * H * W >= V.LABELS_DEVICE_MIN and dev.array.shape == host.array.shape == (H, V.uniform_extent(W, 2.5, 0.8), 3)
    assert np.array_equal(dev.array, host.array) and dev.spacing == host.spacing == (0.8, 0.8) and len(np.unique(dev.array.reshape(-1, 3), axis=0)) > 50
    proj = nrrd.Image((rng.normal(size=(H, 1, W)) * 100).astype(np.float32), (2.5, 1.0, 0.8), (0.0, 0.0, 0.0),
                      (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), 1, {}, None)
    dev, host = image.create_visual(proj, device=0), image.create_visual(proj)
    assert calls == ['labels', 'grey'] and dev.array.shape == (H, V.uniform_extent(W, 2.5, 0.8)) and np.array_equal(dev.array, host.array)
    assert image.create_visual(proj, window='pc5', device=0).array.shape == dev.array.shape and calls == ['labels', 'grey']      # percentile: host only
    # below the size gates the statement answers (it is faster there), above them the device: a grey plane that needs no resample
    small = nrrd.Image(proj.array[:, 0, :], (1.5, 1.5), (0.0, 0.0), EYE2, 1, {}, None)
    big = nrrd.Image((rng.normal(size=(512, 256)) * 100).astype(np.float32), (1.5, 1.5), (0.0, 0.0), EYE2, 1, {}, None)
    assert small.array.size < V.GREY_UNIFORM_DEVICE_MIN <= big.array.size
    image.create_visual(small, device=0)
    assert calls == ['labels', 'grey']
    assert np.array_equal(image.create_visual(big, device=0).array, image.create_visual(big).array) and calls == ['labels', 'grey', 'grey']
    few = nrrd.Image(np.moveaxis(planes[:3], 0, -1), (2.5, 0.8), (0.0, 0.0), EYE2, 3, {}, None)
    assert np.array_equal(image.create_visual(few, labels=True, device=0).array, image.create_visual(few, labels=True).array) and calls == ['labels', 'grey', 'grey']


def test_ts2d_hands_its_results_the_device_and_save_writes_the_same_pngs(tmp_path):
    """A result of a TS2D backed by HIP engines renders its visuals on their device; the files are those of the host statement, byte for byte."""
    import os
    from tests.conftest import GOLDEN
    from tests.surface_util import synthetic_model
    from totalsegmentator2d_amd.tool import TS2D
    mid = 'ts2d-v2-ep4000b2_cardiac'
    with TS2D(models={mid: synthetic_model(mid, 3, 31, patch=(128, 128), mirror=False)[0]}) as ts:
        res = ts.predict(os.path.join(GOLDEN, 'assets', 'sample_s0616.nrrd'))          # 644 x 337, two channels: above the grey gate
        assert res.device == 0
        on_device = res.save(dest=str(tmp_path / 'd'), name='c', models='final', targets='all', content='visual')
        res.device = None
        on_host = res.save(dest=str(tmp_path / 'h'), name='c', models='final', targets='all', content='visual')
    names = [os.path.basename(f) for f in on_device]
    assert names == [os.path.basename(f) for f in on_host] == ['c-ch0.png', 'c-ch1.png', 'c.seg.png', 'c_ch0.png', 'c_ch1.png']
    for a, b in zip(on_device, on_host):
        assert open(a, 'rb').read() == open(b, 'rb').read(), os.path.basename(a)
