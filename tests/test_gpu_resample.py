"""The device export on the MI355X: ts2d_engine_predict_tiled_export (sliding window + order-1 resample-back + threshold in one call)
against the existing entries followed by the numpy statement of the resampling (preprocess.resize_linear_f64) and the export
predicate - every mask byte and every bit of the resampled logits - and the product surface (HIPModel / TS2D.predict / predict_many)
on cases whose spacing is not the plan's against its own host route (``device_threshold = False``).  Product dispatch throughout."""
import os

import numpy as np
import pytest

from tests import cases
from tests.conftest import GOLDEN, blob_for
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, nrrd, prng
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd import sliding_window as sw
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.engine import Engine
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu

A = os.path.join(GOLDEN, 'assets')
THR = np.float32(1.5 * 2.0 ** -24)
# (input extent, export extent): up by 1.6 - 1.7 with an input narrower than the patch (the source rectangle lies inside the padded image)
# and extents that are no multiples of 4; identity; down by 2.4 / 1.6; mixed (up 2.1, down 1.8); up by 2 / 3 on multiples of 4
GEOMETRIES = [((80, 52), (131, 87)), ((100, 130), (100, 130)), ((96, 72), (40, 45)), ((70, 90), (150, 50)), ((64, 64), (128, 192))]


def _plan(data, patch, step):
    """[C,H,W] -> the padded image, its tiles and the rectangle of the padded extent that is the input."""
    padded, revert = sw.pad_nd_image(np.asarray(data, np.float32)[:, None], patch)
    H, W = padded.shape[2:]
    tiles = [(y, x) for (_, y, x) in sw.tile_slicers((H, W), patch, step, 1)]
    return np.ascontiguousarray(padded[:, 0]), tiles, (revert[2].start, revert[3].start) + tuple(data.shape[1:])


def _expected(l16, rect, out_hw):
    y, x, h, w = rect
    f32 = np.stack([P.resize_linear_f64(pl[y:y + h, x:x + w].astype(np.float32), out_hw) for pl in l16])
    return f32, (f32 > THR).astype(np.uint8)


def _check(e, imgs, tiles, rects, outs, patch, mirror, g, full):
    """The export call on these images against the existing entry of the same dispatch + the numpy statement."""
    ex = [r + tuple(o) for r, o in zip(rects, outs)]
    seg, f32, l16, pseg = e.predict_tiled_export(imgs, patch, tiles, ex, mirror, g, want_seg=True, want_f32=True, want_logits=True,
                                                 want_padded_seg=True, full_batch=full)
    if full:
        r16, rseg = e.predict_tiled_batch(imgs, patch, tiles, mirror, g, want_logits=True, want_seg=True)
    else:
        assert len(imgs) == 1
        a, b = e.predict_tiled(imgs[0], patch, tiles[0], mirror, g, want_logits=True, want_seg=True)
        r16, rseg = [a], [b]
    for i in range(len(imgs)):
        assert np.array_equal(l16[i].view(np.uint16), r16[i].view(np.uint16)) and np.array_equal(pseg[i], rseg[i]), i
        wf, ws = _expected(r16[i], rects[i], outs[i])
        assert f32[i].shape == wf.shape and seg[i].shape == ws.shape
        assert np.array_equal(f32[i].view(np.uint32), wf.view(np.uint32)), (i, float(np.abs(f32[i] - wf).max()))
        assert np.array_equal(seg[i], ws), i
        if tuple(outs[i]) == tuple(rects[i][2:]):          # identity extent: the un-resampled segmentation of the rectangle
            y, x, h, w = rects[i]
            assert np.array_equal(seg[i], rseg[i][:, y:y + h, x:x + w])
        assert 0 < seg[i].mean() < 1
    # the segmentation alone (no half logits, no float output travel to the host): the same bytes
    only = e.predict_tiled_export(imgs, patch, tiles, ex, mirror, g, full_batch=full)
    assert only[1] is None and only[2] is None and only[3] is None
    assert all(np.array_equal(a, b) for a, b in zip(only[0], seg))
    assert e.last_tiled_inf is False and e.last_tiled_inf_per_image == [False] * len(imgs)
    return seg, f32


@pytest.mark.parametrize('precision', ['split', 'f16'])
def test_export_equals_the_existing_entries_plus_the_numpy_statement(precision):
    arch, _, patch, step, mirror, _, seed = cases.SW_CASES['sw_2tiles_mirror']
    blob = blob_for(arch, seed)[1]
    g = sw.compute_gaussian(patch)
    plans = [_plan(prng.normal_f32(seed, 300 + i, (arch.input_channels,) + hw), patch, step) for i, (hw, _) in enumerate(GEOMETRIES)]
    outs = [o for _, o in GEOMETRIES]
    with Engine(arch, blob) as e:
        e.set_precision(precision)
        e.set_tile_dtype('half' if precision == 'f16' else 'float')
        for (img, tl, rect), out in zip(plans, outs):            # size-dependent dispatch, one image per call
            _check(e, [img], [tl], [rect], [out], patch, mirror, g, full=False)
        # full-batch dispatch: three images of different extents and ratios in one call, the middle one un-resampled
        imgs, tiles, rects = ([p[j] for p in plans[:3]] for j in range(3))
        seg3, f3 = _check(e, imgs, tiles, rects, outs[:3], patch, mirror, g, full=True)
        # ... all five, and batch independence: an image alone = the same image among others
        seg5, f5 = _check(e, [p[0] for p in plans], [p[1] for p in plans], [p[2] for p in plans], outs, patch, mirror, g, full=True)
        for i in (0, 3):
            s1, f1 = _check(e, [plans[i][0]], [plans[i][1]], [plans[i][2]], [outs[i]], patch, mirror, g, full=True)
            assert np.array_equal(s1[0], seg5[i]) and np.array_equal(f1[0].view(np.uint32), f5[i].view(np.uint32))
        assert all(np.array_equal(a, b) for a, b in zip(seg3, seg5[:3]))


def test_export_on_the_canonical_net():
    """The canonical five-sub-model geometry at one size: 26 heads on a 512 x 512 patch, 560 x 384 network extent -> 840 x 480."""
    arch = UNetArch.canonical()
    blob = blob_for(arch, 1)[1]
    patch = (512, 512)
    img, tl, rect = _plan(prng.normal_f32(7, 1, (arch.input_channels, 560, 384)), patch, 0.5)
    with Engine(arch, blob) as e:
        _check(e, [img], [tl], [rect], [(840, 478)], patch, (0, 1), sw.compute_gaussian(patch), full=False)


def test_bad_exports_are_rejected_by_name_before_any_device_work():
    arch, _, patch, step, mirror, _, seed = cases.SW_CASES['sw_2tiles_mirror']
    blob = blob_for(arch, seed)[1]
    K = arch.num_classes
    imgs = [prng.normal_f32(seed, 100 + i, (arch.input_channels, 80, 64)) for i in range(3)]
    ty = np.array([0, 16], np.int32); tx = np.zeros(2, np.int32)
    with Engine(arch, blob) as e:
        segs = [np.full((K, 50, 40), 7, np.uint8) for _ in range(3)]
        f32 = [np.full((K, 50, 40), 7, np.float32) for _ in range(3)]
        l16 = [np.full((K, 80, 64), 7, np.float16) for _ in range(3)]
        desc, exd = (_lib.TiledImage * 3)(), (_lib.TiledExport * 3)()

        def fill():
            for i in range(3):
                d, x = desc[i], exd[i]
                d.image, d.Hp, d.Wp, d.n_tiles = imgs[i].ctypes.data, 80, 64, 2
                d.tile_y, d.tile_x, d.logits_f16, d.seg_u8 = ty.ctypes.data, tx.ctypes.data, l16[i].ctypes.data, None
                x.src_y, x.src_x, x.src_h, x.src_w, x.out_h, x.out_w = 4, 2, 70, 60, 50, 40
                x.seg_u8, x.logits_f32 = segs[i].ctypes.data, f32[i].ctypes.data

        def call(full=1):
            return e.lib.ts2d_engine_predict_tiled_export(e._h, desc, exd, 3, 64, 64, 3, None, full)

        def untouched():
            return all((a == 7).all() for a in segs + f32 + l16)
        bad = [(1, dict(src_h=0), 'image 1: export: source rectangle 0x60 at (4,2) is empty or leaves the 80x64 image'),
               (2, dict(src_y=11), 'image 2: export: source rectangle 70x60 at (11,2) is empty or leaves'),
               (0, dict(src_x=-1), 'image 0: export: source rectangle'),
               (1, dict(src_w=63), 'image 1: export: source rectangle 70x63 at (4,2)'),
               (2, dict(out_h=0), 'image 2: export: bad output extent 0x40'),
               (1, dict(out_w=-3), 'image 1: export: bad output extent 50x-3'),
               (0, dict(out_h=1 << 15, out_w=1 << 15), 'image 0: export: 32768x32768 exceeds 2^31 output elements'),
               (1, dict(seg_u8=None, logits_f32=None), 'image 1: export: both outputs are null')]
        for i, fields, message in bad:
            for full in (0, 1):
                fill()
                for k, v in fields.items():
                    setattr(exd[i], k, v)
                assert call(full) == -1 and message in _lib.last_error(), (_lib.last_error(), message)
                assert untouched()
        fill()
        desc[2].n_tiles = 0
        assert call() == -1 and 'image 2: bad tiling' in _lib.last_error() and untouched()
        assert e.lib.ts2d_engine_predict_tiled_export(e._h, None, None, 0, 64, 64, 3, None, 1) == 0        # nothing to do
        assert e.lib.ts2d_engine_predict_tiled_export(e._h, desc, None, 3, 64, 64, 3, None, 1) == -1 and 'null pointer' in _lib.last_error()
        fill()
        for i in range(3):
            desc[i].logits_f16 = None                       # both outputs of ts2d_tiled_image NULL: allowed here, the export asks for something
        assert call() == 0
        assert all(s.max() <= 1 for s in segs) and all(np.isfinite(f).all() and (f != 7).any() for f in f32) and all((a == 7).all() for a in l16)
        with pytest.raises(RuntimeError, match='2 tile lists and 3 exports'):
            e.predict_tiled_export(imgs, (64, 64), [[(0, 0)]] * 2, [(0, 0, 80, 64, 8, 8)] * 3)


# ------------------------------------------------------------------------------------------------ surface
IDS = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_ribs')


def _relabelled(name, spacing):
    img = nrrd.read(os.path.join(A, name))
    return nrrd.Image(img.array, tuple(float(v) for v in spacing), img.origin, img.direction, img.components, dict(img.meta), img.space)


def _same_geometry(seg, img):
    return seg.spacing == img.spacing and seg.origin == img.origin and seg.direction == img.direction and seg.size == img.size


def test_resampled_cases_through_the_surface_equal_the_host_route():
    """Cases off the plan spacing (1.5 mm) through TS2D.predict and predict_many: the device export's segmentation equals the host
    route's (float16 logits to the host, scipy order 1, threshold) byte for byte, in the input's geometry."""
    inputs = [_relabelled('sample_s0616.nrrd', (0.9, 1.2)), _relabelled('sample_s0616.nrrd', (2.5, 2.0)),
              _relabelled('sample_s0521.nrrd', (0.8, 0.8, 2.0)), nrrd.read(os.path.join(A, 'sample_s0616.nrrd'))]
    models = {m: synthetic_model(m, 3 + 2 * i, 41 + i, patch=(64, 64), mirror=True)[0] for i, m in enumerate(IDS)}
    for m in models.values():
        m.start()
    seen = []
    with TS2D(models=models) as ts:
        for m in models.values():                            # witness: the export entry really serves the resampled cases
            eng = m._predictor.engines[0]
            orig = eng.predict_tiled_export
            eng.predict_tiled_export = lambda *a, _o=orig, **kw: (seen.append(len(a[0])), _o(*a, **kw))[1]
        for m in models.values():
            m.device_threshold = False
        host = [ts.predict(i) for i in inputs]
        host_many = ts.predict_many(inputs)
        assert not seen
        for m in models.values():
            m.device_threshold = True
        dev = [ts.predict(i) for i in inputs]
        assert seen and all(n == 1 for n in seen)
        del seen[:]
        dev_many = ts.predict_many(inputs)
        assert seen == [len(inputs)] * len(models)           # ONE engine call per sub-model: resampled and un-resampled cases together
        for img, h, hm, d, dm in zip(inputs, host, host_many, dev, dev_many):
            for mid in [None] + list(IDS):
                a, b = h.get_segmentation(mid), d.get_segmentation(mid)
                assert a.array.dtype == b.array.dtype == np.uint8 and np.array_equal(a.array, b.array) and a.meta == b.meta, mid
                assert np.array_equal(hm.get_segmentation(mid).array, dm.get_segmentation(mid).array), mid
                assert _same_geometry(b, a) and _same_geometry(dm.get_segmentation(mid), a), mid
                if img.dimension == 2:
                    assert _same_geometry(b, img), mid
            assert 0 < d.get_segmentation().array.mean() < 1
