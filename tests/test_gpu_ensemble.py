"""ts2d_ensemble_predict_tiled_export: the folds of an ensemble through ONE engine call, the mean of their float16 logits taken on the
device (csrc/kernels_fold.h) in upstream's order and rounding, the export and the threshold behind it.  What is pinned: the mean equals
``predictor.fold_mean_f16`` of the single-engine entries' bytes bit for bit; the predictor's and the model's segmentation of an ensemble
equal the host route's (``predict_logits_from_preprocessed_data`` + export) byte for byte; one engine is the single-engine entry."""
import ctypes

import numpy as np
import pytest

from tests import cases
from tests.conftest import blob_for
from totalsegmentator2d_amd import _lib, export, nrrd, prng, weights
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd import engine as engine_module
from totalsegmentator2d_amd import sliding_window as sw
from totalsegmentator2d_amd.engine import Engine, predict_tiled_export_ensemble
from totalsegmentator2d_amd.model import HIPModel
from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor, fold_mean_f16

pytestmark = pytest.mark.gpu

HALF_THRESHOLD = 1.5 * 2.0 ** -24          # sigmoid(float(half logit)) > 0.5 on the half grid (export.py)
ARCH = cases.unet(3, (32, 32, 64), 3)
PATCH = (64, 64)


def _plan(data, patch=PATCH, step=0.5):
    """[C,H,W] -> the padded image, its tile list and the rectangle (y, x, h, w) of the case in it, as the predictor makes them."""
    padded, revert = sw.pad_nd_image(np.asarray(data, np.float32)[:, None], patch)
    tiles = [(y, x) for (_, y, x) in sw.tile_slicers(padded.shape[2:], patch, step, 1)]
    return np.ascontiguousarray(padded[:, 0]), tiles, (revert[2].start, revert[3].start) + tuple(data.shape[1:])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _same16(a, b):
    return a.dtype == b.dtype == np.float16 and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _engines(n, arch=ARCH, seed0=70, precision='split', order='float', **kw):
    es = [Engine(arch, blob_for(arch, seed0 + f)[1], **kw) for f in range(n)]
    for e in es:
        e.set_precision(precision)
        e.set_tile_dtype(order)
    return es


def _close(es):
    for e in es:
        e.close()


# ------------------------------------------------------------------------------------------------ the mean kernel
@pytest.mark.parametrize('precision', ['split', 'f16'])
@pytest.mark.parametrize('order', ['float', 'half'])
def test_mean_of_the_folds_equals_the_numpy_statement_of_the_single_engine_bytes(order, precision):
    """3 x 65 x 67 and 3 x 73 x 66 elements are no multiples of 8 (the scalar tail of the kernel), 3 x 80 x 72 is; the mean runs over
    every slot up to the end of the LAST image, so each takes the last place once."""
    g = sw.compute_gaussian(PATCH)
    plans = [_plan(prng.normal_f32(11, i, (ARCH.input_channels,) + hw)) for i, hw in enumerate([(65, 67), (80, 72), (73, 66)])]
    es = _engines(5, precision=precision, order=order)
    try:
        for order_of_images in ([0, 1, 2], [1, 2, 0], [2, 0, 1]):
            imgs, tiles = [plans[i][0] for i in order_of_images], [plans[i][1] for i in order_of_images]
            folds = [e.predict_tiled_batch(imgs, PATCH, tiles, (0, 1), g)[0] for e in es]
            assert not _same16(folds[0][0], folds[1][0])
            for F in (2, 3, 5):
                seg, f32, mean, pseg = predict_tiled_export_ensemble(es[:F], imgs, PATCH, tiles, None, (0, 1), g, want_seg=False,
                                                                     want_logits=True, want_padded_seg=True)
                assert seg is None and f32 is None
                for i in range(len(imgs)):
                    want = fold_mean_f16([folds[f][i] for f in range(F)])
                    assert _same16(mean[i], want), (F, i, order_of_images)
                    assert np.array_equal(pseg[i], (want.astype(np.float32) > HALF_THRESHOLD).astype(np.uint8))
                    assert 0 < pseg[i].mean() < 1
                assert es[0].last_tiled_inf_per_image == [False] * 3 and not any(e.last_tiled_inf for e in es[:F])
        # the segmentation alone: nothing but the uint8 planes asked for, the same bytes
        only = predict_tiled_export_ensemble(es[:3], imgs, PATCH, tiles, None, (0, 1), g, want_seg=False, want_padded_seg=True)
        ref = predict_tiled_export_ensemble(es[:3], imgs, PATCH, tiles, None, (0, 1), g, want_seg=False, want_logits=True, want_padded_seg=True)
        assert only[2] is None and all(np.array_equal(a, b) for a, b in zip(only[3], ref[3]))
    finally:
        _close(es)


def test_the_export_of_an_ensemble_is_the_export_of_its_mean():
    """Resample-back and threshold behind the mean: the numpy statement of the export (preprocess.resize_linear_f64) on fold_mean_f16."""
    g = sw.compute_gaussian(PATCH)
    plans = [_plan(prng.normal_f32(12, i, (ARCH.input_channels,) + hw)) for i, hw in enumerate([(90, 70), (64, 64), (50, 100)])]
    outs = [(120, 61), (64, 64), (77, 130)]
    imgs, tiles, rects = ([p[j] for p in plans] for j in range(3))
    ex = [r + o for r, o in zip(rects, outs)]
    es = _engines(3)
    try:
        for full in (True, False):
            seg, f32, mean, _ = predict_tiled_export_ensemble(es, imgs, PATCH, tiles, ex, (0, 1), g, want_f32=True, want_logits=True, full_batch=full)
            for i, (y, x, h, w) in enumerate(rects):
                folds = [e.predict_tiled_export([imgs[i]], PATCH, [tiles[i]], [ex[i]], (0, 1), g, want_logits=True, full_batch=full)[2][0] for e in es]
                want = fold_mean_f16(folds)
                assert _same16(mean[i], want)
                rs = np.stack([P.resize_linear_f64(pl[y:y + h, x:x + w].astype(np.float32), outs[i]) for pl in want])
                assert rs.dtype == np.float32 and np.array_equal(f32[i].view(np.uint32), rs.view(np.uint32))
                assert np.array_equal(seg[i], (f32[i] > HALF_THRESHOLD).astype(np.uint8))
    finally:
        _close(es)


def test_one_engine_is_the_single_engine_entry_byte_for_byte():
    g = sw.compute_gaussian(PATCH)
    plans = [_plan(prng.normal_f32(13, i, (ARCH.input_channels,) + hw)) for i, hw in enumerate([(90, 70), (65, 67)])]
    imgs, tiles, rects = ([p[j] for p in plans] for j in range(3))
    ex = [rects[0] + (120, 61), rects[1] + rects[1][2:]]
    es = _engines(1)
    try:
        e = es[0]
        for full in (True, False):
            a = e.predict_tiled_export(imgs, PATCH, tiles, ex, (0, 1), g, want_f32=True, want_logits=True, want_padded_seg=True, full_batch=full)
            b = predict_tiled_export_ensemble(es, imgs, PATCH, tiles, ex, (0, 1), g, want_f32=True, want_logits=True, want_padded_seg=True,
                                              full_batch=full)
            for x, y in zip(a, b):
                assert all(u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(x, y))
        l16, pseg = e.predict_tiled_batch(imgs, PATCH, tiles, (0, 1), g, want_logits=True, want_seg=True)
        _, _, m16, mseg = predict_tiled_export_ensemble(es, imgs, PATCH, tiles, None, (0, 1), g, want_seg=False, want_logits=True,
                                                        want_padded_seg=True)
        assert all(_same16(u, v) for u, v in zip(l16, m16)) and all(np.array_equal(u, v) for u, v in zip(pseg, mseg))
        assert e.lib.ts2d_ensemble_predict_tiled_export((ctypes.c_void_p * 1)(e._h), 1, None, None, 0, 64, 64, 3, None, 1) == 0     # nothing to do
    finally:
        _close(es)


# ------------------------------------------------------------------------------------------------ inf: arithmetic, per fold and per image
def test_an_inf_in_one_fold_of_one_image_is_flagged_there_and_the_predictor_names_the_input():
    """The head-bias recipe of the single-engine test in ONE fold of three: without Gaussian weighting the float16 accumulator holds the
    SUM of the overlapping tiles, so a bias of 40 000 stays finite where one tile covers a pixel and passes 65 504 where two do.  The
    fp32 tile logits are finite throughout (ts2d_engine_check has nothing to report): only that fold's aggregated half value overflows,
    and upstream looks for inf in every fold's array, not in the mean."""
    arch, shape, patch, step, mirror, _, seed = cases.SW_CASES['sw_2tiles_mirror']
    sds = [dict(blob_for(arch, seed + f)[0]) for f in range(3)]
    key = [k for k in sds[1] if 'seg_layers' in k and k.endswith('bias')][-1]
    sds[1][key] = np.full_like(sds[1][key], 4e4)
    two_tiles = prng.normal_f32(seed, 999, (arch.input_channels,) + tuple(shape))          # 80 x 52 -> 2 tiles of 64 x 64
    one_tile = prng.normal_f32(seed, 998, (arch.input_channels, 1, 60, 50))
    p = HIPnnUNetPredictor(tile_step_size=step, use_mirroring=True, use_gaussian=False)
    p.manual_initialization(arch, [weights.pack_blob(arch, sd) for sd in sds], patch, inference_allowed_mirroring_axes=mirror)
    try:
        ok = p.predict_segmentation_from_preprocessed_data_batch([one_tile, one_tile])
        assert ok is not None and not any(e.last_tiled_inf for e in p.engines)
        with pytest.raises(RuntimeError, match='input 1: Encountered inf in predicted array'):
            p.predict_segmentation_from_preprocessed_data_batch([one_tile, two_tiles, one_tile])
        assert p.engines[0].last_tiled_inf_per_image == [False, True, False]
        assert [e.last_tiled_inf for e in p.engines] == [False, True, False]
        assert [e.lib.ts2d_engine_tiled_inf_flag(e._h) for e in p.engines] == [0, 1, 0]
        with pytest.raises(RuntimeError, match='^Encountered inf in predicted array'):
            p.predict_segmentation_from_preprocessed_data(two_tiles)
        with pytest.raises(RuntimeError, match='^Encountered inf in predicted array'):          # ... as the host statement does
            p.predict_logits_from_preprocessed_data(two_tiles)
        assert p.predict_segmentation_from_preprocessed_data(one_tile) is not None
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ the predictor
def _props(hw):
    hw = tuple(int(v) for v in hw)
    return {'shape_after_cropping_and_before_resampling': (1,) + hw, 'shape_before_cropping': (1,) + hw,
            'bbox_used_for_cropping': [(0, 1), (0, hw[0]), (0, hw[1])]}


def _host_seg(logits, hw):
    lg = logits.cpu().numpy() if hasattr(logits, 'cpu') else logits
    return export.convert_predicted_logits_to_segmentation_with_correct_shape(lg, _props(hw))


@pytest.mark.parametrize('mirror', [None, (0, 1)])
def test_the_predictors_segmentation_of_an_ensemble_equals_the_host_route(mirror, monkeypatch):
    arch, shape, patch, step, _, folds, seed = cases.SW_CASES['sw_folds_nomirror']
    assert folds == 2
    blobs = [blob_for(arch, seed + f)[1] for f in range(folds)]
    data = prng.normal_f32(seed, 999, (arch.input_channels,) + tuple(shape))
    more = [prng.normal_f32(seed, 990 + i, (arch.input_channels, 1) + hw) for i, hw in enumerate([(70, 64), (131, 90)])]
    p = HIPnnUNetPredictor(tile_step_size=step, use_mirroring=mirror is not None)
    p.manual_initialization(arch, blobs, patch, inference_allowed_mirroring_axes=mirror)
    try:
        calls = []
        orig = engine_module.predict_tiled_export_ensemble          # the predictor looks it up at call time: calls INTO THE LIBRARY are counted
        monkeypatch.setattr(engine_module, 'predict_tiled_export_ensemble',
                            lambda engines, images, *a, **kw: (calls.append(len(images)), orig(engines, images, *a, **kw))[1])
        lg = p.predict_logits_from_preprocessed_data(data)
        for out_shape in (None, (1, 150, 111)):
            seg = p.predict_segmentation_from_preprocessed_data(data, **({} if out_shape is None else {'out_shape': out_shape}))
            hw = tuple(shape[1:]) if out_shape is None else out_shape[1:]
            assert seg is not None and seg.dtype == np.uint8 and seg.shape == (arch.num_classes, 1) + tuple(hw)
            assert np.array_equal(seg, _host_seg(lg, hw)) and 0 < seg.mean() < 1
        assert calls == [1, 1]
        datas = [data] + more
        lgs = p.predict_logits_from_preprocessed_data_batch(datas)
        for out_shapes in (None, [(1, 150, 111), None, (90, 131)]):
            segs = p.predict_segmentation_from_preprocessed_data_batch(datas, **({} if out_shapes is None else {'out_shapes': out_shapes}))
            assert segs is not None and len(segs) == 3
            for i, (d, l, s) in enumerate(zip(datas, lgs, segs)):
                hw = d.shape[2:] if out_shapes is None or out_shapes[i] is None else tuple(out_shapes[i])[-2:]
                assert s.dtype == np.uint8 and np.array_equal(s, _host_seg(l, hw)), (i, out_shapes)
        assert calls == [1, 1, 3, 3]
        assert p.predict_segmentation_from_preprocessed_data(np.concatenate([data, data], axis=1)) is None        # a z-stack needs the logits
        assert p.predict_segmentation_from_preprocessed_data_batch([]) == []
    finally:
        p.close()


def test_full_batch_bytes_do_not_depend_on_the_batch_and_equal_the_sbk0_twins():
    g = sw.compute_gaussian(PATCH)
    plans = [_plan(prng.normal_f32(14, i, (ARCH.input_channels,) + hw)) for i, hw in enumerate([(90, 70), (65, 67), (64, 128)])]
    imgs, tiles = [p[0] for p in plans], [p[1] for p in plans]
    es, twins = _engines(3), _engines(3, options={'sbk': 0})
    try:
        def run(idx):
            return predict_tiled_export_ensemble(es, [imgs[i] for i in idx], PATCH, [tiles[i] for i in idx], None, (0, 1), g, want_seg=False,
                                                 want_logits=True)[2]
        alone, abc, cab = run([0]), run([0, 1, 2]), run([2, 0, 1])
        assert _same16(alone[0], abc[0]) and _same16(alone[0], cab[1]) and _same16(abc[2], cab[0]) and _same16(abc[1], cab[2])
        for i in range(3):
            want = fold_mean_f16([t.predict_tiled(imgs[i], PATCH, tiles[i], (0, 1), g)[0] for t in twins])
            assert _same16(abc[i], want)
    finally:
        _close(es + twins)


# ------------------------------------------------------------------------------------------------ the surface
def _two_fold_model(K=4, seed=81, patch=PATCH):
    arch = cases.unet(3, (32, 32, 64), K)
    blobs = [blob_for(arch, seed + f)[1] for f in range(2)]
    ds = {'channel_names': {'0': 'mean', '1': 'max'}, 'labels': {'background': 0, **{f'cardiac_{i + 1}': i + 1 for i in range(K)}},
          'file_ending': '.nrrd', 'multilabel': True}
    return HIPModel({'model': 'ts2d-v2-ep4000b2_cardiac', 'revision': 1, 'param': {},
                     'synthetic': {'arch': arch, 'blobs': blobs, 'patch_size': patch, 'dataset_json': ds}})


def _image(hw, spacing, seed):
    return nrrd.Image((np.random.default_rng(seed).standard_normal(tuple(hw) + (2,)) * 200 + 50).astype(np.float32), spacing, (0.0, 0.0),
                      (1.0, 0.0, 0.0, 1.0), 2, {}, None)


def test_apply_and_apply_batch_of_a_two_fold_model_equal_the_host_route(monkeypatch):
    cases_ = [_image((100, 90), (1.5, 1.5), 1), _image((150, 128), (0.8, 1.0), 2), _image((70, 131), (1.5, 1.5), 3)]
    m = _two_fold_model()
    m.start()
    try:
        p = m._predictor
        assert len(p.engines) == 2 and p._device_ensemble()
        calls = []
        orig = engine_module.predict_tiled_export_ensemble          # the predictor looks it up at call time: calls INTO THE LIBRARY are counted
        monkeypatch.setattr(engine_module, 'predict_tiled_export_ensemble',
                            lambda engines, images, *a, **kw: (calls.append(len(images)), orig(engines, images, *a, **kw))[1])
        m.device_threshold = False
        host = [m.apply(c) for c in cases_]
        host_many = m.apply_batch(cases_)
        assert not calls
        m.device_threshold = True
        dev = []
        for c in cases_:
            dev.append(m.apply(c))
            assert {'start', 'preprocessed', 'predicted', 'exported', 'done'} <= set(m.timestamps)
        assert calls == [1, 1, 1]
        dev_many = m.apply_batch(cases_)
        assert calls == [1, 1, 1, 3]                               # ONE engine call: every fold, resampled and un-resampled cases together
        assert all({'start', 'preprocessed', 'predicted', 'exported', 'done'} <= set(t) for t in m.batch_timestamps.values())
        for c, h, d, (hn, hm), (dn, dm) in zip(cases_, host, dev, host_many.items(), dev_many.items()):
            assert hn == dn and h.array.shape == d.array.shape and h.array.any()
            assert np.array_equal(h.array, d.array) and np.array_equal(hm.array, dm.array)
            assert d.spacing == c.spacing and d.size == c.size
    finally:
        m.stop()


# ------------------------------------------------------------------------------------------------ errors and scratch
def test_mismatched_folds_and_bad_images_are_refused_by_name_and_nothing_is_written():
    g = None
    img, tl, rect = _plan(prng.normal_f32(15, 0, (ARCH.input_channels, 80, 64)))
    imgs, tiles = [img] * 3, [tl] * 3
    other_k = cases.unet(3, (32, 32, 64), 4)
    es = _engines(2)
    odd = Engine(other_k, blob_for(other_k, 90)[1])
    bare = Engine(ARCH, None)
    try:
        def refuse(engines, message, code=-1):
            with pytest.raises(RuntimeError) as ei:
                predict_tiled_export_ensemble(engines, imgs, PATCH, tiles, None, (0, 1), g, want_seg=False, want_logits=True)
            assert message in str(ei.value) and f'({code})' in str(ei.value), str(ei.value)
        refuse([es[0], es[1], odd], 'fold 2 has num_classes 4, fold 0 has 3')
        es[1].set_precision('f16')
        refuse(es, 'fold 1 runs precision mode 2, fold 0 mode 1')
        es[1].set_precision('split')
        es[1].set_tile_dtype('half')
        refuse(es, 'fold 1 blends with tile dtype 1, fold 0 with 0')
        es[1].set_tile_dtype('float')
        refuse([es[0], bare], 'fold 1: weights not loaded', code=-4)
        # per image: the words of the single-engine entry, and the arrays stay as they were
        K = ARCH.num_classes
        l16 = [np.full((K, 80, 64), 7, np.float16) for _ in range(3)]
        ty, tx = np.array([0, 16], np.int32), np.zeros(2, np.int32)
        bad_ty = np.array([0, 17], np.int32)
        desc = (_lib.TiledImage * 3)()
        for i in range(3):
            d = desc[i]
            d.image, d.Hp, d.Wp, d.n_tiles = img.ctypes.data, 80, 64, 2
            d.tile_y, d.tile_x, d.logits_f16, d.seg_u8 = (bad_ty if i == 1 else ty).ctypes.data, tx.ctypes.data, l16[i].ctypes.data, None
        handles = (ctypes.c_void_p * 2)(es[0]._h, es[1]._h)
        lib = es[0].lib
        assert lib.ts2d_ensemble_predict_tiled_export(handles, 2, desc, None, 3, 64, 64, 3, None, 1) == -1
        ensemble_words = _lib.last_error()
        assert lib.ts2d_engine_predict_tiled_batch(es[0]._h, desc, 3, 64, 64, 3, None) == -1
        assert ensemble_words == _lib.last_error() == 'image 1: tile 1 at (17,0) leaves the 80x64 image'
        desc[1].tile_y = ty.ctypes.data
        desc[2].logits_f16 = None
        assert lib.ts2d_ensemble_predict_tiled_export(handles, 2, desc, None, 3, 64, 64, 3, None, 1) == -1
        assert _lib.last_error() == 'image 2: both outputs are null'
        assert all((a.view(np.uint16) == np.float16(7).view(np.uint16)).all() for a in l16) and all(desc[i].inf_flag == 0 for i in range(3))
        desc[2].logits_f16 = l16[2].ctypes.data
        assert lib.ts2d_ensemble_predict_tiled_export(handles, 2, desc, None, 3, 64, 64, 3, None, 1) == 0
        assert all(np.isfinite(a.astype(np.float32)).all() and (a != 7).any() for a in l16)
    finally:
        _close(es + [odd, bare])


def test_only_the_half_buffers_exist_once_per_fold():
    """engines[0] holds all scratch: three folds cost the half outputs of two more folds (and a few flags), not three tile scratches."""
    g = sw.compute_gaussian(PATCH)
    plans = [_plan(prng.normal_f32(16, i, (ARCH.input_channels,) + hw)) for i, hw in enumerate([(90, 70), (65, 67), (128, 128)])]
    imgs, tiles, rects = ([p[j] for p in plans] for j in range(3))
    ex = [r + r[2:] for r in rects]
    K, C = ARCH.num_classes, ARCH.input_channels
    grown = {}
    for F in (1, 3):
        es = _engines(3)
        try:
            before = [e.device_bytes() for e in es]
            predict_tiled_export_ensemble(es[:F], imgs, PATCH, tiles, ex, (0, 1), g)
            grown[F] = [e.device_bytes() - b for e, b in zip(es, before)]
        finally:
            _close(es)
    half = sum(-(-K * im.shape[1] * im.shape[2] // 256) * 256 * 2 for im in imgs)          # one fold's half outputs, 256-element aligned
    rows = max(len(t) for t in tiles) * 4                     # (the largest image: no more than the fullest chunk)
    tile_scratch = rows * (K + C) * PATCH[0] * PATCH[1] * 4
    extra = grown[3][0] - grown[1][0]
    assert 2 * half <= extra <= 2 * half + 1024, (extra, half)
    assert extra < tile_scratch
    # the later folds hold their activation workspace and nothing of the sliding window; folds that did not run hold nothing
    assert grown[1][1] == grown[1][2] == 0 and 0 < grown[3][1] == grown[3][2] < grown[3][0] - 2 * half
