"""The device export of a LABEL-MAP model on the MI355X: the kernel sw_labelmap (csrc/kernels_labelmap.h) on crafted planes through
ts2d_labelmap_from_logits, the engine entry ts2d_ensemble_predict_tiled_labelmap (one model and fold ensembles) against the numpy
statement ``export.labelmap_statement`` of the half logits the same call returns, and the product surface (a non-multilabel model folder
through HIPModel.apply / apply_batch and TS2D.predict) against its own host route (``device_labelmap = False``).  Every comparison is
exact: both routes decide on the same float32 values."""
import json
import os

import numpy as np
import pytest

from tests import cases
from tests.conftest import GOLDEN, blob_for
from totalsegmentator2d_amd import engine as engine_module
from totalsegmentator2d_amd import export, nrrd, prng, weights
from totalsegmentator2d_amd import sliding_window as sw
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.engine import Engine, labelmap_from_logits, predict_tiled_labelmap_ensemble
from totalsegmentator2d_amd.model import HIPModel
from totalsegmentator2d_amd.predictor import fold_mean_f16
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu

A = os.path.join(GOLDEN, 'assets')
ARCH = cases.unet(3, (32, 32, 64), 5)
PATCH = (64, 64)


def _h(bits):
    return np.array(bits, np.uint16).view(np.float16)


def _crafted(K, H, W, seed):
    """Half planes [K,H,W] no network produces: few distinct values (exact ties across heads), signed zeros, subnormals, the largest
    halves, and sprinkled over them +-inf heads and NaN heads."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([_h([0x0000, 0x8000, 0x0001, 0x8001, 0x0002, 0x03FF, 0x0400, 0x3C00, 0x3C01, 0x3BFF, 0xBC00, 0x7BFF, 0xFBFF]),
                           (rng.standard_normal(6) * 2).astype(np.float16)])
    lg = rng.choice(pool, size=(K, H, W))
    flat = lg.reshape(-1)
    n = flat.size
    flat[rng.integers(0, n, max(2, n // 60))] = np.inf
    flat[rng.integers(0, n, max(2, n // 60))] = -np.inf
    flat[rng.integers(0, n, max(2, n // 90))] = np.nan
    flat[rng.integers(0, n, max(1, n // 200))] = _h(0xFE01)          # a NaN of another sign and payload
    return lg


# (K, plane extent, rectangle (y, x, h, w), export extent): identity on 8-byte aligned quads, identity off them and with a width that is
# no multiple of 4, up, down, mixed with one axis kept, widths 1 .. 3 (a row is one partial quad), K up to 256
CRAFTED = [(3, (20, 24), (0, 0, 20, 24), (20, 24)), (18, (24, 32), (4, 8, 16, 20), (16, 20)), (5, (23, 30), (2, 3, 19, 21), (19, 21)),
           (2, (17, 19), (1, 2, 15, 13), (15, 13)), (4, (20, 28), (0, 0, 20, 28), (33, 47)), (18, (40, 36), (3, 5, 31, 22), (12, 9)),
           (3, (17, 30), (0, 0, 17, 30), (40, 13)), (7, (12, 18), (1, 1, 9, 14), (9, 31)), (256, (14, 16), (1, 0, 12, 16), (12, 16)),
           (256, (14, 15), (0, 1, 12, 13), (25, 18)), (6, (9, 9), (2, 2, 5, 5), (7, 3)), (2, (8, 8), (0, 0, 8, 8), (5, 1)),
           (9, (64, 80), (0, 0, 64, 80), (129, 160)), (33, (50, 70), (5, 6, 40, 60), (20, 30))]


@pytest.mark.parametrize('K,plane,rect,out', CRAFTED)
def test_kernel_on_crafted_planes_equals_the_statement(K, plane, rect, out):
    lg = _crafted(K, plane[0], plane[1], K * 1000 + out[0])
    with np.errstate(invalid='ignore'):
        want = export.labelmap_statement(lg, rect, out)
    got = labelmap_from_logits(lg, rect, out)
    assert got.dtype == np.uint8 and got.shape == tuple(out)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])
    if K <= 18 and out[0] * out[1] > 100:
        assert len(np.unique(got)) >= 2


def test_kernel_on_the_cases_by_name():
    """One pixel per case, identity and resampled alike where the case survives resampling: exact ties (first index), +0 against -0,
    subnormals, an infinite head, a NaN head (the first NaN wins whatever follows)."""
    cols = [[1.0, 2.0, 2.0, 2.0], [0.0, -0.0, 0.0, -0.0], [-0.0, 0.0, -0.0, 0.0], [_h(0x0001), _h(0x0002), _h(0x0002), 0.0],
            [_h(0x8001), -0.0, 0.0, _h(0x8002)], [5.0, np.inf, np.inf, 7.0], [-np.inf, -np.inf, -7.0, -np.inf],
            [1.0, np.nan, np.inf, np.nan], [np.nan, np.inf, 3.0, 4.0], [np.inf, -np.inf, _h(0xFE01), np.nan]]
    want = [1, 0, 0, 1, 1, 1, 2, 1, 0, 2]
    lg = np.array(cols, np.float32).T.astype(np.float16)[:, None, :].repeat(6, axis=1)          # [4 heads, 6 rows, 10 columns]
    got = labelmap_from_logits(lg, (0, 0, 6, 10), (6, 10))
    assert np.array_equal(got, export.labelmap_statement(lg, (0, 0, 6, 10), (6, 10))) and [int(v) for v in got[0]] == want
    for r in range(3):                                              # constant planes resample to themselves wherever no inf meets a zero weight
        col = lg[:, :, r:r + 1].repeat(8, axis=2)
        up = labelmap_from_logits(col, (0, 0, 6, 8), (11, 19))
        assert np.array_equal(up, export.labelmap_statement(col, (0, 0, 6, 8), (11, 19))) and (up == want[r]).all()


def test_bad_arguments_are_refused_by_name_and_nothing_is_written():
    lg = np.zeros((3, 8, 8), np.float16)
    for rect, out, word in [((0, 0, 9, 8), (4, 4), 'source rectangle 9x8 at (0,0) is empty or leaves the 8x8 image'),
                            ((2, 2, 7, 4), (4, 4), 'source rectangle'), ((0, 0, 8, 8), (0, 4), 'bad output extent 0x4')]:
        with pytest.raises(RuntimeError, match='ts2d_labelmap_from_logits') as ei:
            labelmap_from_logits(lg, rect, out)
        assert word in str(ei.value)
    assert labelmap_from_logits(lg, (0, 0, 8, 8), (4, 4)).shape == (4, 4)


# ------------------------------------------------------------------------------------------------ the engine entry
def _plan(data, patch=PATCH, step=0.5):
    """[C,H,W] -> the padded image, its tile list and the rectangle (y, x, h, w) of the case in it, as the predictor makes them."""
    padded, revert = sw.pad_nd_image(np.asarray(data, np.float32)[:, None], patch)
    tiles = [(y, x) for (_, y, x) in sw.tile_slicers(padded.shape[2:], patch, step, 1)]
    return np.ascontiguousarray(padded[:, 0]), tiles, (revert[2].start, revert[3].start) + tuple(data.shape[1:])


def _same16(a, b):
    return a.dtype == b.dtype == np.float16 and a.shape == b.shape and np.array_equal(a.view(np.uint16), b.view(np.uint16))


def _engines(n, arch=ARCH, seed0=170, precision='split', order='float', **kw):
    es = [Engine(arch, blob_for(arch, seed0 + f)[1], **kw) for f in range(n)]
    for e in es:
        e.set_precision(precision)
        e.set_tile_dtype(order)
    return es


def _close(es):
    for e in es:
        e.close()


# (input extent, export extent): up with an input narrower than the patch and extents that are no multiples of 4; identity; down; mixed; up on multiples of 4
GEOMETRIES = [((80, 52), (131, 87)), ((100, 130), (100, 130)), ((96, 72), (40, 45)), ((70, 90), (150, 50)), ((64, 64), (128, 192))]


@pytest.mark.parametrize('precision', ['split', 'f16'])
def test_engine_entry_equals_the_statement_of_its_own_logits(precision):
    g = sw.compute_gaussian(PATCH)
    plans = [_plan(prng.normal_f32(21, i, (ARCH.input_channels,) + hw)) for i, (hw, _) in enumerate(GEOMETRIES)]
    imgs, tiles, rects = ([p[j] for p in plans] for j in range(3))
    lms = [r + tuple(o) for r, (_, o) in zip(rects, GEOMETRIES)]
    es = _engines(1, precision=precision, order='half' if precision == 'f16' else 'float')
    try:
        e = es[0]
        for full, groups in ((False, [[i] for i in range(5)]), (True, [[0, 1, 2, 3, 4]])):
            for grp in groups:
                sub = lambda v: [v[i] for i in grp]                                        # noqa: E731
                labels, l16 = predict_tiled_labelmap_ensemble(es, sub(imgs), PATCH, sub(tiles), sub(lms), (0, 1), g, want_logits=True, full_batch=full)
                ref16 = e.predict_tiled_export(sub(imgs), PATCH, sub(tiles), [lms[i][:4] + lms[i][2:4] for i in grp], (0, 1), g, want_logits=True,
                                               full_batch=full)[2]
                for j, i in enumerate(grp):
                    assert _same16(l16[j], ref16[j])                       # the half logits of the existing entry of the same dispatch
                    want = export.labelmap_statement(l16[j], rects[i], GEOMETRIES[i][1])
                    assert labels[j].dtype == np.uint8 and labels[j].shape == tuple(GEOMETRIES[i][1])
                    assert np.array_equal(labels[j], want), (precision, full, i)
                    assert len(np.unique(labels[j])) >= 2
                assert e.last_tiled_inf is False and e.last_tiled_inf_per_image == [False] * len(grp)
        # the label maps alone (no half logits travel to the host): the same bytes
        only, none = predict_tiled_labelmap_ensemble(es, imgs, PATCH, tiles, lms, (0, 1), g)
        assert none is None and all(np.array_equal(a, b) for a, b in zip(only, labels))
    finally:
        _close(es)


def test_engine_entry_on_the_canonical_net():
    """One canonical sub-model with 18 heads on its 512 x 512 patch, 560 x 384 network extent -> 840 x 478 (no multiple of 4)."""
    arch = UNetArch.canonical(num_classes=18)
    blob = blob_for(arch, 1)[1]
    patch = (512, 512)
    img, tl, rect = _plan(prng.normal_f32(7, 1, (arch.input_channels, 560, 384)), patch, 0.5)
    with Engine(arch, blob) as e:
        for out in [(840, 478), (560, 384)]:
            labels, l16 = predict_tiled_labelmap_ensemble([e], [img], patch, [tl], [rect + out], (0, 1), sw.compute_gaussian(patch), want_logits=True,
                                                          full_batch=False)
            assert np.array_equal(labels[0], export.labelmap_statement(l16[0], rect, out)) and len(np.unique(labels[0])) >= 2


def test_full_batch_bytes_do_not_depend_on_the_batch():
    g = sw.compute_gaussian(PATCH)
    plans = [_plan(prng.normal_f32(22, i, (ARCH.input_channels,) + hw)) for i, hw in enumerate([(90, 70), (65, 67), (64, 128)])]
    imgs, tiles, rects = ([p[j] for p in plans] for j in range(3))
    lms = [rects[0] + (120, 61), rects[1] + rects[1][2:], rects[2] + (40, 50)]
    es = _engines(1)
    try:
        def run(idx):
            return predict_tiled_labelmap_ensemble(es, [imgs[i] for i in idx], PATCH, [tiles[i] for i in idx], [lms[i] for i in idx], (0, 1), g)[0]
        alone, abc, cab, ba = [run([i])[0] for i in range(3)], run([0, 1, 2]), run([2, 0, 1]), run([1, 0])
        for i in range(3):
            assert np.array_equal(alone[i], abc[i]) and np.array_equal(alone[i], cab[(i + 1) % 3])
        assert np.array_equal(ba[0], alone[1]) and np.array_equal(ba[1], alone[0])
        assert all(len(np.unique(a)) >= 2 for a in alone)
    finally:
        _close(es)


@pytest.mark.parametrize('F', [2, 3])
def test_an_ensemble_is_the_statement_of_the_mean_of_its_folds(F):
    g = sw.compute_gaussian(PATCH)
    plans = [_plan(prng.normal_f32(23, i, (ARCH.input_channels,) + hw)) for i, hw in enumerate([(90, 70), (64, 64), (50, 100)])]
    outs = [(120, 61), (64, 64), (77, 130)]
    imgs, tiles, rects = ([p[j] for p in plans] for j in range(3))
    lms = [r + o for r, o in zip(rects, outs)]
    es = _engines(F)
    try:
        for full in (True, False):          # (the size-dependent dispatch: one image per call, so that ensemble and folds run the same batch)
            labels, mean = [], []
            for grp in ([[0, 1, 2]] if full else [[0], [1], [2]]):
                out = predict_tiled_labelmap_ensemble(es, [imgs[i] for i in grp], PATCH, [tiles[i] for i in grp], [lms[i] for i in grp], (0, 1), g,
                                                      want_logits=True, full_batch=full)
                labels += out[0]
                mean += out[1]
            for i in range(3):
                folds = [predict_tiled_labelmap_ensemble([e], [imgs[i]], PATCH, [tiles[i]], [lms[i]], (0, 1), g, want_logits=True, full_batch=full)[1][0]
                         for e in es]
                assert not _same16(folds[0], folds[1])
                want16 = fold_mean_f16(folds)
                assert _same16(mean[i], want16), (F, full, i)
                assert np.array_equal(labels[i], export.labelmap_statement(want16, rects[i], outs[i])), (F, full, i)
                assert len(np.unique(labels[i])) >= 2
    finally:
        _close(es)


def test_bad_labelmaps_are_refused_by_name_before_any_device_work():
    import ctypes
    from totalsegmentator2d_amd import _lib
    es = _engines(2)
    try:
        img, tl, rect = _plan(prng.normal_f32(24, 0, (ARCH.input_channels, 80, 64)))
        for bad, word in [((4, 2, 0, 60, 50, 40), 'image 1: labelmap: source rectangle 0x60 at (4,2) is empty or leaves the 80x64 image'),
                          ((4, 2, 70, 60, 0, 40), 'image 1: labelmap: bad output extent 0x40'),
                          ((4, 2, 70, 60, 1 << 16, 1 << 15), 'image 1: labelmap: 65536x32768 exceeds 2^31 output elements')]:
            with pytest.raises(RuntimeError, match='ts2d_ensemble_predict_tiled_labelmap') as ei:
                _raw(es, img, tl, [rect + (50, 40), bad])
            assert word in str(ei.value), str(ei.value)
        desc, lmd = (_lib.TiledImage * 1)(), (_lib.TiledLabelmap * 1)()
        ty, tx = np.array([t[0] for t in tl], np.int32), np.array([t[1] for t in tl], np.int32)
        d = desc[0]
        d.image, d.Hp, d.Wp, d.n_tiles, d.tile_y, d.tile_x = img.ctypes.data, 80, 64, len(tl), ty.ctypes.data, tx.ctypes.data
        x = lmd[0]
        x.src_y, x.src_x, x.src_h, x.src_w, x.out_h, x.out_w, x.label_u8 = 0, 0, 80, 64, 50, 40, None
        handles = (ctypes.c_void_p * 2)(es[0]._h, es[1]._h)
        lib = es[0].lib
        assert lib.ts2d_ensemble_predict_tiled_labelmap(handles, 2, desc, lmd, 1, 64, 64, 3, None, 1) == -1
        assert _lib.last_error() == 'image 0: labelmap: the output is null'
        assert lib.ts2d_ensemble_predict_tiled_labelmap(handles, 2, desc, None, 1, 64, 64, 3, None, 1) == -1 and 'null pointer' in _lib.last_error()
        assert lib.ts2d_ensemble_predict_tiled_labelmap(handles, 2, None, None, 0, 64, 64, 3, None, 1) == 0          # nothing to do
        es[1].set_precision('f16')
        with pytest.raises(RuntimeError, match='fold 1 runs precision mode 2, fold 0 mode 1'):
            predict_tiled_labelmap_ensemble(es, [img], PATCH, [tl], [rect + (50, 40)], (0, 1), None)
    finally:
        _close(es)


def _raw(es, img, tl, lms):
    """The entry on descriptors whose label_u8 is a 16-byte dummy (the marshaller would allocate every extent it is asked for): for calls
    the library must refuse before it writes anything."""
    import ctypes
    from totalsegmentator2d_amd import _lib
    n = len(lms)
    desc, lmd = (_lib.TiledImage * n)(), (_lib.TiledLabelmap * n)()
    ty, tx = np.array([t[0] for t in tl], np.int32), np.array([t[1] for t in tl], np.int32)
    dummy = np.zeros(16, np.uint8)
    for i, lm in enumerate(lms):
        d, x = desc[i], lmd[i]
        d.image, d.Hp, d.Wp, d.n_tiles, d.tile_y, d.tile_x = img.ctypes.data, img.shape[1], img.shape[2], len(tl), ty.ctypes.data, tx.ctypes.data
        x.src_y, x.src_x, x.src_h, x.src_w, x.out_h, x.out_w = lm
        x.label_u8 = dummy.ctypes.data
    handles = (ctypes.c_void_p * len(es))(*[e._h for e in es])
    _lib.check(es[0].lib.ts2d_ensemble_predict_tiled_labelmap(handles, len(es), desc, lmd, n, 64, 64, 3, None, 1), 'ts2d_ensemble_predict_tiled_labelmap')
    assert not dummy.any()


# ------------------------------------------------------------------------------------------------ model folders through the surface
def _write_model_folder(root, group, arch, seeds, patch=PATCH):
    """A LABEL-MAP nnU-Net model folder as upstream writes it: Dataset###_x/nnUNetTrainer__nnUNetPlans__2d with dataset.json (no
    `multilabel`: one head per label, background at 0), plans.json and fold_N/checkpoint_final.pth."""
    import torch
    d = os.path.join(root, 'Dataset001_' + group, 'nnUNetTrainer__nnUNetPlans__2d')
    os.makedirs(d)
    labels = {'background': 0, **{f'{group}_{i}': i for i in range(1, arch.num_classes)}}
    with open(os.path.join(d, 'dataset.json'), 'w') as f:
        json.dump({'channel_names': {'0': 'mean', '1': 'max'}, 'labels': labels, 'file_ending': '.nrrd', 'numTraining': 1}, f)
    n = arch.n_stages
    kw = {'n_stages': n, 'features_per_stage': list(arch.features_per_stage), 'conv_op': 'torch.nn.modules.conv.Conv2d', 'kernel_sizes': [[3, 3]] * n,
          'strides': [[1, 1]] + [[2, 2]] * (n - 1), 'n_conv_per_stage': list(arch.n_conv_per_stage),
          'n_conv_per_stage_decoder': list(arch.n_conv_per_stage_decoder), 'conv_bias': True, 'norm_op': 'torch.nn.modules.instancenorm.InstanceNorm2d',
          'norm_op_kwargs': {'eps': 1e-05, 'affine': True}, 'dropout_op': None, 'dropout_op_kwargs': None, 'nonlin': 'torch.nn.LeakyReLU',
          'nonlin_kwargs': {'inplace': True}}
    plans = {'plans_name': 'nnUNetPlans', 'transpose_forward': [0, 1, 2], 'transpose_backward': [0, 1, 2],
             'configurations': {'2d': {'patch_size': list(patch), 'spacing': [1.5, 1.5], 'normalization_schemes': ['ZScoreNormalization'] * 2,
                                       'use_mask_for_norm': [False, False],
                                       'architecture': {'network_class_name': 'dynamic_network_architectures.architectures.unet.PlainConvUNet',
                                                        'arch_kwargs': kw, '_kw_requires_import': ['conv_op', 'norm_op', 'dropout_op', 'nonlin']}}}}
    with open(os.path.join(d, 'plans.json'), 'w') as f:
        json.dump(plans, f)
    for fold, seed in enumerate(seeds):
        sd = weights.synthetic_state_dict(arch, seed)
        os.makedirs(os.path.join(d, f'fold_{fold}'))
        torch.save({'network_weights': {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, 'inference_allowed_mirroring_axes': (0, 1),
                    'trainer_name': 'nnUNetTrainer', 'init_args': {'configuration': '2d', 'fold': fold}},
                   os.path.join(d, f'fold_{fold}', 'checkpoint_final.pth'))
    return labels


def _folder_model(root, group, K, seeds):
    arch = cases.unet(3, (32, 32, 64), K)
    sub = os.path.join(root, group)
    labels = _write_model_folder(sub, group, arch, seeds)
    m = HIPModel({'root': sub, 'model': f'ts2d-v2-ep4000b2_{group}', 'revision': 1, 'folds': tuple(range(len(seeds))),
                  'param': {'nnu.configuration': '2d'}})
    assert not m.multilabel and m.labels == {v: k for k, v in labels.items() if k != 'background'}
    return m


def _relabelled(name, spacing):
    img = nrrd.read(os.path.join(A, name))
    return nrrd.Image(img.array, tuple(float(v) for v in spacing), img.origin, img.direction, img.components, dict(img.meta), img.space)


def _same_image(a, b):
    return a.array.dtype == b.array.dtype == np.uint8 and a.array.shape == b.array.shape and np.array_equal(a.array, b.array) and a.meta == b.meta \
        and a.spacing == b.spacing and a.origin == b.origin and a.direction == b.direction and a.size == b.size


@pytest.mark.parametrize('folds', [1, 2])
def test_a_label_map_model_folder_through_apply_and_apply_batch_equals_the_host_route(tmp_path, folds, monkeypatch):
    """The reference's 2-D sample on the plan spacing and relabelled off it (up and down): the device route and ``device_labelmap = False``
    give byte-identical images and metadata, and the device route brings ONE plane per case from the predictor."""
    inputs = {'on': nrrd.read(os.path.join(A, 'sample_s0616.nrrd')), 'fine': _relabelled('sample_s0616.nrrd', (0.9, 1.2)),
              'coarse': _relabelled('sample_s0616.nrrd', (2.5, 2.0))}
    m = _folder_model(str(tmp_path), 'cardiac', 6, list(range(31, 31 + folds)))
    m.start()
    try:
        p = m._predictor
        assert len(p.engines) == folds and p.arch.num_classes == 6
        calls, planes = [], []
        orig = engine_module.predict_tiled_labelmap_ensemble          # the predictor looks it up at call time: calls INTO THE LIBRARY are counted
        monkeypatch.setattr(engine_module, 'predict_tiled_labelmap_ensemble',
                            lambda engines, images, *a, **kw: (calls.append((len(engines), len(images))), orig(engines, images, *a, **kw))[1])
        for name in ('predict_labelmap_from_preprocessed_data', 'predict_labelmap_from_preprocessed_data_batch'):
            fn = getattr(p, name)
            monkeypatch.setattr(p, name, lambda data, *a, _f=fn, _b=name.endswith('_batch'), **kw:
                                (lambda out: (planes.extend(out if _b else [out]), out)[1])(_f(data, *a, **kw)))
        m.device_labelmap = False
        host = {k: m.apply(v) for k, v in inputs.items()}
        host_many = m.apply_batch(dict(inputs))
        assert not calls and not planes
        m.device_labelmap = True
        dev = {}
        for k, v in inputs.items():
            dev[k] = m.apply(v)
            assert {'start', 'preprocessed', 'predicted', 'exported', 'done'} <= set(m.timestamps)
        assert calls == [(folds, 1)] * 3
        dev_many = m.apply_batch(dict(inputs))
        assert calls == [(folds, 1)] * 3 + [(folds, 3)]               # ONE engine call: every fold, resampled and un-resampled cases together
        assert len(planes) == 6
        for k, plane in zip(list(inputs) * 2, planes):                 # one uint8 plane per case, already in the case's own extent
            assert plane.dtype == np.uint8 and plane.shape == (1, 1) + inputs[k].array.shape[:2], (k, plane.shape)
        for k, img in inputs.items():
            assert _same_image(dev[k], host[k]) and _same_image(dev_many[k], host_many[k]), k
            assert dev[k].array.shape == img.array.shape[:2] and dev[k].spacing == img.spacing and dev[k].components == 1
            assert 2 <= len(np.unique(dev[k].array)) <= 6 and dev[k].array.max() < 6
    finally:
        m.stop()


def test_two_label_map_sub_models_merge_as_on_the_host_route(tmp_path):
    inputs = [nrrd.read(os.path.join(A, 'sample_s0616.nrrd')), _relabelled('sample_s0616.nrrd', (0.9, 1.2)),
              _relabelled('sample_s0521.nrrd', (0.8, 0.8, 2.0)), nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))]
    ids = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_ribs')
    import warnings
    models = {ids[0]: _folder_model(str(tmp_path), 'cardiac', 4, [41]), ids[1]: _folder_model(str(tmp_path), 'ribs', 6, [42])}
    seen = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                              # ("not configured for multilabel inference": the point of this test)
        ts = TS2D(models=models)
    with ts:
        orig = engine_module.predict_tiled_labelmap_ensemble
        engine_module.predict_tiled_labelmap_ensemble = lambda engines, images, *a, **kw: (seen.append(len(images)), orig(engines, images, *a, **kw))[1]
        try:
            for m in models.values():
                m.device_labelmap = False
            host = [ts.predict(i) for i in inputs]
            host_many = ts.predict_many(inputs)
            assert not seen
            for m in models.values():
                m.device_labelmap = True
            dev = [ts.predict(i) for i in inputs]
            assert seen == [1] * (len(inputs) * len(models))
            del seen[:]
            dev_many = ts.predict_many(inputs)
            assert seen == [len(inputs)] * len(models)               # ONE engine call per sub-model
        finally:
            engine_module.predict_tiled_labelmap_ensemble = orig
        for h, hm, d, dm in zip(host, host_many, dev, dev_many):
            for mid in [None] + list(ids):
                assert _same_image(d.get_segmentation(mid), h.get_segmentation(mid)), mid
                assert _same_image(dm.get_segmentation(mid), hm.get_segmentation(mid)), mid
            assert d.get_segmentation().array.any() and all(len(np.unique(d.get_segmentation(mid).array)) >= 2 for mid in ids)
