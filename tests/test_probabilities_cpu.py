"""``save_probabilities`` as far as it goes without a GPU: the export writes ``<ofile>.npz`` / ``<ofile>.pkl`` and fills around the crop
box as upstream does, the numpy statement of the device kernel (``export.probabilities_statement``) is the host route inside the box and
is held to the accuracy yardstick of tests/prob_util.py, and synthetic models of all three label conventions run end to end on the host
route, on the plan spacing and off it, with a segmentation that does not change by a byte when the probabilities are asked for."""
import ctypes
import os
import pickle
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import prob_util
from tests.batch_util import HostBatchModel
from tests.conftest import ROOT
from tests.surface_util import HostModel, synthetic_model
from totalsegmentator2d_amd import _lib, export, nrrd

DATASETS = prob_util.DATASETS
PROPS = {'shape_after_cropping_and_before_resampling': (1, 14, 10), 'shape_before_cropping': (1, 17, 15),
         'bbox_used_for_cropping': [(0, 1), (2, 16), (3, 13)]}


def _ref_image(hw):
    return nrrd.Image(np.zeros(hw + (2,), np.float32), (1.0, 1.0), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


# ------------------------------------------------------------------------------------------------ 1. the export
def test_the_export_writes_npz_and_pkl_in_the_pre_crop_shape(tmp_path):
    """The test that failed before the feature: the flag was accepted and ignored."""
    lg = (np.random.default_rng(3).standard_normal((2, 1, 9, 13)) * 2).astype(np.float16)
    ofile = str(tmp_path / 'case')
    ds = dict(DATASETS['multilabel'], labels={'background': 0, 'a': 1, 'b': 2})
    img = export.export_prediction_from_logits(lg, dict(PROPS), None, SimpleNamespace(transpose_backward=[0, 1, 2]), ds, ofile,
                                               save_probabilities=True, ref_image=_ref_image((17, 15)))
    assert sorted(os.listdir(tmp_path)) == ['case.npz', 'case.nrrd', 'case.pkl']
    prob = np.load(ofile + '.npz')['probabilities']
    assert prob.dtype == np.float32 and prob.shape == (2, 1, 17, 15) and np.array_equal(prob, img.probabilities)
    with open(ofile + '.pkl', 'rb') as f:
        assert pickle.load(f) == PROPS
    plain = export.export_prediction_from_logits(lg, dict(PROPS), None, SimpleNamespace(transpose_backward=[0, 1, 2]), ds, None,
                                                 ref_image=_ref_image((17, 15)))
    assert np.array_equal(plain.array, img.array) and plain.array.shape == (17, 15, 2) and not hasattr(plain, 'probabilities')
    assert np.array_equal(nrrd.read(ofile + '.nrrd').array, img.array)


@pytest.mark.parametrize('mode', export.PROBABILITY_MODES)
def test_the_fill_around_the_crop_box_and_the_statement_inside_it(mode):
    K = 3
    lg = (np.random.default_rng(5).standard_normal((K, 1, 9, 13)) * 2).astype(np.float16)
    seg, prob = export.convert_predicted_logits_to_segmentation_with_correct_shape(
        lg, PROPS, multilabel=mode == 'multilabel', regions=(1, 2, 3) if mode == 'regions' else None, return_probabilities=True)
    plain = export.convert_predicted_logits_to_segmentation_with_correct_shape(
        lg, PROPS, multilabel=mode == 'multilabel', regions=(1, 2, 3) if mode == 'regions' else None)
    assert np.array_equal(seg, plain) and prob.dtype == np.float32 and prob.shape == (K, 1, 17, 15)
    outside = np.ones((17, 15), bool)
    outside[2:16, 3:13] = False
    for k in range(K):
        assert (prob[k, 0][outside] == (1.0 if mode == 'labelmap' and k == 0 else 0.0)).all(), k
    want = export.probabilities_statement(lg[:, 0], (0, 0, 9, 13), (14, 10), (17, 15), (2, 3), mode)
    assert np.array_equal(prob[:, 0], want)
    inside = prob[:, 0, 2:16, 3:13]
    assert ((inside > 0) & (inside < 1)).all()
    if mode == 'labelmap':
        assert np.abs(inside.sum(0) - 1).max() < 1e-6 and np.array_equal(inside.argmax(0), seg[0, 2:16, 3:13])
    else:
        above = (inside > 0.5)
        decided = seg[:, 0, 2:16, 3:13] if mode == 'multilabel' else export.paint_regions(above, (1, 2, 3))
        assert np.array_equal(above.astype(np.uint8) if mode == 'multilabel' else seg[0, 2:16, 3:13], decided)
    with pytest.raises(ValueError, match='need the logits'):
        export.convert_predicted_logits_to_segmentation_with_correct_shape(seg[None] if seg.ndim == 3 else seg, PROPS, multilabel=mode == 'multilabel',
                                                                           return_probabilities=True)


def test_a_device_pair_passes_through_the_export_untouched():
    dec = np.random.default_rng(1).integers(0, 3, (1, 1, 17, 15)).astype(np.uint8)
    pr = np.random.default_rng(2).random((3, 1, 17, 15)).astype(np.float32)
    seg, prob = export.convert_predicted_logits_to_segmentation_with_correct_shape(dec, PROPS, multilabel=False, return_probabilities=True,
                                                                                   probabilities=pr)
    assert np.array_equal(seg, dec[0]) and np.array_equal(prob, pr)


def test_special_values_of_the_statement():
    h = np.array([0x7E00, 0x7C00, 0xFC00, 0x0000, 0x8000], np.uint16).view(np.float16)      # NaN, +inf, -inf, +0, -0
    lg = np.zeros((3, 1, 5), np.float16)
    lg[1, 0] = h
    sg = export.probabilities_statement(lg, (0, 0, 1, 5), (1, 5), (1, 5), (0, 0), 'multilabel')
    assert np.isnan(sg[1, 0, 0]) and sg[1, 0, 1:].tolist() == [1.0, 0.0, 0.5, 0.5] and (sg[[0, 2]] == 0.5).all()
    sm = export.probabilities_statement(lg, (0, 0, 1, 5), (1, 5), (1, 5), (0, 0), 'labelmap')
    assert np.isnan(sm[:, 0, :2]).all()                                 # a NaN or +inf head: every head of the pixel
    assert sm[:, 0, 2].tolist() == [0.5, 0.0, 0.5] and np.allclose(sm[:, 0, 3:], 1 / 3, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 2. the accuracy of the statement
def test_statement_sigmoid_on_all_halves_meets_the_yardstick():
    v = np.arange(65536, dtype=np.uint16).view(np.float16).reshape(1, 256, 256)
    p = export.probabilities_statement(v, (0, 0, 256, 256), (256, 256), (256, 256), (0, 0), 'multilabel')
    fig = prob_util.measure('statement sigmoid, all halves', p, v.astype(np.float32), False)
    assert fig['n'] == (65536 - 2046) - 9867            # every non-NaN half (the infinities included) but the 9 867 whose sigmoid is below 2^-126
    prob_util.assert_within(fig)
    ok = ~np.isnan(v)
    assert np.array_equal((p > 0.5)[ok], (v.astype(np.float32) > export.SIGMOID_HALF_THRESHOLD)[ok])      # the .npz never contradicts the .nrrd


@pytest.mark.parametrize('K', [2, 3, 18])
def test_statement_softmax_meets_the_yardstick(K):
    lg = (np.random.default_rng(K).standard_normal((K, 64, 64)) * 8).astype(np.float16)
    p = export.probabilities_statement(lg, (0, 0, 64, 64), (64, 64), (64, 64), (0, 0), 'labelmap')
    prob_util.assert_within(prob_util.measure(f'statement softmax K={K}', p, lg.astype(np.float32), True))
    assert np.array_equal(p.argmax(0), lg.astype(np.float32).argmax(0))


# ------------------------------------------------------------------------------------------------ 3. models on the host route
def _config(kind, seed=47):
    m0, _, _ = synthetic_model('ts2d-v2-ep4000b2_' + kind, 3, seed, network=True, feats=(32, 32))
    cfg = dict(m0._config)
    cfg['synthetic'] = dict(cfg['synthetic'], dataset_json=dict(DATASETS[kind]))
    cfg['param'] = dict(cfg['param'], **{'nnu.result.colors': None})
    return cfg


def _image(seed, hw, spacing, margin):
    """Noise with a margin of zeros in every channel: the crop box of the preprocessing is smaller than the image."""
    a = (np.random.default_rng(seed).standard_normal(hw + (2,)) * 300).astype(np.float32)
    keep = np.zeros(hw, bool)
    keep[margin[0]:hw[0] - margin[0], margin[1]:hw[1] - margin[1]] = True
    a[~keep] = 0
    return nrrd.Image(a, spacing, (3.0, -7.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


def _recording(base):
    class Recording(base):
        def _preprocess_input(self, img):
            out = super()._preprocess_input(img)
            self.props.append(out[2])
            return out

        def _predict(self, datas, *a, **kw):
            out = super()._predict(datas, *a, **kw)
            self.logits += out
            return out
    return Recording


@pytest.mark.parametrize('kind', export.PROBABILITY_MODES)
def test_models_of_every_convention_on_the_host_route(kind, tmp_path):
    """On the plan spacing and off it, ``apply`` through the double of tests/surface_util.py (its predictor has the probabilities method and
    answers None: no engines) and ``apply_batch`` through that of tests/batch_util.py (its ``_sliding_window_batch`` does not know the
    keyword): the host route computes the probabilities from the logits, and the segmentation is that of the call without the flag."""
    imgs = {'on': _image(1, (80, 70), (1.5, 1.5), (5, 7)), 'off': _image(2, (70, 90), (0.9, 1.2), (4, 6))}
    for base, batched in ((HostModel, False), (HostBatchModel, True)):
        m = _recording(base)(_config(kind))
        m.props, m.logits = [], []
        assert m.device_probabilities is True
        m.start()
        try:
            call = m.apply_batch if batched else (lambda d, *a, **kw: {k: m.apply({k: v}, *a, **kw)[k] for k, v in d.items()})
            plain = call(dict(imgs))
            n = len(m.logits)
            out = call(dict(imgs), save_probabilities=True)
            props, logits = m.props[-2:], m.logits[n:]
            files = call(dict(imgs), str(tmp_path / f'{kind}{int(batched)}'), save_probabilities=True) if not batched else None
        finally:
            m.stop()
        assert len(logits) == 2
        for (k, img), pr, lg in zip(imgs.items(), props, logits):
            assert np.array_equal(out[k].array, plain[k].array) and out[k].meta == plain[k].meta and not hasattr(plain[k], 'probabilities')
            lg = np.asarray(lg)
            assert lg.dtype == np.float16 and lg.shape[:2] == (3, 1)
            tgt, full = tuple(pr['shape_after_cropping_and_before_resampling'])[1:], tuple(pr['shape_before_cropping'])[1:]
            (y0, y1), (x0, x1) = pr['bbox_used_for_cropping'][1:]
            assert full == img.array.shape[:2] and (y1 - y0, x1 - x0) == tgt != full and (tgt != lg.shape[2:]) == (k == 'off')
            want = export.probabilities_statement(lg[:, 0], (0, 0) + lg.shape[2:], tgt, full, (y0, x0), kind)
            got = out[k].probabilities
            assert got.dtype == np.float32 and got.shape == (3, 1) + full and np.array_equal(got[:, 0], want)
            if files is not None:
                assert files[k].endswith(k + '.nrrd') and np.array_equal(nrrd.read(files[k]).array, plain[k].array)
                assert np.array_equal(np.load(files[k][:-5] + '.npz')['probabilities'], got)
                with open(files[k][:-5] + '.pkl', 'rb') as f:
                    assert tuple(pickle.load(f)['shape_before_cropping']) == (1,) + full


def test_override_false_skips_a_case_only_if_every_requested_file_exists(tmp_path):
    m = _recording(HostModel)(_config('labelmap'))
    m.props, m.logits = [], []
    m.start()
    try:
        img = _image(1, (80, 70), (1.5, 1.5), (5, 7))
        m.apply({'a': img}, str(tmp_path))
        assert len(m.logits) == 1 and sorted(os.listdir(tmp_path)) == ['a.nrrd']
        m.apply({'a': img}, str(tmp_path), override=False)
        assert len(m.logits) == 1                                       # skipped
        m.apply({'a': img}, str(tmp_path), override=False, save_probabilities=True)
        assert len(m.logits) == 2 and sorted(os.listdir(tmp_path)) == ['a.npz', 'a.nrrd', 'a.pkl']
        m.apply({'a': img}, str(tmp_path), override=False, save_probabilities=True)
        assert len(m.logits) == 2
    finally:
        m.stop()


# ------------------------------------------------------------------------------------------------ 4. the ABI
def test_the_new_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    for name in ('ts2d_ensemble_predict_tiled_probabilities', 'ts2d_probabilities_from_logits'):
        assert name in _lib.SYMBOLS and name in _lib.OPTIONAL and hasattr(lib, name), name
    assert lib.ts2d_abi_version() == _lib.ABI_VERSION == 9
    header = open(os.path.join(ROOT, 'include', 'ts2d_engine.h')).read()
    assert re.search(r'\}\s*ts2d_tiled_probabilities;', header)
    assert [int(v) for v in re.findall(r'#define TS2D_PROB_(?:MULTILABEL|LABELMAP|REGIONS) (\d)', header)] == [0, 1, 2]
    assert (_lib.PROB_MULTILABEL, _lib.PROB_LABELMAP, _lib.PROB_REGIONS) == (0, 1, 2) == tuple(range(len(export.PROBABILITY_MODES)))
    assert ctypes.sizeof(_lib.TiledProbabilities) == 10 * 4 + 2 * 8 and _lib.TiledProbabilities.prob_f32.offset == 40
