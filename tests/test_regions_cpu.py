"""REGION-BASED nnU-Net models (label values are lists, one head per foreground region, ``regions_class_order``) as far as they go
without a GPU: the label convention read from ``dataset.json``, the numpy statement of the device export pinned from outside (scipy's
zoom, torch's sigmoid, the painting loop spelled out), its special values, and a synthetic region model end to end on the host route."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from tests.batch_util import HostBatchModel
from tests.surface_util import HostModel, synthetic_model
from totalsegmentator2d_amd import export, nrrd
from totalsegmentator2d_amd.image import get_annotation_labels
from totalsegmentator2d_amd.labels import label_convention

BRATS = {'channel_names': {'0': 'mean', '1': 'max'}, 'file_ending': '.nrrd',
         'labels': {'background': 0, 'whole': [1, 2, 3], 'core': [2, 3], 'enh': [3]}, 'regions_class_order': [1, 2, 3]}


# ------------------------------------------------------------------------------------------------ 1. label conventions
def test_a_brats_like_dataset_is_a_region_model_of_three_heads():
    c = label_convention(BRATS)
    assert c.kind == 'regions' and c.n_heads == 3 and c.class_order == (1, 2, 3) and c.names == {1: 'whole', 2: 'core', 3: 'enh'}


def test_ignore_and_a_background_list_are_no_regions():
    ds = dict(BRATS, labels={'background': [0], 'whole': [1, 2, 3], 'core': (2, 3), 'ignore': 4, 'enh': 3}, regions_class_order=[5, 0, 5])
    c = label_convention(ds)
    assert c.kind == 'regions' and c.n_heads == 3 and c.class_order == (5, 0, 5)
    assert c.names == {5: 'enh'}                     # a repeated class value carries its last painter's name; 0 is background


def test_bad_region_datasets_are_refused_with_the_reason():
    no_order = {k: v for k, v in BRATS.items() if k != 'regions_class_order'}
    with pytest.raises(ValueError, match='no regions_class_order'):
        label_convention(no_order)
    with pytest.raises(ValueError, match=r'regions_class_order has 2 entries for 3 foreground regions \(whole, core, enh\)'):
        label_convention(dict(BRATS, regions_class_order=[1, 2]))
    with pytest.raises(ValueError, match=r'class value 300, outside 0\.\.255: the segmentation is one uint8 plane'):
        label_convention(dict(BRATS, regions_class_order=[1, 300, 3]))


def test_integer_and_multilabel_datasets_come_out_as_before():
    labels = {'background': 0, 'a': 1, 'b': 2, 'c': 3}
    lm = label_convention({'labels': labels})
    assert (lm.kind, lm.n_heads, lm.class_order, lm.names) == ('labelmap', 4, None, {1: 'a', 2: 'b', 3: 'c'})
    for flag in ('multilabel', 'multiclass'):
        ml = label_convention({'labels': labels, flag: True})
        assert (ml.kind, ml.n_heads, ml.class_order, ml.names) == ('multilabel', 3, None, {1: 'a', 2: 'b', 3: 'c'})
    m, _, _ = synthetic_model('ts2d-v2-ep4000b2_cardiac', 3, 31)
    assert m.multilabel and m.labels == {1: 'cardiac_1', 2: 'cardiac_2', 3: 'cardiac_3'}


# ------------------------------------------------------------------------------------------------ 2. the statement, pinned from outside
def _direct(case_f16, out_hw, order):
    """The export of a region model spelled out with nothing of this package: scipy's order-1 zoom per plane where the extent differs,
    torch's float32 sigmoid, > 0.5, the painting loop."""
    lg = case_f16.astype(np.float32)
    if tuple(out_hw) != lg.shape[1:]:
        lg = np.stack([ndi.zoom(pl, [o / i for o, i in zip(out_hw, pl.shape)], order=1, mode='nearest', grid_mode=True) for pl in lg])
        assert lg.dtype == np.float32 and lg.shape[1:] == tuple(out_hw)
    prob = torch.sigmoid(torch.from_numpy(lg)).numpy()
    seg = np.zeros(lg.shape[1:], np.uint8)
    for i, c in enumerate(order):
        seg[prob[i] > 0.5] = c
    return seg


@pytest.mark.parametrize('out', [(9, 13), (14, 10), (5, 7)])
@pytest.mark.parametrize('K,order', [(3, (1, 2, 3)), (5, (4, 0, 9, 4, 200))])
def test_statement_equals_zoom_sigmoid_and_the_painting_loop(K, order, out):
    rng = np.random.default_rng(K * 100 + out[0])
    padded = (rng.standard_normal((K, 12, 18)) * 2).astype(np.float16)
    padded[:, ::3, ::4] *= np.float16(1e-3)                           # values near the threshold as well
    rect = (2, 3, 9, 13)
    got = export.regions_statement(padded, rect, out, order)
    assert got.dtype == np.uint8 and got.shape == out
    assert np.array_equal(got, _direct(padded[:, 2:11, 3:16], out, order))
    assert set(np.unique(got).tolist()) <= {0, *order} and len(np.unique(got)) >= 3


# ------------------------------------------------------------------------------------------------ 3. special values
ORDER4 = (2, 0, 2, 7)
SPECIAL = [(0x0001, False), (0x0002, True), (0x8000, False), (0x7C00, True), (0xFC00, False), (0x7E00, False)]      # 2^-24, 2^-23, -0, +inf, -inf, NaN


def _h(bits):
    return np.array(bits, np.uint16).view(np.float16)


def test_special_values_on_every_head_in_turn():
    for k in range(4):
        lg = np.full((4, 1, len(SPECIAL)), -1.0, np.float16)
        lg[k, 0] = _h([b for b, _ in SPECIAL])
        got = export.regions_statement(lg, (0, 0, 1, len(SPECIAL)), (1, len(SPECIAL)), ORDER4)
        assert got[0].tolist() == [ORDER4[k] if painted else 0 for _, painted in SPECIAL], k
        assert np.array_equal(got, _direct(lg, (1, len(SPECIAL)), ORDER4))


def test_a_later_head_overrides_an_earlier_one_whatever_its_class():
    on, off = 1.0, -1.0
    cols = [[on, on, on, on], [on, on, off, off], [on, off, on, off], [off, on, off, off], [on, off, off, off], [off, off, off, off]]
    lg = np.array(cols, np.float16).T[:, None, :]                     # [4 heads, 1 row, 6 columns]
    got = export.regions_statement(lg, (0, 0, 1, 6), (1, 6), ORDER4)
    assert got[0].tolist() == [7, 0, 2, 0, 2, 0]                      # class 0 paints over 2; the repeated 2 comes from head 0 or head 2
    with pytest.raises(ValueError, match='3 entries, the prediction 4 heads'):
        export.regions_statement(lg, (0, 0, 1, 6), (1, 6), (1, 2, 3))


def test_resampled_infinities_meet_zero_weights_and_are_not_painted():
    lg = np.full((1, 4, 4), -1.0, np.float16)
    lg[0, 1, 1] = np.inf
    same = export.regions_statement(lg, (0, 0, 4, 4), (4, 4), (9,))
    assert same[1, 1] == 9 and same.sum() == 9                        # identity: the infinite logit stays infinite
    up = export.regions_statement(lg, (0, 0, 4, 4), (8, 8), (9,))
    assert np.array_equal(up, _direct(lg, (8, 8), (9,))) and (up == 9).any()


def test_the_export_paints_on_the_host_and_takes_a_decided_plane_unchanged():
    rng = np.random.default_rng(5)
    props = {'shape_after_cropping_and_before_resampling': (1, 14, 10), 'shape_before_cropping': (1, 17, 15),
             'bbox_used_for_cropping': [(0, 1), (2, 16), (3, 13)]}
    lg = (rng.standard_normal((3, 1, 9, 13)) * 2).astype(np.float16)
    seg = export.convert_predicted_logits_to_segmentation_with_correct_shape(lg, props, multilabel=False, regions=(1, 2, 3))
    want = np.zeros((1, 17, 15), np.uint8)
    want[0, 2:16, 3:13] = export.regions_statement(lg[:, 0], (0, 0, 9, 13), (14, 10), (1, 2, 3))
    assert seg.dtype == np.uint8 and np.array_equal(seg, want) and len(np.unique(seg)) == 4
    plane = want[:, 2:16, 3:13][None]                                 # uint8 [1, 1, 14, 10]: decided on the device
    assert np.array_equal(export.convert_predicted_logits_to_segmentation_with_correct_shape(plane, props, multilabel=False, regions=(1, 2, 3)), want)


# ------------------------------------------------------------------------------------------------ 4. end to end on the host route
def _region_config(seed=47):
    m0, _, _ = synthetic_model('ts2d-v2-ep4000b2_tumour', 3, seed, network=True, feats=(32, 32))
    cfg = dict(m0._config)
    cfg['synthetic'] = dict(cfg['synthetic'], dataset_json=dict(BRATS))
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
        """The model with the properties of every preprocessed case and the logits its predictor returned on record."""
        def _preprocess_input(self, img):
            out = super()._preprocess_input(img)
            self.props.append(out[2])
            return out

        def _predict(self, datas, *a, **kw):
            out = super()._predict(datas, *a, **kw)
            self.logits += out
            return out
    return Recording


def _check(img, seg, props, logits):
    order = tuple(BRATS['regions_class_order'])
    assert seg.components == 1 and seg.array.dtype == np.uint8 and seg.array.shape == img.array.shape[:2]
    assert set(np.unique(seg.array).tolist()) <= {0, *order} and len(np.unique(seg.array)) >= 2
    lg = np.asarray(logits)
    assert lg.dtype == np.float16 and lg.shape[:2] == (3, 1)
    tgt = tuple(props['shape_after_cropping_and_before_resampling'])[1:]
    want = np.zeros(tuple(props['shape_before_cropping'])[1:], np.uint8)
    (y0, y1), (x0, x1) = props['bbox_used_for_cropping'][1:]
    assert (y1 - y0, x1 - x0) == tgt and tgt != want.shape                                   # a real crop box
    want[y0:y1, x0:x1] = export.regions_statement(lg[:, 0], (0, 0) + lg.shape[2:], tgt, order)
    assert np.array_equal(seg.array, want)
    names = {v: k for k, v in {1: 'whole', 2: 'core', 3: 'enh'}.items()}
    found = get_annotation_labels(seg)
    assert found and {k: v['value'] for k, v in found.items()} == {n: names[n] for n in found}
    assert set(names[n] for n in found) == set(np.unique(seg.array).tolist()) - {0}


def test_a_region_model_end_to_end_on_the_host_route():
    """On the plan spacing and off it (the logits are resampled back on the host), through ``apply`` of the host double of
    tests/surface_util.py and through ``apply`` and ``apply_batch`` of tests/batch_util.py's (the double of surface_util has no batch
    path without engines; batch_util's is built on it and does not know the ``regions`` keyword: the host route untouched).  Before
    region models existed this failed at ``HIPModel(...)``: ``int()`` of a list."""
    imgs = {'on': _image(1, (80, 70), (1.5, 1.5), (5, 7)), 'off': _image(2, (70, 90), (0.9, 1.2), (4, 6))}
    for base, batched in ((HostModel, False), (HostBatchModel, False), (HostBatchModel, True)):
        m = _recording(base)(_region_config())
        m.props, m.logits = [], []
        assert not m.multilabel and m.labels == {1: 'whole', 2: 'core', 3: 'enh'} and m.device_regions is True
        m.start()
        try:
            assert m._predictor.regions_class_order == (1, 2, 3) and m._predictor.arch.num_classes == 3
            out = m.apply_batch(dict(imgs)) if batched else {k: m.apply(v) for k, v in imgs.items()}
        finally:
            m.stop()
        assert len(m.props) == len(m.logits) == 2
        for (k, img), props, lg in zip(imgs.items(), m.props, m.logits):
            _check(img, out[k], props, lg)
