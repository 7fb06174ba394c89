"""The export's probabilities on the MI355X: the kernel sw_probabilities (csrc/kernels_prob.h) on crafted planes through
ts2d_probabilities_from_logits, the engine entry ts2d_ensemble_predict_tiled_probabilities under the predictor - one model, a fold
ensemble, a batch - and ``HIPModel.apply(save_probabilities=True)`` with the device route against the host route.  The decided maps are
compared byte for byte with the routes that existed; the probabilities with the yardstick of tests/prob_util.py (the reference's own
operators against float64; at most twice their error plus 1 ulp).  Every figure is printed before it is asserted (run with -s);
``scripts/gpu_probabilities_case.py --accuracy`` writes the table of them."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from tests import cases, prob_util
from totalsegmentator2d_amd import _lib, export, nrrd, prng, weights
from totalsegmentator2d_amd import engine as engine_module
from totalsegmentator2d_amd.engine import labelmap_from_logits, probabilities_from_logits, regions_from_logits
from totalsegmentator2d_amd.model import HIPModel
from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor

pytestmark = pytest.mark.gpu
THR = export.SIGMOID_HALF_THRESHOLD


def _h(bits):
    return np.array(bits, np.uint16).view(np.float16)


def _decided(lg, rect, out, mode, order):
    """The decided map of the routes that existed before the probabilities: the label-map and regions kernels, the threshold predicate."""
    if mode == 'labelmap':
        return labelmap_from_logits(lg, rect, out)
    if mode == 'regions':
        return regions_from_logits(lg, rect, out, order)
    return (prob_util.resampled(lg, rect, out) > THR).astype(np.uint8)


def _check(prob, dec, lg, rect, out, full, box, mode, order, name):
    """Everything one device result is held to: exact fill, the decided bytes, the accuracy of the probabilities inside the box."""
    K = lg.shape[0]
    (by, bx), (oh, ow) = box, out
    softmax = mode == 'labelmap'
    assert prob.dtype == np.float32 and prob.shape == (K,) + tuple(full) and dec.dtype == np.uint8
    outside = np.ones(full, bool)
    outside[by:by + oh, bx:bx + ow] = False
    for k in range(K):
        assert (prob[k][outside] == (1.0 if softmax and k == 0 else 0.0)).all(), (name, k)
    assert (dec[..., outside] == 0).all(), name
    want = _decided(lg, rect, out, mode, order)
    inside_dec = dec[..., by:by + oh, bx:bx + ow]
    assert np.array_equal(inside_dec, want), (name, np.argwhere(inside_dec != want)[:5])
    v = prob_util.resampled(lg, rect, out)
    inside = prob[:, by:by + oh, bx:bx + ow]
    fig = prob_util.measure(name, inside, v, softmax)
    prob_util.assert_within(fig)
    if softmax:
        # every pixel without NaN or +inf - and with a head above -inf: where EVERY head is -inf the maximum is -inf and -inf - -inf is NaN in
        # every head, in torch's softmax as here (measure() has just checked that the NaNs coincide with float64's)
        ok = ~(np.isnan(v) | (v == np.inf)).any(0) & (v > -np.inf).any(0)
        assert ok.any() and np.array_equal(np.take_along_axis(inside, inside_dec[None].astype(np.int64), 0)[0][ok], inside.max(0)[ok]), name
    return fig


# ------------------------------------------------------------------------------------------------ 1. the kernel on crafted planes
def test_sigmoid_on_all_65536_halves():
    v = np.arange(65536, dtype=np.uint16).view(np.float16).reshape(1, 256, 256)
    p, dec = probabilities_from_logits(v, (0, 0, 256, 256), (256, 256), (256, 256), (0, 0), 'multilabel')
    fig = prob_util.measure('device sigmoid, all halves', p, v.astype(np.float32), False)
    assert fig['n'] == (65536 - 2046) - 9867
    prob_util.assert_within(fig)
    ok = ~np.isnan(v)
    assert np.array_equal(np.isnan(p), ~ok)
    assert np.array_equal((p > 0.5)[ok], (v.astype(np.float32) > THR)[ok])           # the .npz never contradicts the .nrrd
    assert np.array_equal(dec, (v.astype(np.float32) > THR).astype(np.uint8))


SPECIAL = [0x0000, 0x8000, 0x7BFF, 0xFBFF, 0xFC00]          # +0, -0, 65504, -65504, -inf


def _crafted(K, seed):
    rng = np.random.default_rng(seed)
    lg = rng.uniform(-20, 20, (K, 13, 10)).astype(np.float16)
    flat = lg.reshape(-1)
    at = rng.choice(flat.size, size=max(len(SPECIAL), flat.size // 8), replace=False)
    flat[at] = _h([SPECIAL[i % len(SPECIAL)] for i in range(at.size)])
    lg[:, 4, 5] = lg[0, 4, 5]                               # a tie over every head
    if K > 1:
        lg[K - 1, 6, 6] = lg[0, 6, 6] = np.float16(19.5)    # a tie of the maximum between the first and the last head
    lg[K // 2, 8, 4] = np.inf                               # one pixel with +inf, one with NaN
    lg[0, 9, 7] = np.nan
    return lg


@pytest.mark.parametrize('K', [1, 2, 3, 18, 33, 256])
def test_kernel_on_crafted_planes(K):
    """(K = 33 and 256: the passes over the heads at the head counts of label-map models - tests/test_gpu_many_heads.py has the engine entry.)
    13 x 10 planes, the rectangle (1, 3, 11, 6) with an odd src_x (the unaligned read path); identity and 17 x 7 (a width that is no multiple
    of 4); in a 20 x 9 extent at (2, 1) (scalar stores, the fill on every side) and with the output as the whole extent."""
    rect = (1, 3, 11, 6)
    order = tuple(int(c) for c in np.random.default_rng(K).integers(0, 256, K))
    lg = _crafted(K, 100 + K)
    for out in ((11, 6), (17, 7)):
        for full, box in (((20, 9), (2, 1)), (out, (0, 0))):
            for mode in export.PROBABILITY_MODES:
                p, dec = probabilities_from_logits(lg, rect, out, full, box, mode, order if mode == 'regions' else None)
                _check(p, dec, lg, rect, out, full, box, mode, order, f'crafted K={K} {mode} out={out} full={full}')
                p2, none = probabilities_from_logits(lg, rect, out, full, box, mode, order if mode == 'regions' else None, want_decided=False)
                assert none is None and np.array_equal(p2.view(np.uint32), p.view(np.uint32))


def test_aligned_planes_take_the_vector_stores_and_more_than_one_block():
    """Full width 64 (float4 / 32-bit stores), 70 rows x 16 quads: more than four blocks of 256 lanes, the last one ending inside the block;
    an aligned identity rectangle and a resampled one."""
    lg = (np.random.default_rng(7).standard_normal((3, 40, 48)) * 4).astype(np.float16)
    for rect, out in (((4, 8, 30, 36), (30, 36)), ((4, 8, 30, 36), (61, 52))):
        for mode in export.PROBABILITY_MODES:
            p, dec = probabilities_from_logits(lg, rect, out, (70, 64), (5, 8), mode, (3, 1, 2) if mode == 'regions' else None)
            _check(p, dec, lg, rect, out, (70, 64), (5, 8), mode, (3, 1, 2), f'aligned {mode} out={out}')


# ------------------------------------------------------------------------------------------------ 2. the engine path under the predictor
ARCH = cases.unet(2, (32, 32), 3)
PATCH = (64, 64)
# (data extent, extent after resampling back, extent before cropping, origin of the crop box): on the plan spacing, and two off it
CASES = [((70, 90), (70, 90), (76, 96), (3, 4)), ((70, 90), (81, 100), (81, 100), (0, 0)), ((64, 66), (50, 75), (57, 80), (7, 5))]


def _predictor(mode, folds):
    p = HIPnnUNetPredictor()
    p.manual_initialization(ARCH, [weights.pack_blob(ARCH, weights.synthetic_state_dict(ARCH, 181 + f)) for f in range(folds)], PATCH,
                            dataset_json=dict(prob_util.DATASETS[mode]))
    return p


class _Calls:
    """Every call into the library's probabilities entry, with the half logits asked for in the SAME call."""
    def __init__(self, monkeypatch):
        self.seen = []
        orig = engine_module.predict_tiled_probabilities_ensemble

        def wrapped(engines, images, patch, tiles, rects, mode, *a, **kw):
            kw['want_logits'] = True
            probs, maps, logits = orig(engines, images, patch, tiles, rects, mode, *a, **kw)
            self.seen.append((len(engines), bool(kw.get('full_batch', True)), list(rects), mode, logits))
            return probs, maps, logits
        monkeypatch.setattr(engine_module, 'predict_tiled_probabilities_ensemble', wrapped)

    def pop(self):
        out = list(self.seen)
        del self.seen[:]
        return out


@pytest.mark.parametrize('folds', [1, 2])
@pytest.mark.parametrize('mode', export.PROBABILITY_MODES)
def test_engine_path_single_cases_and_a_batch(mode, folds, monkeypatch):
    p = _predictor(mode, folds)
    try:
        calls = _Calls(monkeypatch)
        order = p.regions_class_order
        assert (order is not None) == (mode == 'regions') and len(p.engines) == folds
        datas = [prng.normal_f32(31, i, (2, 1) + c[0]) for i, c in enumerate(CASES)]
        args = ([c[1] for c in CASES], [c[2] for c in CASES], [c[3] for c in CASES])
        dec0, prob0 = p.predict_probabilities_from_preprocessed_data(datas[2], *(a[2] for a in args))
        (F, full, rects, m, logits), = calls.pop()
        assert F == folds and not full and m == mode and rects[0][4:] == CASES[2][1] + CASES[2][2] + CASES[2][3]
        _check(prob0[:, 0], dec0[:, 0] if mode == 'multilabel' else dec0[0, 0], logits[0], rects[0][:4], CASES[2][1], CASES[2][2], CASES[2][3], mode, order,
               f'engine single {mode} F={folds}')
        batch = p.predict_probabilities_from_preprocessed_data_batch(datas, *args)
        (F, full, rects, m, logits), = calls.pop()
        assert F == folds and full and len(batch) == 3
        for i, (dec, prob) in enumerate(batch):
            assert prob.shape == (3, 1) + CASES[i][2] and dec.shape == ((3, 1) if mode == 'multilabel' else (1, 1)) + CASES[i][2]
            _check(prob[:, 0], dec[:, 0] if mode == 'multilabel' else dec[0, 0], logits[i], rects[i][:4], CASES[i][1], CASES[i][2], CASES[i][3], mode, order,
                   f'engine batch[{i}] {mode} F={folds}')
        # the determinism rule of the full-batch dispatch: a case's bytes do not depend on its batch-mates or its position
        back = p.predict_probabilities_from_preprocessed_data_batch(datas[::-1], *(a[::-1] for a in args))
        alone = p.predict_probabilities_from_preprocessed_data_batch(datas[1:2], *(a[1:2] for a in args))
        for i in range(3):
            assert np.array_equal(back[2 - i][0], batch[i][0]) and np.array_equal(back[2 - i][1].view(np.uint32), batch[i][1].view(np.uint32)), i
        assert np.array_equal(alone[0][0], batch[1][0]) and np.array_equal(alone[0][1].view(np.uint32), batch[1][1].view(np.uint32))
        # the decided maps of the routes that run without the probabilities
        sib = p.predict_segmentation_from_preprocessed_data_batch(datas, args[0]) if mode == 'multilabel' else p.predict_labelmap_from_preprocessed_data_batch(datas, args[0])
        for i, c in enumerate(CASES):
            (by, bx), (oh, ow) = c[3], c[1]
            assert np.array_equal(batch[i][0][..., by:by + oh, bx:bx + ow], sib[i]), i
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 3. HIPModel.apply end to end
def _image(seed, hw, spacing, margin):
    """Noise with a margin of zeros in every channel: the crop box of the preprocessing is smaller than the image."""
    a = (np.random.default_rng(seed).standard_normal(hw + (2,)) * 300).astype(np.float32)
    keep = np.zeros(hw, bool)
    keep[margin[0]:hw[0] - margin[0], margin[1]:hw[1] - margin[1]] = True
    a[~keep] = 0
    return nrrd.Image(a, spacing, (3.0, -7.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


@pytest.mark.parametrize('mode', export.PROBABILITY_MODES)
def test_model_apply_device_route_against_host_route(mode, monkeypatch, tmp_path):
    class Recording(HIPModel):
        def _preprocess_input(self, img):
            out = super()._preprocess_input(img)
            self.props.append(out[2])
            return out

        def _predict(self, datas, *a, **kw):
            out = super()._predict(datas, *a, **kw)
            self.logits += out
            return out
    m = Recording({'model': 'ts2d-v2-ep4000b2_' + mode, 'revision': 1, 'param': {},
                   'synthetic': {'arch': ARCH, 'blobs': [weights.pack_blob(ARCH, weights.synthetic_state_dict(ARCH, 181))], 'patch_size': PATCH,
                                 'dataset_json': dict(prob_util.DATASETS[mode])}})
    m.props, m.logits = [], []
    imgs = {'on': _image(1, (80, 70), (1.5, 1.5), (5, 7)), 'off': _image(2, (70, 90), (0.9, 1.2), (4, 6))}
    m.start()
    try:
        calls = _Calls(monkeypatch)
        plain = {k: m.apply({k: v})[k] for k, v in imgs.items()}
        assert not calls.pop()
        del m.logits[:]
        dev = {k: m.apply({k: v}, save_probabilities=True)[k] for k, v in imgs.items()}
        assert len(calls.pop()) == 2 and not m.logits                     # the device route: no logits travel
        batch = m.apply_batch(dict(imgs), str(tmp_path), save_probabilities=True)
        assert [(c[0], c[1], len(c[2])) for c in calls.pop()] == [(1, True, 2)]
        m.device_probabilities = False
        host = {k: m.apply({k: v}, save_probabilities=True)[k] for k, v in imgs.items()}
        assert not calls.pop() and len(m.logits) == 2
    finally:
        m.stop()
    assert sorted(os.listdir(tmp_path)) == ['off.npz', 'off.nrrd', 'off.pkl', 'on.npz', 'on.nrrd', 'on.pkl']
    for (k, img), props, lg in zip(imgs.items(), m.props[-2:], m.logits):
        assert np.array_equal(dev[k].array, plain[k].array) and np.array_equal(host[k].array, plain[k].array) and dev[k].meta == host[k].meta
        assert np.array_equal(nrrd.read(batch[k]).array, plain[k].array)
        saved = np.load(batch[k][:-5] + '.npz')['probabilities']
        with open(batch[k][:-5] + '.pkl', 'rb') as f:
            assert tuple(pickle.load(f)['shape_before_cropping']) == (1,) + img.array.shape[:2]
        lg = np.asarray(lg)[:, 0]
        tgt, full = tuple(props['shape_after_cropping_and_before_resampling'])[1:], tuple(props['shape_before_cropping'])[1:]
        (y0, y1), (x0, x1) = props['bbox_used_for_cropping'][1:]
        assert np.array_equal(host[k].probabilities[:, 0], export.probabilities_statement(lg, (0, 0) + lg.shape[1:], tgt, full, (y0, x0), mode))
        v = prob_util.resampled(lg, (0, 0) + lg.shape[1:], tgt)
        outside = np.ones(full, bool)
        outside[y0:y1, x0:x1] = False
        for name, got in (('apply', dev[k].probabilities), ('apply_batch', saved)):
            assert got.dtype == np.float32 and got.shape == (3, 1) + full
            assert np.array_equal(got[:, 0][:, outside], host[k].probabilities[:, 0][:, outside])
            prob_util.assert_within(prob_util.measure(f'model {mode} {k} {name}', got[:, 0, y0:y1, x0:x1], v, mode == 'labelmap'))


# ------------------------------------------------------------------------------------------------ 4. validation
def test_bad_calls_are_refused_by_name_and_nothing_is_written():
    lib = _lib.load()
    lg, rect = np.zeros((3, 8, 8), np.float16), (ctypes.c_int32 * 4)(0, 0, 8, 8)
    prob, dec, order = np.full((3, 6, 7), 7.0, np.float32), np.full((6, 7), 0xAB, np.uint8), np.array((1, 2, 3), np.uint8)
    fn, name = lib.ts2d_probabilities_from_logits, 'ts2d_probabilities_from_logits'

    def call(K=3, out=(5, 5), full=(6, 7), box=(1, 2), mode=1, order_=None, prob_=prob.ctypes.data, r=rect):
        return fn(0, lg.ctypes.data, K, 8, 8, ctypes.byref(r), out[0], out[1], full[0], full[1], box[0], box[1], mode, order_, prob_, dec.ctypes.data)
    for kw, msg in (({'prob_': None}, 'probabilities: the output is null'), ({'mode': 3}, 'probabilities: unknown mode 3'),
                    ({'mode': 2}, 'probabilities: the class order is null'), ({'box': (2, 2)}, 'probabilities: the 5x5 output at (2,2) leaves the full extent 6x7'),
                    ({'box': (-1, 0)}, 'probabilities: the 5x5 output at (-1,0) leaves the full extent 6x7'),
                    ({'full': (32768, 32768), 'K': 2}, 'probabilities: 2 x 32768x32768 exceeds 2^31 output elements'),
                    ({'K': 0}, 'probabilities: 0 heads outside 1 ... 256'), ({'K': 257, 'mode': 0}, 'probabilities: 257 heads outside 1 ... 256'), ({'out': (0, 5)}, 'bad output extent 0x5'),
                    ({'r': (ctypes.c_int32 * 4)(0, 4, 8, 8)}, 'source rectangle 8x8 at (0,4) is empty or leaves the 8x8 image')):
        assert call(**kw) == -1 and _lib.last_error() == f'{name}: {msg}', (kw, _lib.last_error())
    assert (prob == 7.0).all() and (dec == 0xAB).all()
    assert call(mode=2, order_=order.ctypes.data) == 0 and not (prob == 7.0).any() and not (dec == 0xAB).any()
    with pytest.raises(RuntimeError, match='mode must be one of'):
        probabilities_from_logits(lg, (0, 0, 8, 8), (5, 5), (6, 7), (1, 2), 'softmax')
    # the engine entry: the same refusals, the image named, before any device work
    from totalsegmentator2d_amd import sliding_window as sw
    from totalsegmentator2d_amd.engine import Engine
    img = np.ascontiguousarray(prng.normal_f32(30, 0, (2, 64, 80)))
    tl = [(y, x) for (_, y, x) in sw.tile_slicers((64, 80), PATCH, 0.5, 1)]
    ty, tx = np.array([t[0] for t in tl], np.int32), np.array([t[1] for t in tl], np.int32)
    prob, dec = np.full((3, 6, 7), 7.0, np.float32), np.full((6, 7), 0xAB, np.uint8)
    desc, pd = (_lib.TiledImage * 1)(), (_lib.TiledProbabilities * 1)()
    d, x = desc[0], pd[0]
    d.image, d.Hp, d.Wp, d.n_tiles, d.tile_y, d.tile_x = img.ctypes.data, 64, 80, len(tl), ty.ctypes.data, tx.ctypes.data
    x.src_y, x.src_x, x.src_h, x.src_w, x.out_h, x.out_w, x.full_h, x.full_w, x.box_y, x.box_x = 0, 0, 64, 80, 5, 5, 6, 7, 1, 2
    x.prob_f32, x.decided_u8 = prob.ctypes.data, dec.ctypes.data
    entry = 'ts2d_ensemble_predict_tiled_probabilities'
    with Engine(ARCH, weights.pack_blob(ARCH, weights.synthetic_state_dict(ARCH, 181))) as e:
        handles = (ctypes.c_void_p * 1)(e._h)
        call = lambda mode, o, n: getattr(e.lib, entry)(handles, 1, desc, pd, 1, 64, 64, 3, None, 1, mode, o, n)      # noqa: E731
        assert call(5, None, 0) == -1 and _lib.last_error() == f'{entry}: probabilities: unknown mode 5'
        assert call(2, None, 3) == -1 and _lib.last_error() == f'{entry}: probabilities: the class order is null'
        assert call(2, order.ctypes.data, 2) == -1 and _lib.last_error() == f'{entry}: probabilities: 2 class values for a model of 3 heads'
        x.prob_f32 = None
        assert call(1, None, 0) == -1 and _lib.last_error() == 'image 0: probabilities: the output is null'
        x.prob_f32 = prob.ctypes.data
        x.out_h = 0
        assert call(1, None, 0) == -1 and _lib.last_error() == 'image 0: probabilities: bad output extent 0x5'
        x.out_h, x.box_y = 5, 2
        assert call(1, None, 0) == -1 and _lib.last_error() == 'image 0: probabilities: the 5x5 output at (2,2) leaves the full extent 6x7'
        x.box_y, x.src_w = 1, 81
        assert call(0, None, 0) == -1 and _lib.last_error() == 'image 0: probabilities: source rectangle 64x81 at (0,0) is empty or leaves the 64x80 image'
        x.src_w = 80
        assert (prob == 7.0).all() and (dec == 0xAB).all() and d.inf_flag == 0
        assert call(1, None, 0) == 0 and not (prob == 7.0).any() and not (dec == 0xAB).any()
        assert np.abs(prob[:, 1:, 2:].sum(0) - 1).max() < 1e-6 and (prob[0, 0] == 1).all() and (prob[1:, :, :2] == 0).all()
