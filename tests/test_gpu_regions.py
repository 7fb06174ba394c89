"""The device export of a REGION-BASED model on the MI355X: the kernel sw_regions (csrc/kernels_regions.h) on crafted planes through
ts2d_regions_from_logits, and the engine entry ts2d_ensemble_predict_tiled_regions under the product surface - one model, a fold
ensemble and a batch - against the numpy statement ``export.regions_statement`` of the half logits the same call returns and against
the model's own host route (``device_regions = False``).  Every comparison is exact: both routes decide on the same float32 values."""
import ctypes

import numpy as np
import pytest

from tests import cases
from totalsegmentator2d_amd import _lib, export, nrrd, prng, weights
from totalsegmentator2d_amd import engine as engine_module
from totalsegmentator2d_amd import sliding_window as sw
from totalsegmentator2d_amd.engine import Engine, regions_from_logits
from totalsegmentator2d_amd.model import HIPModel

pytestmark = pytest.mark.gpu


def _h(bits):
    return np.array(bits, np.uint16).view(np.float16)


# ------------------------------------------------------------------------------------------------ 1. the kernel on crafted planes
SPECIAL = [0x0001, 0x0002, 0x8000, 0x7C00, 0xFC00, 0x7E00]          # 2^-24 (not painted), 2^-23 (painted), -0, +inf, -inf, NaN
# (plane extent, rectangles): 9 x 13 - a row pitch that is no multiple of 4: the scalar read path, the second rectangle off the origin;
# 9 x 16 with an aligned rectangle: the 8-byte vector read path
PLANES = [((9, 13), [(0, 0, 9, 13), (1, 3, 7, 9)]), ((9, 16), [(0, 4, 8, 8)])]
# identity (None); widths that are no multiple of 4 (per-byte stores, the clamped last quad) up and down; a 32-bit store; 520 quads:
# more than one block of 256 lanes, the last one ending inside the block
OUTS = [None, (14, 10), (5, 7), (8, 12), (40, 52)]


def _crafted(K, hw, seed):
    rng = np.random.default_rng(seed)
    lg = (rng.standard_normal((K,) + hw) * 2).astype(np.float16)
    flat = lg.reshape(-1)
    at = rng.choice(flat.size, size=max(len(SPECIAL), flat.size // 6), replace=False)
    flat[at] = _h([SPECIAL[i % len(SPECIAL)] for i in range(at.size)])
    return lg


@pytest.mark.parametrize('K', [1, 3, 256])
def test_kernel_on_crafted_planes_equals_the_statement(K):
    order = {1: (5,), 3: (2, 0, 7)}.get(K) or tuple(int(v) for v in np.random.default_rng(K).integers(0, 256, K))
    painted = 0
    for hw, rects in PLANES:
        lg = _crafted(K, hw, K * 10 + hw[1])
        for rect in rects:
            for out in OUTS:
                out = out or rect[2:]
                want = export.regions_statement(lg, rect, out, order)
                got = regions_from_logits(lg, rect, out, order)
                assert got.dtype == np.uint8 and got.shape == tuple(out)
                assert np.array_equal(got, want), (K, hw, rect, out, np.argwhere(got != want)[:5])
                painted += int((want != 0).sum())
    assert painted > 0


def test_special_values_by_name_on_every_head():
    order = (2, 0, 2, 7)
    want_painted = [False, True, False, True, False, False]
    for k in range(4):
        lg = np.full((4, 2, len(SPECIAL)), -1.0, np.float16)
        lg[k] = _h(SPECIAL)
        got = regions_from_logits(lg, (0, 0, 2, 6), (2, 6), order)
        assert got[0].tolist() == got[1].tolist() == [order[k] if p else 0 for p in want_painted], k
    lg = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, 1, -1], [-1, 1, -1, -1]], np.float16).T[:, None, :].repeat(3, axis=1)
    got = regions_from_logits(lg, (0, 0, 3, 4), (3, 4), order)
    assert got[0].tolist() == [7, 0, 2, 0]                            # a later head overrides, class 0 included; 2 repeats


# ------------------------------------------------------------------------------------------------ 2. end to end
ARCH = cases.unet(2, (32, 32), 3)
PATCH = (32, 32)
ORDER = (1, 2, 3)
DATASET = {'channel_names': {'0': 'mean', '1': 'max'}, 'file_ending': '.nrrd',
           'labels': {'background': 0, 'whole': [1, 2, 3], 'core': [2, 3], 'enh': [3]}, 'regions_class_order': list(ORDER)}
# Synthetic weights put a head's logits on one side of the threshold more often than not, so each head's bias is minus the median of
# its logits (3 decimals), taken once with the torch oracle on the CPU: seeds 181 / 182 of weights.synthetic_state_dict, sliding window
# over prng.normal_f32(29, i, (2, 1, h, w)) for (h, w) = (40, 52), (33, 47), (64, 36).  With these biases the test's own cases, run on the
# CPU through the host double of the predictor, give these shares of (background, 1, 2, 3) in the statement's output: fold 0 alone
# 0.094-0.124, 0.091-0.113, 0.280-0.302, 0.493-0.505; the mean of the two folds 0.125-0.187, 0.093-0.113, 0.232-0.259, 0.482-0.503 -
# every class far above the 1 % that _assert_statement asks for.
HEAD_BIAS = {181: (-0.594, 0.862, 0.144), 182: (-0.223, -0.007, -0.224)}
HEAD_KEY = f'decoder.seg_layers.{ARCH.n_stages - 2}.bias'


def state_dict(seed):
    sd = dict(weights.synthetic_state_dict(ARCH, seed))
    sd[HEAD_KEY] = np.array(HEAD_BIAS[seed], np.float32)
    return sd


def _spaced(i, hw, net):
    """Case `i`: an image of extent `hw` whose spacing makes the plan's 1.5 mm grid `net` points wide ((h, w); equal: on the plan spacing)."""
    a = prng.normal_f32(29, i, hw + (2,))
    sy, sx = (1.5 * n / e for n, e in zip(net, hw))
    return nrrd.Image(a, (sx, sy), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


def inputs():
    """name -> (image, extent of the preprocessed data): on the plan spacing; off it, the export resamples 40 x 52 -> 57 x 44; the other
    extents of the batch, one of them lower than the patch (padded: its rectangle starts off the origin)."""
    return {'on': (_spaced(0, (40, 52), (40, 52)), (40, 52)), 'off': (_spaced(1, (57, 44), (40, 52)), (40, 52)),
            'small': (_spaced(2, (30, 47), (30, 47)), (30, 47)), 'wide': (_spaced(3, (30, 70), (64, 36)), (64, 36))}


def _model(folds):
    m = HIPModel({'model': 'ts2d-v2-ep4000b2_tumour', 'revision': 1, 'param': {},
                  'synthetic': {'arch': ARCH, 'blobs': [weights.pack_blob(ARCH, state_dict(181 + f)) for f in range(folds)], 'patch_size': PATCH,
                                'dataset_json': dict(DATASET)}})
    assert not m.multilabel and m.labels == {1: 'whole', 2: 'core', 3: 'enh'} and m.device_regions
    return m


class _Calls:
    """Every call into the library's region entry, with the half logits asked for in the SAME call (the predictor looks the function up
    at call time): (folds, full_batch, rects, labels, logits)."""
    def __init__(self, monkeypatch):
        self.seen = []
        orig = engine_module.predict_tiled_regions_ensemble

        def wrapped(engines, images, patch, tiles, rects, class_order, *a, **kw):
            kw['want_logits'] = True
            labels, logits = orig(engines, images, patch, tiles, rects, class_order, *a, **kw)
            assert tuple(class_order) == ORDER
            self.seen.append((len(engines), bool(kw.get('full_batch', True)), list(rects), labels, logits))
            return labels, logits
        monkeypatch.setattr(engine_module, 'predict_tiled_regions_ensemble', wrapped)

    def pop(self):
        out = list(self.seen)
        del self.seen[:]
        return out


def _assert_statement(label, logits16, rect6):
    """The device's plane is the statement of the half logits of its own call; the statement's output has every class (and background)
    on at least 1 % of its pixels - the input condition, asserted on the statement."""
    want = export.regions_statement(logits16, rect6[:4], rect6[4:], ORDER)
    shares = [float((want == c).mean()) for c in (0,) + ORDER]
    assert min(shares) >= 0.01, shares
    assert label.dtype == np.uint8 and np.array_equal(label, want), np.argwhere(label != want)[:5]


@pytest.mark.parametrize('folds', [1, 2])
def test_single_cases_equal_the_statement_of_their_own_logits_and_the_host_route(folds, monkeypatch):
    """One model (F = 1) and an ensemble of two folds; out_shape None (identity route) and (57, 44) (resampling route); input 2 x 1 x 40 x 52
    under a 32 x 32 patch: several overlapping tiles, mirrored on both axes."""
    cases_ = inputs()
    m = _model(folds)
    m.start()
    try:
        p = m._predictor
        assert len(p.engines) == folds and p.regions_class_order == ORDER and p.allowed_mirroring_axes == (0, 1)
        calls = _Calls(monkeypatch)
        for name, out_shape in (('on', None), ('off', (57, 44))):
            img, net = cases_[name]
            _, data, props = m._preprocess_input(img)
            assert tuple(np.shape(data)) == (2, 1) + net == (2, 1, 40, 52)
            plane = p.predict_labelmap_from_preprocessed_data(data, out_shape)
            (F, full, rects, labels, logits), = calls.pop()
            assert F == folds and not full and logits[0].shape == (3, 40, 52) and rects[0][4:] == (out_shape or net)
            assert plane.shape == (1, 1) + (out_shape or net) and np.array_equal(plane[0, 0], labels[0])
            _assert_statement(labels[0], logits[0], rects[0])
            dev = m.apply(img)
            assert len(calls.pop()) == 1
            m.device_regions = False
            host = m.apply(img)
            m.device_regions = True
            assert not calls.pop()                                    # the host route: logits to the host, painted there
            assert host.array.dtype == np.uint8 and host.array.shape == img.array.shape[:2] and host.components == 1
            assert np.array_equal(dev.array, host.array) and dev.meta == host.meta and np.array_equal(plane[0, 0], host.array)
    finally:
        m.stop()


def test_a_batch_equals_the_statement_the_host_route_and_a_batch_of_one(monkeypatch):
    """Three inputs of different extents in ONE engine call, out_shapes mixing None and real extents; every case's bytes equal those of
    a batch of one under the same full-batch dispatch (the determinism rule)."""
    cases_ = inputs()
    names = ['small', 'off', 'wide']
    m = _model(1)
    m.start()
    try:
        p = m._predictor
        calls = _Calls(monkeypatch)
        pre = [m._preprocess_input(cases_[n][0]) for n in names]
        datas = [d for _, d, _ in pre]
        assert [tuple(np.shape(d))[2:] for d in datas] == [cases_[n][1] for n in names]
        out_shapes = [None, (1, 57, 44), (30, 70)]
        planes = p.predict_labelmap_from_preprocessed_data_batch(datas, out_shapes)
        (F, full, rects, labels, logits), = calls.pop()
        assert F == 1 and full and len(labels) == 3
        for i, n in enumerate(names):
            assert planes[i].shape == (1, 1) + cases_[n][0].array.shape[:2] and np.array_equal(planes[i][0, 0], labels[i])
            _assert_statement(labels[i], logits[i], rects[i])
            alone = p.predict_labelmap_from_preprocessed_data_batch([datas[i]], [out_shapes[i]])
            assert np.array_equal(alone[0], planes[i]), n
        assert all(c[1] for c in calls.pop())
        imgs = {n: cases_[n][0] for n in names}
        dev = m.apply_batch(dict(imgs))
        assert [(c[0], c[1], len(c[3])) for c in calls.pop()] == [(1, True, 3)]
        m.device_regions = False
        host = m.apply_batch(dict(imgs))
        assert not calls.pop()
        for i, n in enumerate(names):
            assert np.array_equal(dev[n].array, host[n].array) and dev[n].meta == host[n].meta and np.array_equal(planes[i][0, 0], host[n].array)
    finally:
        m.stop()


# ------------------------------------------------------------------------------------------------ 4. validation
def test_bad_region_calls_are_refused_by_name_and_nothing_is_written():
    lib = _lib.load()
    lg, rect = np.zeros((3, 8, 8), np.float16), (ctypes.c_int32 * 4)(0, 0, 8, 8)
    out, order = np.full((5, 5), 0xAB, np.uint8), np.array(ORDER, np.uint8)
    args = (0, lg.ctypes.data, 3, 8, 8, ctypes.byref(rect), 5, 5)
    assert lib.ts2d_regions_from_logits(*args, None, out.ctypes.data) == -1
    assert _lib.last_error() == 'ts2d_regions_from_logits: regions: the class order is null'
    assert lib.ts2d_regions_from_logits(*args, order.ctypes.data, None) == -1
    assert _lib.last_error() == 'ts2d_regions_from_logits: regions: the output is null'
    with pytest.raises(RuntimeError, match='2 class values for 3 heads'):
        regions_from_logits(lg, (0, 0, 8, 8), (5, 5), (1, 2))
    with pytest.raises(RuntimeError, match='outside 0..255'):
        regions_from_logits(lg, (0, 0, 8, 8), (5, 5), (1, 2, 300))
    img = np.ascontiguousarray(prng.normal_f32(30, 0, (2, 40, 64)))
    tl = [(y, x) for (_, y, x) in sw.tile_slicers((40, 64), PATCH, 0.5, 1)]
    ty, tx = np.array([t[0] for t in tl], np.int32), np.array([t[1] for t in tl], np.int32)
    desc, maps = (_lib.TiledImage * 1)(), (_lib.TiledLabelmap * 1)()
    d, x = desc[0], maps[0]
    d.image, d.Hp, d.Wp, d.n_tiles, d.tile_y, d.tile_x = img.ctypes.data, 40, 64, len(tl), ty.ctypes.data, tx.ctypes.data
    x.src_y, x.src_x, x.src_h, x.src_w, x.out_h, x.out_w, x.label_u8 = 0, 0, 40, 64, 5, 5, out.ctypes.data
    with Engine(ARCH, weights.pack_blob(ARCH, state_dict(181))) as e:
        handles = (ctypes.c_void_p * 1)(e._h)
        call = lambda o, n: e.lib.ts2d_ensemble_predict_tiled_regions(handles, 1, desc, maps, 1, 32, 32, 3, None, 1, o, n)      # noqa: E731
        assert call(None, 3) == -1 and _lib.last_error() == 'ts2d_ensemble_predict_tiled_regions: regions: the class order is null'
        assert call(order.ctypes.data, 2) == -1
        assert _lib.last_error() == 'ts2d_ensemble_predict_tiled_regions: regions: 2 class values for a model of 3 heads'
        x.label_u8 = None
        assert call(order.ctypes.data, 3) == -1 and _lib.last_error() == 'image 0: regions: the output is null'
        x.label_u8 = out.ctypes.data
        x.out_h = 0
        assert call(order.ctypes.data, 3) == -1 and _lib.last_error() == 'image 0: regions: bad output extent 0x5'
        assert (out == 0xAB).all() and d.inf_flag == 0
        x.out_h = 5
        assert call(order.ctypes.data, 3) == 0 and not (out == 0xAB).all() and set(np.unique(out).tolist()) <= {0, *ORDER}
