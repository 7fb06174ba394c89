"""Probabilities of slice stacks on the MI355X: the entry ts2d_ensemble_predict_tiled_probabilities_stack (csrc/kernels_prob.h:
sw_probabilities<ProbStackSeg>) under the predictor's stack probabilities methods - every slice held to the checks of
tests/test_gpu_probabilities.py on the half logits of the same call, the slabs outside the box exact, the bytes those of the per-image entry and
of the decided-map route, whatever the call budget and the batch-mates - ``HIPModel.apply(save_probabilities=True)`` of 3-D volumes against the
host route, and the entry's refusals.  Every figure is printed before it is asserted (run with -s)."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from tests import prob_util
from tests.test_gpu_probabilities import ARCH, PATCH, _check, _predictor
from tests.test_gpu_stack import _folder_model, _volume
from totalsegmentator2d_amd import _lib, export, nrrd, prng, weights
from totalsegmentator2d_amd import engine as engine_module
from totalsegmentator2d_amd.model import HIPModel

pytestmark = pytest.mark.gpu

# (extent after resampling back, extent before cropping, origin of the crop box) of a [2, 3, 70, 90] stack: resampled into a width that is a
# multiple of 4 (the vector stores) with fill slabs in front and behind; the identity in an odd width (the scalar stores) with one slab behind
GEOMETRIES = [((3, 81, 100), (5, 88, 104), (1, 3, 4)), ((3, 70, 90), (4, 73, 101), (0, 2, 7))]


class _Calls:
    """Every call into the library's stack entry, with the half logits asked for in the SAME call."""
    def __init__(self, monkeypatch):
        self.seen = []
        orig = engine_module.predict_tiled_probabilities_stack_ensemble

        def wrapped(engines, images, patch, tiles, runs, mode, *a, **kw):
            kw['want_logits'] = True
            logits = orig(engines, images, patch, tiles, runs, mode, *a, **kw)
            self.seen.append((len(engines), bool(kw.get('full_batch', True)), [(r[0], r[1], r[2]) for r in runs], mode, logits))
            return logits
        monkeypatch.setattr(engine_module, 'predict_tiled_probabilities_stack_ensemble', wrapped)

    def pop(self):
        out = list(self.seen)
        del self.seen[:]
        return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_volume(dec, prob, slices, out, full, box, mode, order, name):
    """`slices`: per slice of the stack ``(half logits [K,Hp,Wp], source rectangle)``.  Every slice inside the box by the 2-D checks, the slabs
    outside it exactly the fill."""
    K = prob.shape[0]
    assert prob.dtype == np.float32 and prob.shape == (K,) + full and dec.dtype == np.uint8 and dec.shape == ((K if mode == 'multilabel' else 1),) + full
    for z, (lg, rect) in enumerate(slices):
        Z = box[0] + z
        _check(prob[:, Z], dec[:, Z] if mode == 'multilabel' else dec[0, Z], lg, rect, out[1:], full[1:], box[1:], mode, order, f'{name} z={z}')
    slab = np.ones(full[0], bool)
    slab[box[0]:box[0] + len(slices)] = False
    assert slab.sum() == full[0] - len(slices) and (dec[:, slab] == 0).all(), name
    assert (prob[1:, slab] == 0).all() and (prob[0, slab] == (1 if mode == 'labelmap' else 0)).all(), name


# ------------------------------------------------------------------------------------------------ 1. the engine path
@pytest.mark.parametrize('folds', [1, 2])
@pytest.mark.parametrize('mode', export.PROBABILITY_MODES)
def test_engine_path_one_call_per_slice_and_one_run_of_slices(mode, folds, monkeypatch):
    p = _predictor(mode, folds)
    try:
        calls = _Calls(monkeypatch)
        order = p.regions_class_order
        data = prng.normal_f32(41, 0, (2, 3, 70, 90))
        for out, full, box in GEOMETRIES:
            rect = (0, 0, 70, 90) + out[1:] + full[1:] + box[1:]
            dec, prob = p.predict_stack_probabilities_from_preprocessed_data(data, out, full, box)
            seen = calls.pop()
            assert [(c[0], c[1], c[2], c[3]) for c in seen] == [(folds, False, [(0, 1, rect)], mode)] * 3
            _check_volume(dec, prob, [(c[4][0], rect[:4]) for c in seen], out, full, box, mode, order, f'stack single {mode} F={folds} out={out}')
            (dec, prob), = p.predict_stack_probabilities_from_preprocessed_data_batch([data], [out], [full], [box])
            (F, fb, runs, m, logits), = calls.pop()
            assert (F, fb, runs, m) == (folds, True, [(0, 3, rect)], mode) and len(logits) == 3
            _check_volume(dec, prob, [(lg, rect[:4]) for lg in logits], out, full, box, mode, order, f'stack batch {mode} F={folds} out={out}')
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 2., 3. against the code that exists; budget and batch-mates
@pytest.mark.parametrize('mode', export.PROBABILITY_MODES)
def test_the_batch_method_has_the_bytes_of_the_per_image_entry_whatever_the_budget_and_the_mates(mode):
    p = _predictor(mode, 1)
    try:
        data = prng.normal_f32(42, 0, (2, 3, 70, 90))
        mates = [prng.normal_f32(42, 1, (2, 2, 64, 66)), prng.normal_f32(42, 2, (2, 1, 100, 70))]
        assert p.stack_call_bytes == 1 << 30
        for out, full, box in GEOMETRIES:
            (dec, prob), = p.predict_stack_probabilities_from_preprocessed_data_batch([data], [out], [full], [box])
            # the slices as separate single-slice cases of the probabilities method that existed
            flat = p.predict_probabilities_from_preprocessed_data_batch([data[:, z:z + 1] for z in range(3)], [out[1:]] * 3, [full[1:]] * 3, [box[1:]] * 3)
            for z, (d2, p2) in enumerate(flat):
                assert np.array_equal(_bits(prob[:, box[0] + z]), _bits(p2[:, 0])) and np.array_equal(dec[:, box[0] + z], d2[:, 0]), (out, z)
            # the decided bytes inside the box: the stack route without the flag
            maps, = p.predict_stack_from_preprocessed_data_batch([data], [out])
            inside = tuple(slice(b, b + o) for b, o in zip(box, out))
            assert maps.shape == dec[(slice(None),) + inside].shape and np.array_equal(dec[(slice(None),) + inside], maps), out
            # a budget of one image per call, one that splits the stack (a slice and a half), the default; alone and between two mates
            one = 2 * 70 * 90 * 4 + 3 * 70 * 90 * 2 + full[1] * full[2] * (3 * 4 + (3 if mode == 'multilabel' else 1))
            for budget in (1, int(1.5 * one), 1 << 30):
                p.stack_call_bytes = budget
                (d3, p3), = p.predict_stack_probabilities_from_preprocessed_data_batch([data], [out], [full], [box])
                got = p.predict_stack_probabilities_from_preprocessed_data_batch([mates[0], data, mates[1]], [None, out, (1, 50, 80)],
                                                                                 [(3, 64, 70), full, None], [(1, 0, 2), box, None])
                assert [g[1].shape for g in got] == [(3, 3, 64, 70), (3,) + full, (3, 1, 50, 80)]
                for d, pr in ((d3, p3), got[1]):
                    assert np.array_equal(d, dec) and np.array_equal(_bits(pr), _bits(prob)), (out, budget)
            p.stack_call_bytes = 1 << 30
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 4. HIPModel.apply end to end
@pytest.mark.parametrize('mode', export.PROBABILITY_MODES)
def test_model_apply_of_volumes_device_route_against_host_route(mode, monkeypatch, tmp_path):
    class Recording(HIPModel):
        def _preprocess_input(self, img):
            out = super()._preprocess_input(img)
            self.props.append(out[2])
            return out

        def _predict(self, datas, *a, **kw):
            out = super()._predict(datas, *a, **kw)
            self.logits += out
            return out
    K = 6
    imgs = {'on': _volume(61, (1.5, 1.5, 3.0)), 'off': _volume(62, (0.8, 1.0, 3.0))}
    m = _folder_model(str(tmp_path / 'model'), mode, [71])
    m.__class__ = Recording
    m.props, m.logits = [], []
    m.start()
    try:
        p = m._predictor
        assert m.device_stack_probabilities is True and callable(getattr(p, 'predict_stack_probabilities_from_preprocessed_data', None)) \
            and callable(getattr(p, 'predict_stack_probabilities_from_preprocessed_data_batch', None)) and engine_module.has_stack_probabilities()
        calls = _Calls(monkeypatch)
        plain = {k: m.apply({k: v})[k] for k, v in imgs.items()}
        plain_batch = m.apply_batch(dict(imgs))
        assert not calls.pop() and not m.logits
        dev = {k: m.apply({k: v}, save_probabilities=True)[k] for k, v in imgs.items()}
        seen = calls.pop()
        assert len(seen) == 10 and not any(c[1] for c in seen) and not m.logits                 # one call per slice; the device route: no logits travel
        files = m.apply_batch(dict(imgs), str(tmp_path / 'out'), save_probabilities=True)
        seen = calls.pop()
        assert seen and all(c[1] for c in seen) and sum(r[1] for c in seen for r in c[2]) == 10 and not m.logits
        m.device_stack_probabilities = False
        host = {k: m.apply({k: v}, save_probabilities=True)[k] for k, v in imgs.items()}
        host_batch = m.apply_batch(dict(imgs), save_probabilities=True)
        assert not calls.pop() and len(m.logits) == 4
    finally:
        m.stop()
    assert sorted(os.listdir(tmp_path / 'out')) == ['off.npz', 'off.nrrd', 'off.pkl', 'on.npz', 'on.nrrd', 'on.pkl']
    softmax = mode == 'labelmap'
    for i, k in enumerate(imgs):
        props = m.props[-2 + i]
        assert np.array_equal(dev[k].array, plain[k].array) and np.array_equal(host[k].array, plain[k].array) and dev[k].meta == host[k].meta
        assert np.array_equal(nrrd.read(files[k]).array, plain_batch[k].array) and np.array_equal(host_batch[k].array, plain_batch[k].array)
        saved = np.load(files[k][:-5] + '.npz')['probabilities']
        with open(files[k][:-5] + '.pkl', 'rb') as f:
            assert tuple(pickle.load(f)['shape_before_cropping']) == (6, 90, 80)
        tgt, full = tuple(props['shape_after_cropping_and_before_resampling']), tuple(props['shape_before_cropping'])
        box = tuple(b[0] for b in props['bbox_used_for_cropping'])
        assert full == (6, 90, 80) and box == (1, 3, 2) and tgt == (5, 86, 75)
        inside = (slice(None),) + tuple(slice(b, b + t) for b, t in zip(box, tgt))
        outside = np.ones(full, bool)
        outside[inside[1:]] = False
        for name, got, ref, lg in (('apply', dev[k].probabilities, host[k].probabilities, m.logits[i]), ('apply_batch', saved, host_batch[k].probabilities, m.logits[2 + i])):
            lg = np.asarray(lg)
            assert got.dtype == np.float32 and got.shape == (K, 6, 90, 80) and lg.dtype == np.float16 and lg.shape[:2] == (K, 5)
            assert np.array_equal(ref, export.stack_probabilities_statement(lg, (0, 0) + lg.shape[2:], tgt[1:], full, box, mode))
            assert np.array_equal(got[:, outside], ref[:, outside])
            v = np.stack([prob_util.resampled(lg[:, z], (0, 0) + lg.shape[2:], tgt[1:]) for z in range(5)], axis=1)
            prob_util.assert_within(prob_util.measure(f'model volume {mode} {k} {name}', got[inside], v, softmax))


# ------------------------------------------------------------------------------------------------ 5. validation
def test_bad_runs_are_refused_by_name_and_nothing_is_written():
    from totalsegmentator2d_amd import sliding_window as sw
    from totalsegmentator2d_amd.engine import Engine
    img = np.ascontiguousarray(prng.normal_f32(30, 0, (2, 64, 80)))
    tl = [(y, x) for (_, y, x) in sw.tile_slicers((64, 80), PATCH, 0.5, 1)]
    ty, tx = np.array([t[0] for t in tl], np.int32), np.array([t[1] for t in tl], np.int32)
    prob, dec = np.full((3, 3, 6, 7), 7.0, np.float32), np.full((3, 6, 7), 0xAB, np.uint8)
    desc, rd = (_lib.TiledImage * 3)(), (_lib.TiledProbabilitiesRun * 2)()
    for d in desc:
        d.image, d.Hp, d.Wp, d.n_tiles, d.tile_y, d.tile_x = img.ctypes.data, 64, 80, len(tl), ty.ctypes.data, tx.ctypes.data

    def good():
        for r, (first, n) in enumerate(((0, 2), (2, 1))):
            x = rd[r]
            x.src_y, x.src_x, x.src_h, x.src_w, x.out_h, x.out_w, x.full_h, x.full_w, x.box_y, x.box_x = 0, 0, 64, 80, 5, 5, 6, 7, 1, 2
            x.first_image, x.n_slices = first, n
            x.prob_f32, x.prob_head_stride = prob.ctypes.data + first * 42 * 4, 3 * 42
            x.decided_u8, x.decided_head_stride = dec.ctypes.data + first * 42, 0
    entry = 'ts2d_ensemble_predict_tiled_probabilities_stack'
    order = np.array((1, 2, 3), np.uint8)
    with Engine(ARCH, weights.pack_blob(ARCH, weights.synthetic_state_dict(ARCH, 181))) as e:
        handles = (ctypes.c_void_p * 1)(e._h)

        def call(mode=1, o=None, n=0, n_images=3, n_runs=2, runs=rd):
            return getattr(e.lib, entry)(handles, 1, desc, n_images, runs, n_runs, 64, 64, 3, None, 1, mode, o, n)

        def refused(msg, **kw):
            assert call(**kw) == -1 and _lib.last_error() == msg, (msg, _lib.last_error())
            assert (prob == 7.0).all() and (dec == 0xAB).all() and not any(d.inf_flag for d in desc)
        good()
        rd[1].first_image = 1
        refused(f'{entry}: run 1: probabilities: begins at image 1 and overlaps the run before it, which ends at image 1')
        good()
        rd[0].n_slices = 1
        refused(f'{entry}: run 1: probabilities: begins at image 2 and leaves a gap behind image 0')
        good()
        refused(f'{entry}: probabilities: the 1 runs end at image 1 and leave a gap to the call\'s 3 images', n_runs=1)
        rd[1].n_slices = 2
        refused(f'{entry}: run 1: probabilities: 2 slices from image 2 leave the call\'s 3 images')
        good()
        rd[0].prob_head_stride = 2 * 42 - 1
        refused(f'{entry}: run 0: probabilities: head stride 83 is below 2 slices of 6x7')
        good()
        rd[0].decided_head_stride = 42
        refused(f'{entry}: run 0: probabilities: decided head stride 42 is below 2 slices of 6x7', mode=0)
        good()
        rd[1].prob_f32 = None
        refused(f'{entry}: run 1: probabilities: the output is null')
        good()
        refused(f'{entry}: probabilities: unknown mode 5', mode=5)
        refused(f'{entry}: probabilities: the class order is null', mode=2, n=3)
        refused(f'{entry}: probabilities: 2 class values for a model of 3 heads', mode=2, o=order.ctypes.data, n=2)
        refused(f'{entry}: 0 runs at a null pointer', runs=None, n_runs=0)
        rd[1].out_h = 0                                  # what the sibling entry refuses, in its words, with the run named
        refused('run 1: image 2: probabilities: bad output extent 0x5')
        good()
        rd[0].box_y = 2
        refused('run 0: image 0: probabilities: the 5x5 output at (2,2) leaves the full extent 6x7')
        good()
        desc[1].Wp = 96
        refused(f'{entry}: run 0: image 1: probabilities: the padded extent 64x96 differs from 64x80 of the run\'s first image')
        desc[1].Wp = 80
        assert call(n_images=0, n_runs=0, runs=None) == 0 and (prob == 7.0).all() and (dec == 0xAB).all()
        assert call() == 0 and not (prob == 7.0).any() and not (dec == 0xAB).any()
        assert np.abs(prob[:, :, 1:, 2:].sum(0) - 1).max() < 1e-6 and (prob[0, :, 0] == 1).all() and (prob[1:, :, :, :2] == 0).all()
        # a run of one slice whose stride is the plane has the sibling entry's bytes
        p1, d1 = np.full((3, 6, 7), 7.0, np.float32), np.full((6, 7), 0xAB, np.uint8)
        pd = (_lib.TiledProbabilities * 1)()
        x = pd[0]
        x.src_y, x.src_x, x.src_h, x.src_w, x.out_h, x.out_w, x.full_h, x.full_w, x.box_y, x.box_x = 0, 0, 64, 80, 5, 5, 6, 7, 1, 2
        x.prob_f32, x.decided_u8 = p1.ctypes.data, d1.ctypes.data
        assert e.lib.ts2d_ensemble_predict_tiled_probabilities(handles, 1, desc, pd, 1, 64, 64, 3, None, 1, 1, None, 0) == 0
        p2, d2 = np.full((3, 6, 7), 7.0, np.float32), np.full((6, 7), 0xAB, np.uint8)
        good()
        rd[0].n_slices, rd[0].prob_f32, rd[0].prob_head_stride, rd[0].decided_u8 = 1, p2.ctypes.data, 42, d2.ctypes.data
        assert call(n_images=1, n_runs=1) == 0 and np.array_equal(_bits(p2), _bits(p1)) and np.array_equal(d2, d1)
        assert np.array_equal(_bits(prob[:, 0]), _bits(p1)) and np.array_equal(dec[0], d1)       # (full batch: the same image in a run of two)
