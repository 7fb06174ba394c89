"""Slice stacks (a 3-D volume through a 2-D model) on the MI355X.  The input side: ts2d_planes_create_stack / ts2d_planes_crop_normalize_stack
(csrc/kernels_prep_stack.h) against the numpy statements (tests/stack_util.py; tests/test_stack_cpu.py pins them to numpy) - the box, every bit of
every float32 result, the statistics, the per-slice clip bounds through the resample, the refusals and the status bits.  The output side and the
surface: folder models of the three label conventions through HIPModel.apply / apply_batch with the stack switches on and off - byte-identical
images - and the determinism of the batch method."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import cases
from tests.conftest import GOLDEN
from tests.prep_schemes_util import CT_PROPS, bits
from tests.stack_util import stack_case, stack_statement
from tests.test_gpu_labelmap import _same_image, _write_model_folder
from totalsegmentator2d_amd import _lib
from totalsegmentator2d_amd import engine as engine_module
from totalsegmentator2d_amd import nrrd, prng, weights
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.model import HIPModel
from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor

pytestmark = pytest.mark.gpu
A = os.path.join(GOLDEN, 'assets')
FIP = {str(c): dict(CT_PROPS, mean=5.0 + c, std=20.0 - 3 * c) for c in range(2)}
Z, CT, RS, RGB, NO = P.NORM_SCHEME_IDS
KINDS = {'z-score': [Z], 'ct': [CT], 'rescale': [RS], 'rgb': [RGB], 'none': [NO], 'ct + z-score': [CT, Z]}


# ------------------------------------------------------------------------------------------------ the entry against the statement
def _check(data, kind, out_hw=None):
    C = data.shape[0]
    schemes = [KINDS[kind][i % len(KINDS[kind])] for i in range(C)]
    box, want, status = stack_statement(data, schemes, FIP)
    assert status == 0, (kind, status)
    (z0, z1), (r0, r1), (c0, c1) = box
    with P.DevicePlanes(data, 0, stack=True) as p:
        assert p.crop_normalize_stack(schemes, [False] * C, FIP) == box and p.status == 0 and p.shape == want.shape and p.slices == z1 - z0
        got = p.download()
        diff = bits(got) != bits(want)
        assert not diff.any(), (kind, data.shape, box, int(diff.sum()), np.argwhere(diff)[:4])
        for c, s in enumerate(schemes):
            vol = np.ascontiguousarray(data[c, z0:z1, r0:r1, c0:c1])
            if s == Z:
                assert np.array_equal(bits(p.stats[c]), bits(np.array(P.zscore_stats_f32_statement(vol.reshape(1, -1))[:2]))), (kind, c)
            elif s == CT:
                assert np.array_equal(bits(p.stats[c]), bits(P.ct_f32_parameters(FIP[str(c)])[:2]))
            elif s == RS:
                assert bits(p.stats[c, 0]) == bits(vol.min()) and bits(p.stats[c, 1]) == bits(max(np.float32(vol.max() - vol.min()), np.float32(1e-8)))
            else:
                assert p.stats[c].tolist() == ([0.0, 255.0] if s == RGB else [0.0, 1.0])
        if out_hw is not None:               # the clip bounds the handle kept are each SLICE's minimum and maximum: the resample shows them
            res = P.resample_planes_cubic_device(p, out_hw, 0)
            assert res.shape == want.shape[:2] + tuple(out_hw)
            for c in range(C):
                for k in range(want.shape[1]):               # (resize_cubic_f64 clips to the bounds of the plane it is given: this slice's)
                    assert np.array_equal(bits(res[c, k]), bits(P.resize_cubic_f64(want[c, k], out_hw))), (kind, out_hw, c, k)
    return got


@pytest.mark.parametrize('kind', list(KINDS))
def test_a_stack_with_a_border_on_all_three_axes_equals_the_statement(kind, monkeypatch):
    data = stack_case(51, 2, 5, 37, 70, (1, 1, 2, 3, 4, 5), rgb=kind == 'rgb')
    data[:, 2, 10:12] = 0; data[0, 1:4, 20, 30:40] = 0                               # zeros inside the box, whole rows among them
    _check(data, kind, (50, 61))
    # ... and through run_case_npy under the key, below the product's size gate
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    from types import SimpleNamespace
    schemes = [KINDS[kind][i % len(KINDS[kind])] for i in range(2)]
    pm = SimpleNamespace(transpose_forward=[0, 1, 2], plans={'foreground_intensity_properties_per_channel': FIP})
    cm = SimpleNamespace(spacing=[1.5, 1.5], normalization_schemes=schemes, use_mask_for_norm=[False, False])
    outs = []
    for extra in ({}, {'device_normalize_stack': 0, 'device_resample': 0}):
        props = dict({'spacing': (3.0, 1.0, 0.8)}, **extra)
        outs.append(P.DefaultPreprocessor(verbose=False).run_case_npy(data.copy(), None, props, pm, cm, {}))
    (a, _, pa), (b, _, pb) = outs
    assert a.shape == b.shape == (2, 3, 21, 33) and np.array_equal(bits(a), bits(b)) and pa == pb and pb['bbox_used_for_cropping'] == [[1, 4], [2, 34], [4, 65]]


@pytest.mark.parametrize('kind', list(KINDS))
def test_chunks_that_cross_the_slices_and_a_width_off_the_wave(kind):
    data = stack_case(52, 1, 7, 131, 97, rgb=kind == 'rgb')                          # 12 707 samples a slice: every chunk boundary lies inside a slice
    _check(data, kind, (160, 75))


def test_more_than_2_24_samples_in_a_channel():
    rng = np.random.default_rng(53)
    data = (rng.standard_normal((1, 65, 520, 500), np.float32) * 30 + 7).astype(np.float32)
    assert data.size > 1 << 24
    _check(data, 'z-score')


def test_refusals_by_name_write_nothing():
    lib = _lib.load()
    c = ctypes
    data = stack_case(54, 2, 3, 20, 30, (1, 0, 2, 0, 3, 0))
    ids, par = np.array([P.NORM_SCHEME_IDS[Z]] * 2, np.int32), np.zeros((2, 4), np.float32)
    box, status, stats = (c.c_int32 * 6)(*[7] * 6), c.c_int(7), np.full((2, 2), 7, np.float32)
    with P.DevicePlanes(data, 0, stack=True) as p:
        def call(h, i, q, m, bx, st, code):
            return lib.ts2d_planes_crop_normalize_stack(h, i, q, m, bx, st, code)
        masked = np.array([0, 1], np.uint8)
        assert call(p._h, ids.ctypes.data, par.ctypes.data, masked.ctypes.data, c.byref(box), stats.ctypes.data, c.byref(status)) == -1
        assert 'ts2d_planes_crop_normalize_stack: channel 1 is normalised inside the non-zero mask' in _lib.last_error()
        none = np.zeros(2, np.uint8)
        for args in ((None, ids.ctypes.data, par.ctypes.data, none.ctypes.data, c.byref(box), stats.ctypes.data, c.byref(status)),
                     (p._h, None, par.ctypes.data, none.ctypes.data, c.byref(box), stats.ctypes.data, c.byref(status)),
                     (p._h, ids.ctypes.data, par.ctypes.data, None, c.byref(box), stats.ctypes.data, c.byref(status)),
                     (p._h, ids.ctypes.data, par.ctypes.data, none.ctypes.data, None, stats.ctypes.data, c.byref(status)),
                     (p._h, ids.ctypes.data, par.ctypes.data, none.ctypes.data, c.byref(box), None, c.byref(status))):
            assert call(*args) == -1 and 'ts2d_planes_crop_normalize_stack: null argument' in _lib.last_error()
        bad = np.array([0, 5], np.int32)
        assert call(p._h, bad.ctypes.data, par.ctypes.data, none.ctypes.data, c.byref(box), stats.ctypes.data, c.byref(status)) == -1 and 'unknown scheme 5' in _lib.last_error()
        assert list(box) == [7] * 6 and (stats == 7).all() and p.shape == data.shape and np.array_equal(bits(p.download()), bits(data))
        # the 2-D crop entries refuse a stack
        b4, flag = (c.c_int32 * 4)(), c.c_int()
        assert lib.ts2d_planes_crop_zscore(p._h, c.byref(b4), stats.ctypes.data, c.byref(flag)) == -1 and 'the handle is a stack of 3 slices' in _lib.last_error()
        assert lib.ts2d_planes_crop_normalize(p._h, ids.ctypes.data, par.ctypes.data, none.ctypes.data, c.byref(b4), stats.ctypes.data, c.byref(flag)) == -1
        assert 'the handle is a stack of 3 slices' in _lib.last_error() and np.array_equal(bits(p.download()), bits(data))
    h = c.c_void_p()
    a = np.zeros(8, np.float32)
    for args, word in (((0, a.ctypes.data, 1, 0, 2, 2, c.byref(h)), '1 channels of 0 slices'), ((0, None, 1, 2, 2, 2, c.byref(h)), 'null argument'),
                       ((0, a.ctypes.data, 1, 2, 2, 2, None), 'null argument'),
                       ((0, a.ctypes.data, 1, 1025, 512, 512, c.byref(h)), 'more than one handle takes (2^28 samples)')):
        assert lib.ts2d_planes_create_stack(*args) == -1 and 'ts2d_planes_create_stack: ' in _lib.last_error() and word in _lib.last_error() and h.value is None


def test_status_bits():
    data = stack_case(55, 2, 4, 40, 30, (0, 1, 0, 0, 2, 0))
    nan = data.copy(); nan[1, 2, 7, 7] = np.nan
    for schemes in ([Z, Z], [CT, NO], [RS, RS]):
        with P.DevicePlanes(nan, 0, stack=True) as p:
            assert p.crop_normalize_stack(schemes, [False, False], FIP) is None and p.status == P.PLANES_NONFINITE, schemes
    rgb = stack_case(56, 2, 4, 40, 30, rgb=True); rgb[0, 3, 5, 5] = 256
    with P.DevicePlanes(rgb, 0, stack=True) as p:
        assert p.crop_normalize_stack([RGB, RGB], [False, False], FIP) is None and p.status == P.PLANES_RGB_RANGE
    neg = np.abs(data); neg[0, 1, 4, 4] = -0.0
    assert stack_statement(neg, [RS, RS])[2] == P.PLANES_ZERO_SIGN
    with P.DevicePlanes(neg, 0, stack=True) as p:
        assert p.crop_normalize_stack([RS, RS], [False, False], FIP) is None and p.status == P.PLANES_ZERO_SIGN
    with P.DevicePlanes(neg, 0, stack=True) as p:                                    # ... which is Rescale's alone
        assert p.crop_normalize_stack([Z, NO], [False, False], FIP) is not None and p.status == 0
    zeros = np.zeros((2, 3, 20, 30), np.float32); zeros[1, 2, 3, 4] = -0.0           # a volume of zeros keeps its whole extent
    with P.DevicePlanes(zeros, 0, stack=True) as p:
        assert p.crop_normalize_stack([Z, Z], [False, False], FIP) == [[0, 3], [0, 20], [0, 30]] and not p.download().any()


# ------------------------------------------------------------------------------------------------ the surface
ARCH = cases.unet(3, (32, 32, 64), 6)
PATCH = (64, 64)
DATASETS = {'labelmap': None,
            'multilabel': {'labels': {'background': 0, **{f'organ_{i}': i for i in range(1, 7)}}, 'multilabel': True},
            'regions': {'labels': {'background': 0, **{f'region_{i}': list(range(i, 7)) for i in range(1, 7)}},
                        'regions_class_order': [1, 2, 3, 4, 5, 6]}}


def _folder_model(root, kind, seeds):
    _write_model_folder(root, kind, ARCH, seeds, PATCH)
    extra = DATASETS[kind]
    if extra is not None:
        path = os.path.join(root, 'Dataset001_' + kind, 'nnUNetTrainer__nnUNetPlans__2d', 'dataset.json')
        with open(path) as f:
            ds = json.load(f)
        ds.update(extra)
        with open(path, 'w') as f:
            json.dump(ds, f)
    m = HIPModel({'root': root, 'model': f'ts2d-v2-ep4000b2_{kind}', 'revision': 1, 'folds': tuple(range(len(seeds))), 'param': {'nnu.configuration': '2d'}})
    assert m.multilabel == (kind == 'multilabel')
    return m


def _volume(seed, spacing):
    """A two-component 3-D image [6, 90, 80]: slice 0, four rows and five columns of it are zero."""
    a = np.zeros((6, 90, 80, 2), np.float32)
    a[1:, 3:89, 2:77] = prng.normal_f32(seed, 0, (5, 86, 75, 2)) * 40 + 10
    return nrrd.Image(a, tuple(spacing), (1.0, 2.0, 3.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), 2, {}, 'left-posterior-superior')


class _Calls:
    """Calls INTO THE LIBRARY (the predictor looks the functions up at call time), and the planes the stack methods hand to the model."""
    def __init__(self, monkeypatch, p):
        self.tiled, self.planes, self.crops = [], [], []
        for name in ('predict_tiled_labelmap_ensemble', 'predict_tiled_regions_ensemble', 'predict_tiled_export_ensemble'):
            orig = getattr(engine_module, name)
            monkeypatch.setattr(engine_module, name, lambda engines, images, *a, _o=orig, _n=name, **kw:
                                (self.tiled.append((_n, len(engines), len(images), bool(kw.get('full_batch', True)))), _o(engines, images, *a, **kw))[1])
        for name in ('predict_stack_from_preprocessed_data', 'predict_stack_from_preprocessed_data_batch'):
            fn = getattr(p, name)
            monkeypatch.setattr(p, name, lambda data, *a, _f=fn, _b=name.endswith('_batch'), **kw:
                                (lambda out: (self.planes.extend(out if _b else [out]), out)[1])(_f(data, *a, **kw)))
        orig_crop = P.DevicePlanes.crop_normalize_stack
        monkeypatch.setattr(P.DevicePlanes, 'crop_normalize_stack', lambda s, *a, **kw: (lambda box: (self.crops.append(box), box)[1])(orig_crop(s, *a, **kw)))

    def clear(self):
        del self.tiled[:], self.planes[:], self.crops[:]


@pytest.mark.parametrize('kind,folds', [('labelmap', 1), ('labelmap', 2), ('multilabel', 1), ('regions', 1)])
def test_stacks_through_apply_and_apply_batch_equal_the_host_route(tmp_path, kind, folds, monkeypatch):
    stacks = {'on': _volume(61, (1.5, 1.5, 3.0)), 'off': _volume(62, (0.8, 1.0, 3.0))}
    many = dict(stacks, flat=nrrd.read(os.path.join(A, 'sample_s0616.nrrd')))
    entry = {'labelmap': 'predict_tiled_labelmap_ensemble', 'regions': 'predict_tiled_regions_ensemble', 'multilabel': 'predict_tiled_export_ensemble'}[kind]
    K = 6
    m = _folder_model(str(tmp_path), kind, list(range(71, 71 + folds)))
    m.start()
    try:
        p = m._predictor
        assert len(p.engines) == folds and p.arch.num_classes == K and m.device_input_stack and m.device_stack
        lead = K if kind == 'multilabel' else 1
        # two and a half slices of the first stack (86 x 75: inputs, the folds' half outputs, the decided planes) per call: a stack of five is
        # split, a call boundary falls inside each stack, and one call holds slices of both
        p.stack_call_bytes = int(2.5 * (2 * 86 * 75 * 4 + folds * K * 86 * 75 * 2 + 86 * 75 * lead))
        calls = _Calls(monkeypatch, p)

        def run():
            calls.clear()
            single = {k: m.apply(v) for k, v in stacks.items()}
            seen = list(calls.tiled), list(calls.planes), list(calls.crops)
            calls.clear()
            return single, m.apply_batch(dict(many)), seen, (list(calls.tiled), list(calls.planes), list(calls.crops))

        m.device_input_stack = m.device_stack = False
        host, host_many, seen, seen_many = run()
        assert not seen[1] and not seen[2] and not seen_many[1] and not seen_many[2] and not any(t[2] > 1 or t[0] != entry for t in seen[0])
        m.device_input_stack = m.device_stack = True
        dev, dev_many, seen, seen_many = run()
        # the input route ran once per stack, the output route one call per slice (apply) and packed full-batch calls (apply_batch)
        box = [[1, 6], [3, 89], [2, 77]]
        assert seen[2] == [box, box] and seen_many[2] == [box, box]
        assert seen[0] == [(entry, folds, 1, False)] * 10
        packed = [t for t in seen_many[0] if t[3]]
        assert all(t[0] == entry and t[1] == folds for t in packed) and sum(t[2] for t in packed) >= 10 and len([t for t in packed if t[2] > 1]) >= 4
        assert max(t[2] for t in packed) <= 3
        assert [pl.shape for pl in seen[1]] == [(lead, 5, 86, 75)] * 2 and [pl.shape for pl in seen_many[1]] == [(lead, 5, 86, 75)] * 2
        assert all(pl.dtype == np.uint8 for pl in seen[1] + seen_many[1])
        for k in stacks:
            assert _same_image(dev[k], host[k]), k
            assert dev[k].array.shape == ((6, 90, 80, K) if kind == 'multilabel' else (6, 90, 80)) and not dev[k].array[0].any() and (kind != 'labelmap' or len(np.unique(dev[k].array)) >= 2)
        for k in many:
            assert _same_image(dev_many[k], host_many[k]), k
        # one switch at a time: the same bytes again
        for inp, out in ((True, False), (False, True)):
            m.device_input_stack, m.device_stack = inp, out
            one, one_many, seen, seen_many = run()
            assert bool(seen[2]) == inp and bool(seen[1]) == out and bool(seen_many[2]) == inp and bool(seen_many[1]) == out
            assert all(_same_image(one[k], host[k]) for k in stacks) and all(_same_image(one_many[k], host_many[k]) for k in many), (inp, out)
    finally:
        m.stop()


def test_a_stack_does_not_depend_on_the_call_budget_nor_on_its_batch_mates():
    ds = {'channel_names': {'0': 'a', '1': 'b'}, 'labels': {'background': 0, **{f'l{i}': i for i in range(1, 6)}}, 'file_ending': '.nrrd'}
    p = HIPnnUNetPredictor()
    p.manual_initialization(ARCH, [weights.pack_blob(ARCH, weights.synthetic_state_dict(ARCH, 81))], PATCH, dataset_json=ds)
    try:
        stack = prng.normal_f32(82, 0, (2, 5, 70, 90))
        mates = [prng.normal_f32(82, 1, (2, 3, 64, 64)), prng.normal_f32(82, 2, (2, 1, 100, 70))]
        assert p.stack_call_bytes == 1 << 30
        alone = p.predict_stack_from_preprocessed_data_batch([stack], [(5, 93, 61)])[0]
        assert alone.dtype == np.uint8 and alone.shape == (1, 5, 93, 61) and len(np.unique(alone)) >= 2
        for budget in (1, 400_000, 1 << 21):
            p.stack_call_bytes = budget
            got = p.predict_stack_from_preprocessed_data_batch([mates[0], stack, mates[1]], [None, (5, 93, 61), (1, 50, 80)])
            assert [g.shape for g in got] == [(1, 3, 64, 64), (1, 5, 93, 61), (1, 1, 50, 80)] and np.array_equal(got[1], alone), budget
        one = p.predict_stack_from_preprocessed_data(stack, (5, 93, 61))
        assert one.shape == alone.shape and (one == alone).mean() > 0.95            # (the size-dependent dispatch: the host route's bytes for `apply`, a few half ulps away)
        assert p.predict_stack_from_preprocessed_data(stack, (4, 93, 61)) is None and p.predict_stack_from_preprocessed_data(stack, (93, 61)) is None
        assert p.predict_stack_from_preprocessed_data_batch([stack], [None, None]) is None and p.predict_stack_from_preprocessed_data_batch([]) == []
    finally:
        p.close()
