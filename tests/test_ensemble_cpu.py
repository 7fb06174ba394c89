"""Fold ensembles on the device, the parts a machine without a GPU can check: the new C-ABI symbol and its argument validation in front
of any device work, the numpy statement of the fold mean (``predictor.fold_mean_f16``) against the predictor's own sum and on the special
values of the half grid, and the guard that predictors without engines (the host doubles) keep the logits route."""
import ctypes
import re

import numpy as np

from tests import cases
from tests.batch_util import HostBatchPredictor
from tests.surface_util import HostModel, synthetic_model
from totalsegmentator2d_amd import _lib, nrrd, prng, weights
from totalsegmentator2d_amd.predictor import fold_mean_f16

NAME = 'ts2d_ensemble_predict_tiled_export'


def test_the_header_declares_the_symbol_the_library_exports_it_and_the_abi_stays_9():
    src = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r'\bint\s+' + NAME + r'\s*\(\s*ts2d_engine\s*\*\s*const\s*\*\s*engines\s*,\s*int\s+n_engines\b', src)
    lib = _lib.load()
    assert hasattr(lib, NAME) and NAME in _lib.SYMBOLS
    assert lib.ts2d_abi_version() == 9 == _lib.ABI_VERSION


def _call(handles, n_engines, n_images=0):
    lib = _lib.load()
    rc = lib.ts2d_ensemble_predict_tiled_export(handles, n_engines, None, None, n_images, 64, 64, 0, None, 1)
    return rc, _lib.last_error()


def test_bad_engine_arrays_are_rejected_by_name_before_any_device_work():
    """No engine exists on a machine without a GPU: every call here must return from the validation of the array itself."""
    rc, msg = _call(None, 2)
    assert rc != 0 and NAME in msg and '2 engines at a null pointer' in msg
    one = (ctypes.c_void_p * 1)(None)
    for n in (0, -1, 33):
        rc, msg = _call(one, n)
        assert rc != 0 and f'n_engines = {n} is outside 1..32' in msg
    rc, msg = _call(one, 1)
    assert rc != 0 and 'engine 0 is null' in msg
    # a handle is only dereferenced after every slot has been found non-null: any address will do in front of the null one
    spare = ctypes.create_string_buffer(64)
    three = (ctypes.c_void_p * 3)(ctypes.addressof(spare), ctypes.addressof(spare), None)
    rc, msg = _call(three, 3, n_images=1)
    assert rc != 0 and 'engine 2 is null' in msg


def _host_predictor(folds, order='float', mirror=(0, 1)):
    arch = cases.unet(2, (32, 32), 3)
    rng_w = [prng.normal_f32(5, 40 + f, (3, arch.input_channels)) for f in range(folds)]

    def network(batch, fold):               # a cheap per-fold "network": a 1x1 mix of the channels, distinct per fold, with some large values
        return np.einsum('kc,bchw->bkhw', rng_w[fold] * (1.0 + 30.0 * fold), batch)
    p = HostBatchPredictor(network=network, tile_step_size=0.5, use_mirroring=mirror is not None, tile_dtype=order)
    p.manual_initialization(arch, [np.zeros(arch.n_params(), np.float32)] * folds, (32, 32), inference_allowed_mirroring_axes=mirror)
    return p


def test_fold_mean_f16_is_the_predictors_own_sum_bit_for_bit():
    for order in ('float', 'half'):
        p = _host_predictor(3, order)
        data = prng.normal_f32(9, 1, (2, 1, 50, 70))
        out = p.predict_logits_from_preprocessed_data(data)
        out = out.cpu().numpy() if hasattr(out, 'cpu') else out
        per_fold = [p.predict_sliding_window_return_logits(data, f) for f in range(3)]
        assert not np.array_equal(per_fold[0], per_fold[1])
        mean = fold_mean_f16(per_fold)
        assert mean.dtype == out.dtype == np.float16 and np.array_equal(mean.view(np.uint16), out.view(np.uint16))
        many = [o.cpu().numpy() if hasattr(o, 'cpu') else o for o in p.predict_logits_from_preprocessed_data_batch([data, data[:, :, :40]])]
        assert np.array_equal(many[0].view(np.uint16), mean.view(np.uint16))
    one = np.arange(6, dtype=np.float16)
    assert fold_mean_f16([one]) is not None and np.array_equal(fold_mean_f16([one]), one)          # upstream divides only when n > 1


def _half(bits):
    return np.array(bits, dtype=np.uint16).view(np.float16)


def test_fold_mean_f16_on_the_special_values_of_the_half_grid():
    """(a, b, F = 2 result) and (a, b, c, F = 3 result) as bit patterns, each worked out by hand from 'fp32 operation, then round to
    nearest even to half'."""
    with np.errstate(over='ignore', invalid='ignore'):
        _special_values()


def _special_values():
    sub_min, sub_max, norm_min, big = 0x0001, 0x03FF, 0x0400, 0x7BFF        # 2^-24, the largest subnormal, 2^-14, 65504
    pinf, ninf, pz, nz = 0x7C00, 0xFC00, 0x0000, 0x8000
    two = [
        (sub_min, sub_min, sub_min),          # 2^-24 + 2^-24 = 2^-23, / 2
        (sub_min, pz, pz),                    # 2^-25 is a tie between 0 and 2^-24: to even, +0
        (0x0003, pz, 0x0002),                 # 1.5 * 2^-24 is a tie between 1 and 2 (x 2^-24): to even, 2
        (sub_max, sub_min, 0x0200),           # 1023 + 1 = 1024 (x 2^-24) = 2^-14, / 2 = 2^-15
        (sub_max, norm_min, 0x0400),          # (1023 + 1024) / 2 = 1023.5 (x 2^-24): a tie, to even 1024
        (big, big, pinf),                     # the half sum overflows before the division: numpy gives inf, and so must the device
        (big, pz, 0x77FF),                    # 65504 / 2 = 32752
        (pinf, big, pinf), (ninf, big, ninf), (pinf, pinf, pinf),
        (pz, nz, pz), (nz, nz, nz), (nz, pz, pz),       # signed zeros: +0 + -0 = +0, -0 + -0 = -0
        (0x8001, pz, nz),                     # -2^-25: the tie rounds to -0
    ]
    for a, b, want in two:
        got = fold_mean_f16([_half([a]), _half([b])]).view(np.uint16)[0]
        assert got == want, (hex(a), hex(b), hex(got), hex(want))
    three = [
        (0x3C00, 0x3C00, 0x3C00, 0x3C00),     # (1 + 1 + 1) / 3 = 1
        (0x3C00, pz, pz, 0x3555),             # 1 / 3 = 0.33325195 (0x3555), the nearest half
        (sub_min, sub_min, sub_min, sub_min),
        (sub_min, pz, pz, pz),                # 2^-24 / 3 is below half the smallest subnormal
        (0x0002, pz, pz, sub_min),            # 2/3 (x 2^-24) rounds to 1
        (big, 0xFBFF, big, 0x7555),           # (65504 - 65504) + 65504 = 65504, / 3 = 21834.67 -> 21840 on the grid of 16
    ]
    for a, b, c, want in three:
        got = fold_mean_f16([_half([a]), _half([b]), _half([c])]).view(np.uint16)[0]
        assert got == want, (hex(a), hex(b), hex(c), hex(got), hex(want))
    assert np.isnan(fold_mean_f16([_half([pinf]), _half([ninf])])[0])                    # inf + -inf: a NaN, whatever its payload
    assert np.isnan(fold_mean_f16([_half([0x7E00]), _half([0x3C00]), _half([0x3C00])])[0])
    # fold order matters, and the statement keeps it: (65504 + 65504) + -65504 = inf, 65504 + (-65504 + 65504) would not be
    assert fold_mean_f16([_half([big]), _half([big]), _half([0xFBFF])]).view(np.uint16)[0] == pinf
    # every half value through F = 2, 3 and 5 against the float64 mean rounded once: the double rounding through fp32 is innocuous here
    allv = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    finite = np.isfinite(allv)
    for F in (2, 3, 5):
        got = fold_mean_f16([allv] + [np.zeros_like(allv)] * (F - 1))
        want = (allv[finite].astype(np.float64) / F).astype(np.float16)
        assert np.array_equal(got[finite].view(np.uint16) & 0x7FFF, want.view(np.uint16) & 0x7FFF)


def test_a_two_fold_host_double_still_takes_the_logits_route():
    """The doubles of the tests have no engines: the segmentation fast path answers None for their ensembles, as before, and the model
    falls back to predict_logits_from_preprocessed_data - the same segmentation with and without device_threshold."""
    m, arch, sd = synthetic_model('ts2d-v2-ep4000b2_cardiac', 3, 61, patch=(32, 32), network=True, feats=(32, 32))
    sd2 = weights.synthetic_state_dict(arch, 62)
    cfg = dict(m._config)
    cfg['synthetic'] = dict(cfg['synthetic'], blobs=[weights.pack_blob(arch, sd), weights.pack_blob(arch, sd2)])
    from oracle import torch_oracle as O
    sds = [sd, sd2]
    cfg['oracle_network'] = lambda batch, fold=0: np.concatenate([O.unet_forward(arch, sds[fold], batch[i:i + 1]).numpy() for i in range(batch.shape[0])])
    model = HostModel(cfg)
    img = nrrd.Image((np.random.default_rng(3).standard_normal((40, 48, 2)) * 200 + 50).astype(np.float32), (1.5, 1.5), (0.0, 0.0),
                     (1.0, 0.0, 0.0, 1.0), 2, {}, None)
    model.start()
    try:
        p = model._predictor
        assert len(p.list_of_parameters) == 2 and p.engines == [] and not p._device_ensemble()
        data = prng.normal_f32(4, 2, (2, 1, 40, 48))
        assert p.predict_segmentation_from_preprocessed_data(data) is None
        assert p.predict_segmentation_from_preprocessed_data_batch([data, data]) is None
        calls = []
        orig = p.predict_logits_from_preprocessed_data
        p.predict_logits_from_preprocessed_data = lambda d: (calls.append(1), orig(d))[1]
        model.device_threshold = True
        a = model.apply(img)
        assert calls, 'the ensemble of a predictor without engines must take the logits route'
        model.device_threshold = False
        b = model.apply(img)
        assert np.array_equal(a.array, b.array) and a.array.any()
    finally:
        model.stop()
