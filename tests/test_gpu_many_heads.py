"""MANY-CLASS HEADS on the MI355X: K above 26, and the kernel ``head_1x1`` (csrc/kernels.h) that serves every model with more than 32 heads.

``kernel_name()`` answers ``head`` for both head kernels, so a case here pins the kernel it means by its CONSTRUCTION - the condition of
``pick_kernel`` (csrc/dispatch.cpp) is restated in :func:`_head_kernel` and asserted per case:
  K > 32, or level-0 width 64 (also (40, 48), which ``pad_arch`` runs at 64)        -> ``head_1x1<C>`` in every mode
  K <= 32 at width 32, W % 32 == 0, default options, split / 16-bit mode             -> ``head_mfma32`` (csrc/kernels_head.h)
  the same with the option ``one`` = 0, the exact mode, or W % 32 != 0                -> ``head_1x1<32>``

Nets: two stages, one conv per stage (``cases.unet(2, feats, K, nconv=1)``), weights ``synthetic_state_dict(arch, 300 + K)``, inputs
``cases.make_input(arch, B, H, W, 300 + K)``, engine option ``sbk`` = 0: (32, 32) with K in {1, 31, 32, 33, 118, 256}, (64, 64) with K in
{7, 40, 256}, (40, 48) with K = 118.  Inputs: B = 3 of 16 x 32 (whole 256-pixel blocks), B = 3 of 4 x 32 (384 pixels: the first block of
``head_1x1`` holds the pixels of two images, the second is half valid; per layer only: its level 1 has 32 pixels per image), B = 5 of 6 x 20 (logits only: W is no
multiple of 32, a block spans more than two images; the engine accepts this extent as it stands).

  a. every op that ran, all rows, under tests/layer_check.py - the head against the float64 head (16-bit mode: the ``emulate='f16'`` head)
     on the engine's own ``dec0.c0``, bounds: the fixed ones of that module (``HEAD_RTOL`` 1e-6 / 1e-6 / 1.5e-3).  The float32 torch head is
     2.0e-7 (C = 32) ... 4.0e-7 (C = 64) of the largest logit away from the float64 head on these nets, so ``max(HEAD_RTOL, 2 E_head)`` would
     be ``HEAD_RTOL`` everywhere: no case needs the second term, none uses it.
  b. end to end against ``torch_oracle.unet_forward``: 1e-4 (split, exact); 16-bit mode: ``F16E_MAX`` / ``F16E_RMS`` of
     tests/test_gpu_parity.py against ``emulate='f16'``.
  c. packed masks of ``forward(x, logits=True, mask=True)``: every plane equals ``v > kSigmoidHalfThreshold`` on the engine's own logits bit
     for bit; against the float64 network (16-bit mode: the 16-bit oracle) a bit differs only within the measured logit error of the
     threshold; every head's plane holds both values.  ONE exception, found on the CPU reference and stated there: head 9 of the (40, 48) net
     is positive on every pixel of its input (smallest reference logit 0.27), so "both values" is asserted for the heads whose REFERENCE
     plane holds both values clear of the threshold by the measured error - all K heads of the other nine nets, 117 of 118 of that one.
  d. a logits-only and a mask-only call give the bytes of the combined call (the ``a.logits != nullptr`` / ``a.mask != nullptr`` branches).
  e. K = 118 and 256: rows 0 and 2 of the B = 3 forward are bit-identical to those rows alone.
  f. K = 118 with the last head's bias infinite: the engine's non-finite error, then a clean forward on the same handle passes b.
Then the sliding window and the exports at K = 118 and 256 ((32, 32) net, data ``prng.normal_f32(300 + K, 999, (2, 1, 40, 52))``, patch
(32, 32), step 0.5, mirror axes (0, 1)): device aggregation against the host restatement bit for bit in both tile orders; the label-map
entry (one fold, two folds with seeds 300 + K and 301 + K; split and 16-bit mode; identity and up to (71, 87)) against
``export.labelmap_statement`` of its own half logits byte for byte, with at least 20 distinct labels >= 32 in the map of the network's extent and 12
in the resampled one (the reference's own counts set both, see the test); the probabilities
entry (softmax) with the label-map entry's segmentation bytes and probabilities under tests/prob_util.py.
tests/test_layer_check_cpu.py shows, without a GPU, which seeded head defects bounds a. and b. catch.

NOT covered: logit buffers beyond 2^31 elements (K = 256 at 64 x 512 x 512 is 17 GB; no host reference fits a test).

MEASURED on an MI355X, 256 CUs (printed by every case as ``[many-heads]``; read them with ``pytest -s``).  Worst |engine head - reference
head| over all rows and the inputs a kernel served, as a fraction of the largest reference logit, split | exact | 16-bit mode (``HEAD_RTOL``
1e-6 | 1e-6 | 1.5e-3; ``head_mfma32`` does not serve the exact mode; ``head_1x1<32>`` at K <= 32: the ``one`` = 0 pass, the exact mode, 6 x 20):
  head_mfma32  C=32 K=1     1.5e-7 |   -    | 2.1e-5        head_1x1<32> K=1     2.0e-7 | 1.6e-7 | 4.3e-4
  head_mfma32  C=32 K=31    2.8e-7 |   -    | 5.6e-5        head_1x1<32> K=31    2.2e-7 | 2.7e-7 | 4.7e-4
  head_mfma32  C=32 K=32    2.3e-7 |   -    | 7.8e-5        head_1x1<32> K=32    2.3e-7 | 2.3e-7 | 3.2e-4
  head_1x1<32> K=33         2.4e-7 | 2.2e-7 | 3.9e-4        head_1x1<64> K=7     3.8e-7 | 3.4e-7 | 3.8e-4
  head_1x1<32> K=118        2.8e-7 | 3.8e-7 | 3.7e-4        head_1x1<64> K=40    4.5e-7 | 4.5e-7 | 4.0e-4
  head_1x1<32> K=256        2.5e-7 | 2.5e-7 | 3.5e-4        head_1x1<64> K=256   4.1e-7 | 4.2e-7 | 3.4e-4
  head_1x1<64> K=118 (40, 48)  2.9e-7 | 2.7e-7 | 3.7e-4
Nothing grows with K.  ``head_1x1`` is 3.2e-4 ... 4.7e-4 from the 16-bit oracle where ``head_mfma32`` is 2.1e-5 ... 7.8e-5: it multiplies fp32 weights
with the fp32-normalised stored value where the oracle (and ``head_mfma32``) round both to fp16 - the CPU shows 2.1e-4 ... 5.3e-4 for exactly that
difference on these nets, so this is the contract's width, a third of ``HEAD_RTOL['f16']``, and no defect.  End to end (b.): 3.4e-6 split, 2.9e-6
exact (bound 1e-4); 16-bit mode 4.2e-3 max / 5.0e-4 rms (0.1 / 0.012).  Masks (c.): no bit differs from the float64 network in the split and exact
mode; 0 ... 61 of up to 393 216 bits in the 16-bit mode, all within the logit error of the threshold.
Distinct labels >= 32 in the device's label maps (label-map entry; extent of the network | (71, 87)), one fold / two folds:
  K = 118   30 | 17  /  24 | 19        K = 256   40 | 21  /  53 | 37        (split and 16-bit mode alike; the CPU reference gives the same eight counts)
Probabilities entry: 10 ... 19 float32 units where torch's own softmax is 10 ... 19 from float64 (bound 2 x + 1); every case of this module takes about a
second or less.
"""
import numpy as np
import pytest

from oracle import torch_oracle as O
from tests import cases, prob_util
from tests import layer_check as LC
from tests.conftest import blob_for
from tests.host_predictor import HostLogicPredictor
from tests.test_gpu_default_dispatch import _ran
from tests.test_gpu_full_batch_layers import _f16_exempt
from tests.test_gpu_labelmap import _close, _engines, _plan, _same16
from tests.test_gpu_parity import F16E_MAX, F16E_RMS, TOL, assert_flips_are_tolerance_flips
from tests.test_gpu_probabilities import _check as _check_probabilities
from totalsegmentator2d_amd import export, prng, weights
from totalsegmentator2d_amd import sliding_window as sw
from totalsegmentator2d_amd.engine import (Engine, predict_tiled_labelmap_ensemble, predict_tiled_probabilities_ensemble, unpack_mask)
from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor

pytestmark = pytest.mark.gpu

MODES = ('split', 'exact', 'f16')
THR = np.float32(1.5 * 2.0 ** -24)   # kSigmoidHalfThreshold = 0x1.8p-24f (csrc/device_tables.h), restated
NETS = [((32, 32), K) for K in (1, 31, 32, 33, 118, 256)] + [((64, 64), K) for K in (7, 40, 256)] + [((40, 48), 118)]
WHOLE, HALF, RAGGED = (3, 16, 32), (3, 4, 32), (5, 6, 20)
MEMO = {}
_refs = {}


@pytest.fixture(autouse=True)
def _full_batch_dispatch():
    """Option ``sbk`` = 0 on every handle of this module, the predictors' included (tests/test_gpu_predictor.py: the device path feeds the
    network chunks, the host side one batch, so the network must not depend on the batch)."""
    old = dict(Engine.default_options)
    Engine.default_options = {**old, 'sbk': 0}
    yield
    Engine.default_options = old


def _net(feats, K):
    arch = cases.unet(2, feats, K, nconv=1)
    sd, blob = blob_for(arch, 300 + K)
    return arch, sd, blob


def _width0(arch):
    return -(-arch.features_per_stage[0] // 32) * 32            # csrc/program.cpp pad_arch


def _head_kernel(arch, H, W, mode, one):
    """``pick_kernel`` of csrc/dispatch.cpp for the head, restated (program.cpp packs the MFMA weights for ``ct == 32 && cout <= 32`` only)."""
    mfma = _width0(arch) == 32 and arch.num_classes <= 32 and mode != 'exact' and one == 1 and (H * W) % 32 == 0 and W % 32 == 0
    return 'head_mfma32' if mfma else f'head_1x1<{_width0(arch)}>'


def _forward64(arch, sd, x):
    """The two-stage, one-conv-per-stage net in float64 from end to end (nothing rounded to float32 on the way)."""
    import torch
    import torch.nn.functional as F
    assert arch.n_stages == 2 and tuple(arch.n_conv_per_stage) == (1, 1) and tuple(arch.n_conv_per_stage_decoder) == (1,)
    t = {k: O._t(v).double() for k, v in sd.items()}

    def block(y, k, stride):
        return O.conv_block(y, t[f'{k}.conv.weight'], t[f'{k}.conv.bias'], t[f'{k}.norm.weight'], t[f'{k}.norm.bias'], stride, arch.norm_eps,
                            arch.leaky_slope)
    with torch.no_grad():
        e0 = block(O._t(x).double(), 'encoder.stages.0.0.convs.0', 1)
        e1 = block(e0, 'encoder.stages.1.0.convs.0', tuple(arch.strides[1]))
        up = F.conv_transpose2d(e1, t['decoder.transpconvs.0.weight'], t['decoder.transpconvs.0.bias'], stride=tuple(arch.strides[1]))
        d0 = block(torch.cat((up, e0), 1), 'decoder.stages.0.convs.0', 1)
        out = F.conv2d(d0, t['decoder.seg_layers.0.weight'], t['decoder.seg_layers.0.bias'])
    assert out.dtype == torch.float64
    return out.numpy()


def _ref(feats, K, shape):
    """(input, float32 oracle logits, 16-bit oracle logits, float64 logits) of a case, made once."""
    key = (feats, K, shape)
    if key not in _refs:
        arch, sd, _ = _net(feats, K)
        x = cases.make_input(arch, *shape, 300 + K)
        _refs[key] = (x, O.unet_forward(arch, sd, x).numpy(), O.unet_forward(arch, sd, x, emulate='f16').numpy(), _forward64(arch, sd, x))
    return _refs[key]


def _end_to_end_ok(lg, ref32, ref16, mode):
    if mode == 'f16':
        d = lg - ref16
        mx, rms = float(np.abs(d).max()), float(np.sqrt((d.astype(np.float64) ** 2).mean()))
        return mx <= F16E_MAX and rms <= F16E_RMS, f'max {mx:.2e} rms {rms:.2e}'
    mx = float(np.abs(lg - ref32).max())
    return mx <= TOL, f'max {mx:.2e}'


def _twins(feats, K):
    """The passes of a net: default options, and for K in {1, 31, 32} at width 32 a second one with ``one`` = 0."""
    return (1, 0) if (feats == (32, 32) and K <= 32) else (1,)


def _pin(arch, K, H, W, mode, one):
    """The kernel this (net, input, mode, option) means, with the conditions of the module docstring asserted."""
    kern = _head_kernel(arch, H, W, mode, one)
    if K > 32 or _width0(arch) == 64:
        assert kern == f'head_1x1<{_width0(arch)}>', (K, kern)
    elif one == 1 and W % 32 == 0 and mode != 'exact':
        assert _width0(arch) == 32 and kern == 'head_mfma32', (K, kern)
    else:
        assert kern == 'head_1x1<32>', (K, kern)
    return kern


# ------------------------------------------------------------------------------------------------------------------ a. b.
@pytest.mark.parametrize('feats,K', NETS)
def test_every_layer_and_the_logits(feats, K):
    arch, sd, blob = _net(feats, K)
    worst, failed = {}, []
    with Engine(arch, blob) as e:
        e.set_profiling(True)
        e.keep_activations(True)
        for one in _twins(feats, K):
            e.set_option('one', one)
            for mode in MODES:
                e.set_precision(mode)
                for shape in (WHOLE, HALF, RAGGED):
                    x, ref32, ref16, _ = _ref(feats, K, shape)
                    kern = _pin(arch, K, shape[1], shape[2], mode, one)
                    lg, _ = e.forward(x, logits=True)
                    ran = _ran(e)
                    assert ran['head'][0] == 'head', ran
                    names = [o['name'] for o in arch.program() if o['name'] in ran]
                    assert set(names) == set(ran) and 'head' in names and 'dec0.c0' in names, ran
                    exempt = _f16_exempt(arch, x) if mode == 'f16' else ()
                    assert 'head' not in exempt
                    w = LC.check_layers(e, arch, sd, mode, names, rows=None, x=x, logits=lg, exempt=exempt, memo=MEMO)
                    worst[(kern, mode)] = max(worst.get((kern, mode), 0.0), w['head'])
                    print(f'[many-heads] {feats} K={K} one={one} {mode} {shape} {kern}: ' + ', '.join(f'{n} {v:.2e}' for n, v in w.items()))
                    if shape != HALF:                           # (level 1 of 4 x 32 has 32 pixels per image: per layer only)
                        ok, text = _end_to_end_ok(lg, ref32, ref16, mode)
                        print(f'[many-heads] {feats} K={K} one={one} {mode} {shape} end to end: {text}')
                        if not ok:
                            failed.append((one, mode, shape, text))
            e.set_option('one', 1)
    for kern in sorted({k for k, _ in worst}):
        print(f'[many-heads] head worst {kern} C={_width0(arch)} K={K} {feats}: ' + ' | '.join(f'{worst.get((kern, m), float("nan")):.1e}' for m in MODES))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------ c. d.
@pytest.mark.parametrize('feats,K', NETS)
def test_packed_masks_and_the_independence_of_the_outputs(feats, K):
    arch, sd, blob = _net(feats, K)
    B, H, W = WHOLE
    x, ref32, ref16, ref64 = _ref(feats, K, WHOLE)
    with Engine(arch, blob) as e:
        for one in _twins(feats, K):
            e.set_option('one', one)
            for mode in MODES:
                e.set_precision(mode)
                kern = _pin(arch, K, H, W, mode, one)
                lg, mk = e.forward(x, logits=True, mask=True)
                assert lg.shape == (B, K, H, W) and mk.shape == (B, K, H, W // 32)
                lg1, none = e.forward(x, logits=True, mask=False)
                assert none is None and np.array_equal(lg1.view(np.uint32), lg.view(np.uint32)), (kern, mode, 'logits-only call')
                none, mk1 = e.forward(x, logits=False, mask=True)
                assert none is None and np.array_equal(mk1.view(np.uint32), mk.view(np.uint32)), (kern, mode, 'mask-only call')
                bits = unpack_mask(mk, W)
                assert np.array_equal(bits, (lg > THR).astype(np.uint8)), (kern, mode, 'the predicate on the own logits')
                ref = ref16.astype(np.float64) if mode == 'f16' else ref64
                want = (ref > THR).astype(np.uint8)
                flips, dist = assert_flips_are_tolerance_flips(lg, ref, bits, want)
                err = float(np.abs(lg - ref).max())
                # both values: the reference's own heads first (a property of the case), then the engine's planes on every head whose REFERENCE
                # plane holds both clear of the threshold by the measured error (module docstring, c.)
                both = [k for k in range(K) if (ref[:, k] > THR).any() and not (ref[:, k] > THR).all()]
                assert len(both) == (K - 1 if feats == (40, 48) else K), (kern, mode, sorted(set(range(K)) - set(both)))
                heads = [k for k in both if (ref[:, k] > THR + err).any() and (ref[:, k] < THR - err).any()]
                assert mode == 'f16' or heads == both, (kern, mode, err, sorted(set(both) - set(heads)))
                flat = [k for k in heads if bits[:, k].all() or not bits[:, k].any()]
                assert not flat, (kern, mode, flat)
                print(f'[many-heads] {feats} K={K} one={one} {mode} {kern} masks: {flips} tolerance flips (farthest {dist:.2e}, logit error {err:.2e}), '
                      f'{len(heads)} of {K} heads hold both values')
            e.set_option('one', 1)


# ------------------------------------------------------------------------------------------------------------------ e.
@pytest.mark.parametrize('feats,K', [n for n in NETS if n[1] in (118, 256)])
def test_rows_of_a_batch_equal_those_rows_alone(feats, K):
    arch, _, blob = _net(feats, K)
    with Engine(arch, blob) as e:
        for mode in MODES:
            e.set_precision(mode)
            for shape in (WHOLE, HALF):                            # (4 x 32: the block that holds two images)
                x = _ref(feats, K, shape)[0]
                _pin(arch, K, shape[1], shape[2], mode, 1)
                lg, mk = e.forward(x, logits=True, mask=True)
                for i in (0, 2):
                    xi = np.ascontiguousarray(x[i:i + 1])
                    li, mi = e.forward(xi, logits=True, mask=True)
                    assert np.array_equal(li[0].view(np.uint32), lg[i].view(np.uint32)), (mode, shape, i)
                    assert np.array_equal(mi[0].view(np.uint32), mk[i].view(np.uint32)), (mode, shape, i)


# ------------------------------------------------------------------------------------------------------------------ f.
def test_an_infinite_head_is_an_error_and_the_handle_recovers():
    feats, K = (32, 32), 118
    arch, sd, blob = _net(feats, K)
    x, ref32, ref16, _ = _ref(feats, K, WHOLE)
    bad = dict(sd)
    key = 'decoder.seg_layers.0.bias'
    b = sd[key].copy()
    with np.errstate(over='ignore'):
        b[K - 1] = b[K - 1] * np.float32(1e39)                      # float32 arithmetic: 1e39 is beyond its range, the product is inf
    assert np.isinf(b[K - 1]) and np.isfinite(b[:K - 1]).all()
    bad[key] = b
    with Engine(arch, weights.pack_blob(arch, bad)) as e:
        for mode in ('split', 'f16'):
            e.set_precision(mode)
            with pytest.raises(RuntimeError, match=r'non-finite logits: inf / NaN first appears in the head'):
                e.forward(x, logits=True)                           # host-buffer forward runs ts2d_engine_check itself
        e.load_weights(blob)                                        # the flag does not stick: clean weights, same handle
        for mode in MODES:
            e.set_precision(mode)
            lg, _ = e.forward(x, logits=True)
            ok, text = _end_to_end_ok(lg, ref32, ref16, mode)
            assert ok, (mode, text)


# ------------------------------------------------------------------------------------------------------------------ sliding window, exports
SW_PATCH, SW_STEP, SW_MIRROR = (32, 32), 0.5, (0, 1)


def _sw_net(K):
    return cases.unet(2, (32, 32), K, nconv=1)


def _sw_data(K):
    return prng.normal_f32(300 + K, 999, (2, 1, 40, 52))


@pytest.mark.parametrize('order', ['float', 'half'])
@pytest.mark.parametrize('K', [118, 256])
def test_device_aggregation_is_bit_identical_to_host_aggregation(K, order):
    """tests/test_gpu_predictor.py::test_device_aggregation_is_bit_identical_to_host_aggregation at K heads."""
    arch, data = _sw_net(K), _sw_data(K)
    blobs = [blob_for(arch, 300 + K)[1]]
    dev = HIPnnUNetPredictor(tile_step_size=SW_STEP, use_mirroring=True, tile_dtype=order)
    dev.manual_initialization(arch, blobs, SW_PATCH, inference_allowed_mirroring_axes=SW_MIRROR)
    try:
        engines = dev.engines

        def net(batch, fold):
            return engines[fold].forward(np.ascontiguousarray(batch))[0]
        host = HostLogicPredictor(network=net, tile_step_size=SW_STEP, use_mirroring=True, tile_dtype=order)
        host.manual_initialization(arch, blobs, SW_PATCH, inference_allowed_mirroring_axes=SW_MIRROR)
        a = dev.predict_logits_from_preprocessed_data(data).cpu().numpy()
        b = host.predict_logits_from_preprocessed_data(data).cpu().numpy()
    finally:
        dev.close()
    assert a.dtype == b.dtype == np.float16 and a.shape == (K, 1, 40, 52) and np.array_equal(a, b)
    assert len(np.unique(a.astype(np.float32).argmax(0))) >= 20


@pytest.mark.parametrize('precision', ['split', 'f16'])
@pytest.mark.parametrize('folds', [1, 2])
@pytest.mark.parametrize('K', [118, 256])
def test_labelmap_and_probabilities_entries(K, folds, precision):
    """The label-map entry as tests/test_gpu_labelmap.py::test_engine_entry_equals_the_statement_of_its_own_logits builds it - identity and
    up to (71, 87) as two images of one call - and the probabilities entry (softmax) on the same engines and geometries."""
    arch = _sw_net(K)
    g = sw.compute_gaussian(SW_PATCH)
    img, tiles, rect = _plan(_sw_data(K)[:, 0], SW_PATCH, SW_STEP)
    assert rect == (0, 0, 40, 52)
    outs = [(40, 52), (71, 87)]
    es = _engines(folds, arch=arch, seed0=300 + K, precision=precision, order='half' if precision == 'f16' else 'float')
    try:
        labels, l16 = predict_tiled_labelmap_ensemble(es, [img, img], SW_PATCH, [tiles, tiles], [rect + o for o in outs], SW_MIRROR, g, want_logits=True)
        assert _same16(l16[0], l16[1]) and l16[0].shape == (K, 40, 52)
        counts = []
        for j, out in enumerate(outs):
            want = export.labelmap_statement(l16[j], rect, out)
            assert labels[j].dtype == np.uint8 and labels[j].shape == out and np.array_equal(labels[j], want), (K, folds, precision, out)
            u = np.unique(labels[j])
            counts.append((len(u), int((u >= 32).sum()), int(u.max())))
        print(f'[many-heads] label-map entry K={K} folds={folds} {precision}: (labels, labels >= 32, largest) identity {counts[0]}, (71, 87) {counts[1]}')
        # so that the comparison cannot pass on low labels alone: >= 20 distinct labels >= 32 in the map of the network's own extent (the CPU reference,
        # ``O.predict_logits`` and argmax, gives 30 / 24 at K = 118 and 40 / 53 at K = 256 for one / two folds).  The order-1 resample to (71, 87)
        # smooths single-pixel winners away - the same reference gives 17 / 19 and 21 / 37 there - so that map is held to >= 12, two thirds of
        # the reference's smallest count (room for the 16-bit mode, whose logits differ from the reference's in the third digit).
        assert counts[0][1] >= 20 and counts[1][1] >= 12, counts
        assert es[0].last_tiled_inf is False
        probs, dec, p16 = predict_tiled_probabilities_ensemble(es, [img, img], SW_PATCH, [tiles, tiles], [rect + o + o + (0, 0) for o in outs], 'labelmap',
                                                               mirror_axes=SW_MIRROR, gaussian=g, want_decided=True, want_logits=True)
        for j, out in enumerate(outs):
            assert _same16(p16[j], l16[j])
            assert dec[j].dtype == np.uint8 and np.array_equal(dec[j], labels[j]), (K, folds, precision, out)          # the segmentation bytes of the label-map entry
            _check_probabilities(probs[j], dec[j], l16[j], rect, out, out, (0, 0), 'labelmap', None, f'many heads K={K} folds={folds} {precision} out={out}')
    finally:
        _close(es)
