"""The DEFAULT small-batch dispatch (option "sbk" on, engines created as the product creates them) under per-layer oracles.

``TS2D.predict`` sends 4-8 rows per sub-model through ``ts2d_engine_predict_tiled``; at those batch sizes every level of 32 x 32 pixels
and below runs the one-image kernels with split-K (fp32 partial sums), one of three reduction kernels, and a composed decoder entry as
a stand-alone transposed conv plus a split-K conv over cat(up, skip).  The other GPU modules switch "sbk" off (they address the
full-batch kernels); tests/test_gpu_small_batch.py pins the default end to end.  Here every block that split is compared with ONE
float64 block of the oracle on the engine's OWN inputs (tests/layer_check.py), and every test first asserts - through ``op_kernels()`` /
``op_ksplit()`` - that the path it means was taken, so that a change of the dispatch rule fails loudly instead of testing something else.

What each case is for (slice bounds restated from csrc/kernels_f16x3_one.h:164 / kernels_h32.h:128: kper = ceil(nchunks / S),
slice s = [s * kper, min((s + 1) * kper, nchunks))):
  a. canonical widths, B = 1 / 2 / 4 / 8: S changes with the batch (fill_ksplit), bn = 64, the three reductions by level.
  b. the edge net (32, 64, 288, 544): an EMPTY slice, a RAGGED last slice, a slice that STRADDLES THE SEAM between the two sources of a
     decoder entry, bn = 32, and - on 96 x 160 - the generic reduction; one input channel, a (2, 1) stage, widths that are no multiples of 32.
  c. the hardening cases of tests/test_gpu_hardening.py through fp32 partial sums and the pivot statistics; the overflowing transposed conv.
  d. device aggregation against the host restatement fed in the SAME chunks, bit for bit, more than 64 rows included.
  e. ``debug_tensor('decN.up')`` of a small batch inside a larger reservation with keep_activations on.
  f. a slice alone and in batches of every regime against its "sbk": 0 twin.

Measured worst per-layer values (MI355X, 256 CUs; printed by every case, read them with ``pytest -s``), against the float64 block:
  split mode, a block that split K    9e-7 ... 2.0e-6 absolute on the normalised output (worst: canonical dec4.c0, B = 4, S = 2)
  exact mode (nothing splits)         1.6e-6 ... 3.1e-6 (conv_mfma_f32, widths (16, 48, 80, 100) dec0.c0)
  stand-alone transposed conv         1.4e-7 ... 6.9e-7 of the largest value (split); 16-bit mode 2.0e-4 ... 6.2e-4 (fp16 storage)
  16-bit mode, a block that split K   max 4.1e-5 ... 4.8e-3 (single fp16 flips of stored values), under tests/test_gpu_parity.py's _f16_layer_ok
The bounds of tests/layer_check.py are at most 4x these: 8e-6 (split / exact block), 2e-6 / 2e-3 (transposed conv).  What ran on that
card (kernel, S) is asserted case by case below; e.g. canonical enc5.c1: S = 8 up to B = 4, 4 at B = 8; the edge net at B = 1: enc3.c1
conv3x3_f16x3_one<32> S = 8, enc3.c0 conv3x3s2_f16x3_one S = 8, dec2.c0 S = 8 (16-bit: conv3x3_h32<32> S = 4)."""
import numpy as np
import pytest

from tests import cases
from tests import layer_check as LC
from tests.test_gpu_parity import TOL, F16E_MAX, F16E_RMS, THR, _oracle_mask, blob_for
from tests.test_gpu_hardening import _case, _wide_case, _rel_err
from totalsegmentator2d_amd import prng, weights
from totalsegmentator2d_amd import sliding_window as sw
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.engine import Engine, unpack_mask

pytestmark = pytest.mark.gpu

CHUNK_ROWS = 64          # kSwChunkRows of csrc/device_tables.h (tiled_plan.cpp packs the rows), restated


# ------------------------------------------------------------------------------------------------------------------ helpers
def _ran(e):
    """{op: (kernel, S)} of the last profiled forward, without the statistics launches."""
    k, s = e.op_kernels(), e.op_ksplit()
    assert set(k) == set(s)
    return {n: (k[n], s[n]) for n in k if not n.endswith('.stats')}


def _split(ran):
    return {n: v for n, v in ran.items() if v[1] > 1}


def _targets(ran):
    """What the per-layer checker looks at: every block that split K, every stand-alone transposed conv and the block that reads it."""
    names = []
    for n, (_, S) in ran.items():
        if S > 1 or n.endswith('.up'):
            names.append(n)
        if n.endswith('.up') and n[:-2] + 'c0' not in names:
            names.append(n[:-2] + 'c0')
    return list(dict.fromkeys(names))


def _chunks(arch, name, kern):
    """(chunks of the K loop, chunk index of the seam between the two sources or None) of block `name` served by kernel `kern`, as the
    kernels count them: stride 1 in chunks of 16 channels over cat(up, skip) (csrc/kernels_f16x3_one.h:148, kernels_f16x3.h:327; 32 in
    conv3x3_h32, kernels_h32.h:109), stride 2 in chunks of 8 in every mode (kernels_f16x3_one.h:335, kernels_f16x3.h:589)."""
    kind, lvl, i = name[:3], int(name[3:name.index('.')]), int(name[name.index('.c') + 2:])
    f = [(c + 31) // 32 * 32 for c in arch.features_per_stage]            # (the engine runs a stage rounded up to 32 channels)
    if kind == 'enc' and i == 0:
        return f[lvl - 1] // 8, None
    ck = 32 if kern.startswith('conv3x3_h32') else 16
    if kind == 'dec' and i == 0:
        return 2 * f[lvl] // ck, f[lvl] // ck
    return f[lvl] // ck, None


def _slices(nchunks, S):
    kper = -(-nchunks // S)
    return [(s * kper, min((s + 1) * kper, nchunks)) for s in range(S)]


def _reduction(HW):
    """Which of the three reduction forms serves a split block of HW pixels (csrc/engine.hip, behind the conv launch)."""
    return 'stats32' if HW == 256 else ('part' if HW % 256 == 0 else 'generic')


def _forward_kept(arch, blob, x, mode, **kw):
    e = Engine(arch, blob)
    e.set_profiling(True)
    e.keep_activations(True)
    e.set_precision(mode)
    out = e.forward(x, logits=True, mask=kw.get('mask', False))
    return e, out


def _report(tag, ran, worst):
    print(f'[default-dispatch] {tag}: ' + ', '.join(f'{n} {ran[n][0]} S={ran[n][1]} {worst[n]:.2e}' for n in worst))


SEEN = {}            # (mode, property) -> ops: filled by the cases, read by test_every_split_k_form_was_seen (runs last in this module)


def _note(arch, ran, mode, H, W):
    storage = 'half' if mode == 'f16' else 'float'
    for n, (kern, S) in ran.items():
        if n.endswith('.up'):
            SEEN.setdefault((storage, 'convT'), []).append(n)
            continue
        if S == 1:
            continue
        lvl = int(n[3:n.index('.')])
        sy = int(np.prod([s[0] for s in arch.strides[:lvl + 1]])); sx = int(np.prod([s[1] for s in arch.strides[:lvl + 1]]))
        kind = 'entry' if (n.startswith('dec') and n.endswith('.c0')) else ('s2' if (n.startswith('enc') and n.endswith('.c0')) else 's1')
        nch, seam = _chunks(arch, n, kern)
        sl = _slices(nch, S)
        for key in (f'S{S}', kind, f'S{S}/{kind}', 'bn64' if '<64>' in kern else ('bn32' if '<32>' in kern else 'bn?'),
                    _reduction((H // sy) * (W // sx))):
            SEEN.setdefault((storage, key), []).append(n)
        if any(b >= e_ for b, e_ in sl):
            SEEN.setdefault((storage, 'empty'), []).append(n)
        if any(0 < e_ - b < sl[0][1] - sl[0][0] for b, e_ in sl):
            SEEN.setdefault((storage, 'ragged'), []).append(n)
        if seam is not None and any(b < seam < e_ for b, e_ in sl):
            SEEN.setdefault((storage, 'seam'), []).append(n)


def _check_case(tag, arch, sd, blob, x, mode, want=None, rows=(0,)):
    """Forward under the default dispatch with kept activations; `want`: {op: (kernel, S)} that must have run (None entries: any);
    every split block and un-composed entry under the per-layer oracle.  Returns (ran, logits, mask)."""
    e, (lg, mk) = _forward_kept(arch, blob, x, mode, mask=x.shape[-1] % 32 == 0)
    with e:
        ran = _ran(e)
        for n, v in (want or {}).items():
            assert n in ran and (v is None or ran[n] == v), (tag, mode, n, v, {k: ran[k] for k in ran if ran[k][1] > 1 or k.endswith('.up')})
        names = _targets(ran)
        worst = LC.check_layers(e, arch, sd, mode, names, rows=rows)
        _report(f'{tag} B={x.shape[0]} {x.shape[2]}x{x.shape[3]} {mode}', ran, worst)
        _note(arch, ran, mode, x.shape[2], x.shape[3])
    return ran, lg, mk


# ------------------------------------------------------------------------------------------------------------------ a. canonical net
@pytest.mark.parametrize('B', [1, 2, 4, 8])
def test_canonical_net_every_split_block_under_the_layer_oracle(B):
    arch = UNetArch.canonical()
    sd, blob = blob_for(arch, 1)
    x = cases.make_input(arch, B, 512, 512, 7)
    for mode in ('split', 'f16'):
        one, s2 = ('conv3x3_f16x3_one<64>', 'conv3x3s2_f16x3_one') if mode == 'split' else ('conv3x3_h32<64>', None)
        ran, lg, mk = _check_case('canonical', arch, sd, blob, x, mode, want={'dec5.up': None, 'dec5.c0': None, 'enc5.c1': None})
        sp = _split(ran)
        # the deepest level (16 x 16) always splits on the one-image kernels; its entry runs un-composed on a split-K conv
        assert ran['enc5.c1'][0] == one and ran['enc5.c1'][1] > 1 and ran['dec5.c0'][0] == one and ran['dec5.c0'][1] > 1, sp
        if s2:
            assert ran['enc5.c0'][0] == s2 and ran['enc5.c0'][1] > 1, sp
        assert ran['enc1.c1'][1] == 1 and ran['dec0.c0'] == ('conv3x3_up0', 1)               # the big levels are untouched
        if B == 1:
            assert {'dec4.up', 'dec4.c0', 'enc4.c1'} <= set(ran) and ran['enc4.c1'][1] > 1, sp
        # fill_ksplit: the factor of ONE layer falls as the batch grows (256 CUs: 8 up to B = 4, 4 at B = 8)
        if mode == 'split':
            assert ran['enc5.c1'][1] == (8 if B <= 4 else 4), (B, ran['enc5.c1'])
        assert np.array_equal(unpack_mask(mk, 512), _oracle_mask(lg))
        SEEN.setdefault(('any', f'canonical B={B} {mode}'), []).append(sorted((n, v[1]) for n, v in sp.items()))


# ------------------------------------------------------------------------------------------------------------------ b. a net built for the edges
EDGE = dict(n_stages=4, feats=(32, 64, 288, 544), K=5)


def _edge():
    arch = cases.unet(EDGE['n_stages'], EDGE['feats'], EDGE['K'])
    sd, blob = blob_for(arch, 81)
    return arch, sd, blob


def test_edge_net_empty_ragged_and_seam_straddling_slices():
    """128 x 128, B = 1.  Split mode (chunks of 16): enc3.c1 544 -> 544 on 16 x 16 has 34 chunks, S = 8, kper = 5: slice 7 starts at 35 >= 34
    and is EMPTY (it must write zeros, not nothing); bn = 32 (544 = 17 x 32); HW = 256 reduction.  enc3.c0 (stride 2, 36 chunks of 8):
    the last slice holds one chunk.  dec2.c0 over cat(288, 288) on 32 x 32: 36 chunks, seam at 18, slice 3 = [15, 20) straddles it; the
    last slice is [35, 36); HW = 1024: splitk_reduce_part + finalize.  16-bit mode: 17 / 18 chunks of 32, S = 4, kper = 5 - ragged last
    slice, seam at 9 inside [5, 10).  Exact mode: nothing splits, nothing is un-composed that was not already."""
    arch, sd, blob = _edge()
    x = cases.make_input(arch, 1, 128, 128, 81)
    ran, lg, mk = _check_case('edge', arch, sd, blob, x, 'split', want={
        'enc3.c1': ('conv3x3_f16x3_one<32>', 8), 'enc3.c0': ('conv3x3s2_f16x3_one', 8), 'dec2.c0': ('conv3x3_f16x3_one<32>', 8), 'dec2.up': None})
    assert _slices(_chunks(arch, 'enc3.c1', ran['enc3.c1'][0])[0], 8)[7] == (35, 34)         # empty
    assert _slices(_chunks(arch, 'enc3.c0', ran['enc3.c0'][0])[0], 8)[7] == (35, 36)          # one chunk
    assert _chunks(arch, 'dec2.c0', ran['dec2.c0'][0]) == (36, 18) and _slices(36, 8)[3] == (15, 20)    # the seam inside a slice
    from oracle import torch_oracle as O
    ref = O.unet_forward(arch, sd, x).numpy()
    assert np.abs(lg - ref).max() <= TOL
    assert np.array_equal(unpack_mask(mk, 128), _oracle_mask(lg))
    ran16, lh, mh = _check_case('edge', arch, sd, blob, x, 'f16', want={
        'enc3.c1': ('conv3x3_h32<32>', 4), 'dec2.c0': ('conv3x3_h32<32>', 4), 'dec2.up': None})
    assert _slices(17, 4)[3] == (15, 17) and _chunks(arch, 'dec2.c0', ran16['dec2.c0'][0]) == (18, 9) and _slices(18, 4)[1] == (5, 10)
    d = lh - O.unet_forward(arch, sd, x, emulate='f16').numpy()
    assert np.abs(d).max() <= F16E_MAX and np.sqrt((d ** 2).mean()) <= F16E_RMS
    assert np.array_equal(unpack_mask(mh, 128), _oracle_mask(lh))
    e, (le, _) = _forward_kept(arch, blob, x, 'exact')
    with e:
        rx = _ran(e)
        assert not _split(rx) and all(v[0] in ('conv_mfma_f32', 'convT_mfma_f32', 'head', 'conv3x3_first') for v in rx.values()), rx
        assert np.abs(le - ref).max() <= TOL


@pytest.mark.parametrize('B,H,W', [(1, 96, 160), (2, 128, 128), (3, 128, 128), (2, 96, 160)])
def test_edge_net_other_batches_and_the_generic_reduction(B, H, W):
    """The same net where the split factor differs (B = 2, 3) and on 96 x 160, whose deep levels (12 x 20, 24 x 40) are no multiples of
    256 pixels: the generic reduction (one block per image walks the pixels) in float and in half storage."""
    arch, sd, blob = _edge()
    x = cases.make_input(arch, B, H, W, 82)
    from oracle import torch_oracle as O
    ref = O.unet_forward(arch, sd, x).numpy()
    for mode in ('split', 'f16'):
        ran, lg, _ = _check_case('edge', arch, sd, blob, x, mode, rows=(0, B - 1))
        sp = _split(ran)
        assert len(sp) >= 2 and any(n.endswith('.up') for n in ran), (mode, ran)
        if H == 96:
            assert all(_reduction((H >> int(n[3])) * (W >> int(n[3]))) == 'generic' for n in sp if int(n[3]) >= 2), sp
        if mode == 'split':
            assert np.abs(lg - ref).max() <= TOL


def test_one_input_channel_and_a_per_axis_stage_beside_split_k_levels():
    from oracle import torch_oracle as O
    arch, _, H, W, seed = cases.SMALL_CASES['xr_1ch']
    sd, blob = blob_for(arch, seed)
    x = cases.make_input(arch, 1, H, W, seed)
    for mode in ('split', 'f16'):
        ran, lg, _ = _check_case('xr_1ch', arch, sd, blob, x, mode)
        assert _split(ran), (mode, ran)
    arch, _, H, W, seed = cases.SMALL_CASES['aniso_21']
    sd, blob = blob_for(arch, seed)
    x = cases.make_input(arch, 1, 2 * H, 2 * W, seed)                   # 64 x 128: levels 32 x 64, 16 x 32, 8 x 32
    ref = O.unet_forward(arch, sd, x).numpy()
    ran, lg, _ = _check_case('aniso_21', arch, sd, blob, x, 'split')
    assert ran['enc3.c0'] == ('conv_mfma_f32', 1), ran                  # the (2, 1) stage: the exact kernel, never split
    assert any(int(n[3]) in (2, 3) for n in _split(ran)), ran           # ... with split-K on its neighbours
    assert np.abs(lg - ref).max() <= TOL


@pytest.mark.parametrize('feats,strides', [((24, 40, 72), None), ((16, 48, 80, 100), [(1, 1), (2, 2), (2, 2), (2, 1)]), ((40, 40), None)])
def test_stage_widths_that_are_not_multiples_of_32_at_b1(feats, strides):
    """tests/test_gpu_parity.py::test_stage_widths_that_are_not_multiples_of_32's nets at B = 1 under the default dispatch, same bound."""
    from oracle import torch_oracle as O
    arch = cases.unet(len(feats), feats, 5, cin=2, nconv=2, strides=strides)
    sd, blob = blob_for(arch, 77)
    dy, dx = arch.divisors
    H, W = 8 * dy, 32 * dx
    x = cases.make_input(arch, 1, H, W, 77)
    ref = O.unet_forward(arch, sd, x).numpy()
    for mode in ('split', 'exact'):
        ran, lg, mk = _check_case(f'widths{feats}', arch, sd, blob, x, mode)
        assert np.abs(lg - ref).max() <= TOL, mode
        assert np.array_equal(unpack_mask(mk, W), _oracle_mask(lg))


# ------------------------------------------------------------------------------------------------------------------ c. hardening
def _hardened(which):
    if which == 'gains':
        arch, sd, x = _case()
        return arch, {k: (v * np.float32(100.0) if k.endswith('norm.weight') else v) for k, v in sd.items()}, x
    if which == 'binades':
        arch, sd, x = _case()
        rng = np.random.default_rng(0)
        sd = dict(sd)
        for k in list(sd):
            if k.endswith('conv.weight') and sd[k].ndim == 4 and sd[k].shape[1] >= 32:
                sd[k] = sd[k] * np.exp2(-rng.integers(0, 21, size=sd[k].shape)).astype(np.float32)
        return arch, sd, x
    if which == 'biases':
        arch, sd, x = _wide_case()
        return arch, {k: (v * np.float32(1000.0) if k.endswith('conv.bias') else v) for k, v in sd.items()}, x
    arch, sd, x = _wide_case()
    return arch, sd, (x + np.float32(50.0)).astype(np.float32)


@pytest.mark.parametrize('which', ['gains', 'binades', 'biases', 'offset'])
def test_hardening_cases_through_partial_sums_and_pivot_statistics(which):
    """The numeric cases of tests/test_gpu_hardening.py at B = 1 with default options: large gains, weights over twenty binades, conv biases
    x 1000 and an input 50 sigma off zero now pass through bias-free fp32 partial sums, a reduction that adds the bias, and shifted sums
    around a pivot.  Same bounds; at least two blocks split."""
    from oracle import torch_oracle as O
    arch, sd, x = _hardened(which)
    x = np.ascontiguousarray(x[:1])
    ref = O.unet_forward(arch, sd, x).numpy()
    with Engine(arch, weights.pack_blob(arch, sd)) as e:
        e.set_profiling(True)
        lg, _ = e.forward(x)
        sp = _split(_ran(e))
        assert len(sp) >= 2, sp
        assert np.isfinite(lg).all() and _rel_err(lg, ref) <= 1e-4, (which, sorted(sp), _rel_err(lg, ref))


def test_overflowing_stand_alone_transposed_conv_is_named():
    """B = 1, default options: dec1.up (32 x 32) runs UN-composed, its un-normalised output beyond 65504 becomes inf as an fp16 operand of
    dec1.c0.  The error names dec1.up or dec1.c0 - on an engine of its own and inside a workspace reserved for a larger batch (where the
    upsampled tensor used to live in the shared scratch region, which the diagnosis skips) - never finite-but-wrong logits, never "the head"."""
    arch, sd, x = _case()
    x = np.ascontiguousarray(x[:1])
    sd = dict(sd)
    sd['decoder.transpconvs.1.weight'] = sd['decoder.transpconvs.1.weight'] * np.float32(3e5)
    blob = weights.pack_blob(arch, sd)
    for reserve in (None, 16):
        with Engine(arch, blob) as e:
            e.set_profiling(True)
            if reserve:
                e.reserve(reserve, 64, 64)
            with pytest.raises(RuntimeError, match=r'non-finite logits: inf / NaN first appears in layer dec1\.(up|c0)') as ei:
                e.forward(x)
            assert 'the head' not in str(ei.value)
            assert 'dec1.up' in e.op_kernels(), sorted(e.op_kernels())         # the path under test: the stand-alone transposed conv


# ------------------------------------------------------------------------------------------------------------------ d. sliding window
def _chunked_network(engines, rows_per_image):
    """The network of the host restatement, called as ``predict_tiled_impl`` (csrc/tiled.hip) calls it for ONE image per call: the rows of
    an image (tile-major, mirror variants inside) in chunks of at most kSwChunkRows = 64, in row order, each chunk one forward."""
    def net(batch, fold):
        out = []
        for i0 in range(0, batch.shape[0], rows_per_image):
            img = batch[i0:i0 + rows_per_image]
            for r0 in range(0, img.shape[0], CHUNK_ROWS):
                out.append(engines[fold].forward(np.ascontiguousarray(img[r0:r0 + CHUNK_ROWS]))[0])
        return np.concatenate(out, 0)
    return net


def _device_vs_host(arch, blobs, data, patch, step, mirror, order):
    from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor
    from tests.host_predictor import HostLogicPredictor
    padded, _ = sw.pad_nd_image(np.asarray(data, np.float32), patch)
    Z = padded.shape[1]
    rows = len(sw.tile_slicers(padded.shape[2:], patch, step, Z)) // Z * len(sw.mirror_combos(mirror))
    dev = HIPnnUNetPredictor(tile_step_size=step, use_mirroring=mirror is not None, tile_dtype=order)
    dev.manual_initialization(arch, blobs, patch, inference_allowed_mirroring_axes=mirror)
    try:
        host = HostLogicPredictor(network=_chunked_network(dev.engines, rows), tile_step_size=step, use_mirroring=mirror is not None, tile_dtype=order)
        host.manual_initialization(arch, blobs, patch, inference_allowed_mirroring_axes=mirror)
        a = dev.predict_logits_from_preprocessed_data(data).cpu().numpy()
        b = host.predict_logits_from_preprocessed_data(data).cpu().numpy()
    finally:
        dev.close()
    assert a.dtype == b.dtype == np.float16 and np.array_equal(a, b), (rows, order, int((a != b).sum()))
    return rows


@pytest.mark.parametrize('order', ['float', 'half'])
@pytest.mark.parametrize('name', list(cases.SW_CASES))
def test_device_aggregation_equals_the_host_restatement_under_the_default_dispatch(name, order):
    arch, shape, patch, step, mirror, folds, seed = cases.SW_CASES[name]
    blobs = [blob_for(arch, seed + f)[1] for f in range(folds)]
    data = prng.normal_f32(seed, 999, (arch.input_channels,) + tuple(shape))
    _device_vs_host(arch, blobs, data, patch, step, mirror, order)


@pytest.mark.parametrize('order', ['float', 'half'])
def test_more_than_64_rows_the_tail_chunk_takes_the_small_batch_plan(order):
    """17 tiles x 4 mirror variants = 68 rows of one image: a chunk of 64 (full-size plan) and a tail of 4 that runs the small-batch plan
    (split-K, un-composed entries into the scratch region) INSIDE the workspace laid out for 64, within one call."""
    arch = cases.unet(4, (32, 64, 128, 256), 3)
    _, blob = blob_for(arch, 91)
    patch, step = (64, 64), 0.5
    data = prng.normal_f32(91, 999, (2, 1, 64, 64 + 16 * 32))           # 1 x 17 tiles at step 32
    rows = _device_vs_host(arch, [blob], data, patch, step, (0, 1), order)
    assert CHUNK_ROWS < rows <= CHUNK_ROWS + 8, rows
    x = cases.make_input(arch, CHUNK_ROWS, 64, 64, 3)
    with Engine(arch, blob) as e:                                         # what the two chunk sizes run, on the same engine in the same order
        e.set_profiling(True)
        e.forward(x)
        big = _ran(e)
        e.forward(np.ascontiguousarray(x[:rows - CHUNK_ROWS]))
        tail = _ran(e)
    assert _split(tail) != _split(big) and any(n.endswith('.up') for n in set(tail) - set(big)), (_split(big), _split(tail))


def test_canonical_sample_case_under_the_default_dispatch_bit_for_bit():
    """BASELINE config 1 (sample_s0616: 2 tiles x 4 mirror variants = 8 rows, the product's headline call)."""
    import os
    from tests.conftest import GOLDEN
    from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor
    arch = UNetArch.canonical()
    _, blob = blob_for(arch, 1)
    p = HIPnnUNetPredictor()
    p.manual_initialization(arch, [blob], (512, 512))
    try:
        pre = p.configuration_manager.preprocessor_class(verbose=False)
        data, _, _ = pre.run_case([os.path.join(GOLDEN, 'assets', 'sample_s0616.nrrd')], None, p.plans_manager, p.configuration_manager, p.dataset_json)
    finally:
        p.close()
    assert _device_vs_host(arch, [blob], data, (512, 512), 0.5, (0, 1), 'float') == 8


# ------------------------------------------------------------------------------------------------------------------ e. keep_activations
@pytest.mark.parametrize('mode', ['split', 'f16'])
def test_kept_activations_of_a_small_batch_inside_a_large_reservation(mode):
    """reserve(64), keep_activations on, forward at B = 1 (at 16 rows only dec1 is composed, the deeper entries still split K): every decL.up that ran un-composed has a buffer of its own (the reserved batch's
    plan composes those entries and holds none; they used to share ONE scratch region and debug_tensor told the caller to switch on what
    was on) and reads back as the transposed conv of the engine's own coarse tensor."""
    arch = cases.unet(5, (32, 64, 128, 256, 512), 6)
    sd, blob = blob_for(arch, 62)
    x = cases.make_input(arch, 64, 128, 128, 62)
    with Engine(arch, blob) as e, Engine(arch, blob) as e1:
        e.set_profiling(True); e1.set_profiling(True)
        e.set_precision(mode); e1.set_precision(mode)
        e.keep_activations(True)
        e.reserve(64, 128, 128)
        big, _ = e.forward(x)
        composed = [n for n in ('dec3.up', 'dec2.up', 'dec1.up') if n not in e.op_kernels()]
        one, _ = e.forward(np.ascontiguousarray(x[3:4]))
        ran = _ran(e)
        ups = [n for n in composed if n in ran]
        assert len(ups) >= 2, (composed, sorted(ran))                     # the path under test: un-composed at B = 1, composed at 64
        worst = LC.check_layers(e, arch, sd, mode, _targets(ran))
        _report(f'kept B=1 in 64 {mode}', ran, worst)
        assert set(ups) <= set(worst)
        fresh, _ = e1.forward(np.ascontiguousarray(x[3:4]))
        assert np.array_equal(one, fresh)                                 # where the tensors live does not change a bit
        again, _ = e.forward(x)
        assert np.array_equal(again, big)
        with pytest.raises(RuntimeError, match='not materialised'):       # at the reserved batch the entry is composed: said so, as before
            e.debug_tensor(ups[0])


# ------------------------------------------------------------------------------------------------------------------ f. across regimes
def test_a_slice_in_batches_of_every_regime_against_its_sbk0_twin():
    arch = cases.unet(5, (32, 64, 128, 256, 512), 6)
    _, blob = blob_for(arch, 62)
    x = cases.make_input(arch, 32, 128, 128, 62)
    tables = {}
    with Engine(arch, blob) as e, Engine(arch, blob, options={'sbk': 0}) as e0:
        e.set_profiling(True)
        for B in (1, 2, 3, 4, 5, 8, 16, 32):
            xb = np.ascontiguousarray(x[:B])
            lg, mk = e.forward(xb, logits=True, mask=True)
            tables[B] = tuple(sorted((n, v[1]) for n, v in _split(_ran(e)).items()))
            lg0, mk0 = e0.forward(xb, logits=True, mask=True)
            assert np.abs(lg - lg0).max() <= 3e-5, B
            flips = unpack_mask(mk[:1], 128)[0] != unpack_mask(mk0[:1], 128)[0]
            assert (np.abs(lg0[0][flips].astype(np.float64) - THR) <= 3e-5).all(), (B, int(flips.sum()))
            lg2, mk2 = e.forward(xb, logits=True, mask=True)
            assert np.array_equal(lg, lg2) and np.array_equal(mk, mk2), B
    assert tables[1] and len(set(tables.values())) >= 3, tables            # several regimes really ran (S changes with B)


# ------------------------------------------------------------------------------------------------------------------ coverage of the forms
def test_every_split_k_form_was_seen():
    """Runs last: what the cases above drove under the per-layer oracle, from op_kernels() / op_ksplit() - S in {2, 4, 8}; bn 32 and 64;
    stride-1, stride-2 and decoder-entry split-K; a seam inside a slice, a ragged and an empty slice; each of the three reductions in
    float and in half storage; the stand-alone transposed conv in both precisions."""
    if not SEEN:
        pytest.skip('the cases of this module did not run in this session')
    missing = []
    for storage in ('float', 'half'):
        for key in ('stats32', 'part', 'generic', 'convT', 'bn32', 'bn64', 's1', 'entry', 'ragged', 'seam'):
            if not SEEN.get((storage, key)):
                missing.append((storage, key))
    for key in ('S2', 'S4', 'S8', 's2', 'empty'):
        if not (SEEN.get(('float', key)) or SEEN.get(('half', key))):
            missing.append(key)
    for kind in ('s1', 's2', 'entry'):
        if not any(SEEN.get(('float', f'S{S}/{kind}')) for S in (2, 4, 8)):
            missing.append(kind)
    assert not missing, (missing, {k: sorted(set(map(str, v))) for k, v in SEEN.items()})
