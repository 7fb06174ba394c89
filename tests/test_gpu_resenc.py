"""ResidualEncoderUNet on the device: the residual blocks (res_join, pool_proj1x1 - csrc/kernels_resblock.h) around the engine's ordinary
3x3 kernels, against the float32 torch restatement of tests/resenc_util.py, per layer against float64 blocks fed with the engine's own
inputs, on both sides of the dispatch options, through the sliding window and through a model folder.

Yardsticks: the logits within max(1e-4, 2 E), E = the float32 oracle's own error against its float64 evaluation of the same case (1e-4:
tests/test_gpu_parity.py TOL); per layer max(SPLIT_LAYER_TOL, 2 E_op) and a join element-wise within 4 * 2^-23 * max(1, |c2|, |r|) of
lrelu(c2 + r) on the values the accessor shows - both rules live in tests/layer_check.py (its module docstring; E_op < 5e-6 on every case,
so SPLIT_LAYER_TOL is the bound everywhere); tests/test_gpu_resenc_layers.py applies them to every op of both dispatches.

Measured on an MI355X (worst over the first seven cases; bound in brackets):
  logits vs the float32 oracle      split 1.0e-5, exact 6.9e-6   [1e-4; 2 E <= 1.8e-5 everywhere, so 1e-4 is the bound of every case]
  stem / .c1 (activated)            split 3.3e-6, exact 2.8e-6   [8e-6]
  .c2 (not activated)               split 3.2e-6, exact 3.1e-6   [8e-6]
  .proj (not activated)             split 5.6e-6, exact 6.6e-6   [8e-6]   (res_deep: the fp32 chain of a 128- / 256-channel contraction)
  join, in units of its bound       split 0.50,   exact 0.50     [1]
  model folder through the predictor: 9.8e-4 on the aggregated float16 logits [1.6e-2], 0.29 % of the oracle's logits inside the band
8e-6 holds for .c2 and .proj as they are: no bound was widened."""
import numpy as np
import pytest

from tests import resenc_util as R
from tests.conftest import blob_for
from tests import layer_check as LC
from tests.layer_check import SPLIT_LAYER_TOL
from totalsegmentator2d_amd import prng
from totalsegmentator2d_amd import sliding_window as sw
from totalsegmentator2d_amd.engine import Engine
from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

TOL = 1e-4                      # tests/test_gpu_parity.py
SW_TOL = 1.6e-2                 # the sliding-window goldens' tolerance: 2 half-ulps at |x| <= 8 (tests/test_gpu_predictor.py)
MODES = ('split', 'exact')


def _engine(name, mode='split', options=None):
    arch, B, H, W, seed = R.RES_CASES[name]
    e = Engine(arch, blob_for(arch, seed)[1], options=options)
    e.set_precision(mode)
    return e


def _parity(name, e, rows=None, what=''):
    want, E = R.oracle_logits(name)
    x = R.case_input(name)
    if rows is not None:
        x, want = np.ascontiguousarray(x[rows]), want[rows]
    got = e.forward(x)[0]
    err = float(np.abs(got - want).max())
    print(f'{name} {what}: max |logits - float32 oracle| {err:.3e}  (E {E:.3e}, bound {max(TOL, 2 * E):.3e})')
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= max(TOL, 2 * E), (name, what, err, E)
    return x, got


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(R.RES_CASES))
def test_logits_match_the_float32_restatement(name, mode):
    with _engine(name, mode) as e:
        e.set_profiling(True)
        _parity(name, e, what=mode)
        kern = e.op_kernels()
    arch = R.RES_CASES[name][0]
    for o in arch.program():
        if o['name'].endswith('.proj'):
            assert kern[o['name']] == 'pool_proj1x1', kern
        if o['op'] == 4:
            assert kern[o['name']] == 'res_join', kern


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(R.RES_CASES))
def test_every_tensor_of_the_encoder_against_a_float64_block_on_the_engines_own_inputs(name, mode):
    """The stem, conv1, conv2, the projection and the join of every block through tests/layer_check.py (the residual rules of its module
    docstring; tests/test_gpu_resenc_layers.py carries on through the decoder and the head, under both dispatches)."""
    arch, B, H, W, seed = R.RES_CASES[name]
    sd = blob_for(arch, seed)[0]
    x = R.case_input(name)
    names = [o['name'] for o in arch.program() if o['name'] == 'stem' or o['name'].startswith('enc')]
    e_ops = {}
    with _engine(name, mode) as e:
        e.keep_activations(True)
        e.forward(x)
        assert e.materialised('stem')                                   # the fused first block is off: the first join reads the stem's output
        got = LC.check_layers(e, arch, sd, mode, names, x=x, e_ops=e_ops)
    assert set(got) == set(names)
    kind = lambda n: 'join' if n not in e_ops else (n.rsplit('.', 1)[1] if n.endswith(('.c2', '.proj')) else 'act')
    worst = {k: max([v for n, v in got.items() if kind(n) == k], default=0.0) for k in ('act', 'c2', 'proj', 'join')}
    print(f'{name} {mode}: worst stem / c1 {worst["act"]:.3e}  c2 {worst["c2"]:.3e}  proj {worst["proj"]:.3e}  (bound {SPLIT_LAYER_TOL:.0e}; '
          f'worst E_op {max(e_ops.values()):.2e});  join {worst["join"]:.3f} of its bound')


@pytest.mark.parametrize('sbk', [1, 0])
@pytest.mark.parametrize('name', ['res_min', 'res_deep'])
def test_one_slice_on_both_sides_of_the_small_batch_dispatch(name, sbk):
    with _engine(name, options={'sbk': sbk}) as e:
        _parity(name, e, rows=[0], what=f'B = 1 sbk = {sbk}')


@pytest.mark.parametrize('upc', [1, 0])
def test_the_decoder_reads_join_outputs_composed_and_as_two_kernels(upc):
    with _engine('res_deep', options={'upc': upc, 'sbk': 0}) as e:
        e.set_profiling(True)
        _parity('res_deep', e, what=f'upc = {upc}')
        kern = e.op_kernels()
    assert ('dec0.up' in kern) == (upc == 0), kern                       # composed: the upsampled tensor has no launch of its own


def _plan(data, patch, step):
    padded, _ = sw.pad_nd_image(np.asarray(data, np.float32), patch)
    Z, H, W = padded.shape[1:]
    slicers = sw.tile_slicers((H, W), patch, step, Z)
    return [np.ascontiguousarray(padded[:, d]) for d in range(Z)], [[(y, x) for (dd, y, x) in slicers if dd == d] for d in range(Z)]


def test_a_rows_bytes_do_not_depend_on_its_batch_mates():
    arch, _, _, _, seed = R.RES_CASES['res_min']
    blob = blob_for(arch, seed)[1]
    patch, g = (64, 64), sw.compute_gaussian((64, 64))
    imgs, tiles = zip(*[(lambda p: (p[0][0], p[1][0]))(_plan(prng.normal_f32(seed + i, 999, (2, 1, 80, 52)), patch, 0.5)) for i in range(3)])
    with Engine(arch, blob) as e, Engine(arch, blob, options={'sbk': 0}) as old:
        alone = e.predict_tiled_batch([imgs[0]], patch, [tiles[0]], (0, 1), g)[0][0].copy()
        first = e.predict_tiled_batch(list(imgs), patch, list(tiles), (0, 1), g)[0][0].copy()
        order = [1, 2, 0]
        last = e.predict_tiled_batch([imgs[i] for i in order], patch, [tiles[i] for i in order], (0, 1), g)[0][2].copy()
        single = old.predict_tiled(imgs[0], patch, tiles[0], (0, 1), g)[0]
    assert alone.dtype == np.float16 and np.isfinite(alone.astype(np.float32)).all()
    for other in (first, last, single):
        assert np.array_equal(alone.view(np.uint16), other.view(np.uint16))


SURFACE_SEED = 74                # (chosen on the CPU from the oracle alone, seeds 40 ... 99: 0.3 % of its logits lie inside the band)


def test_a_model_folder_runs_through_the_predictor(tmp_path):
    """A synthetic ResEnc model folder -> HIPnnUNetPredictor -> aggregated float16 logits of an 80 x 52 image (64 x 64 patch, step 0.5, both
    mirror axes) against oracle.torch_oracle.predict_sliding_window around resenc_forward."""
    from oracle import torch_oracle as O
    from totalsegmentator2d_amd import weights
    arch = R.RES_CASES['res_min'][0]
    patch = (64, 64)
    R.write_model_folder(str(tmp_path), arch, SURFACE_SEED, patch)
    sd = weights.synthetic_state_dict(arch, SURFACE_SEED)
    data = prng.normal_f32(SURFACE_SEED, 999, (arch.input_channels, 1, 80, 52))
    ref = O.predict_sliding_window(lambda x: R.resenc_forward(arch, sd, x), torch.from_numpy(data), patch, 0.5, (0, 1)).numpy()
    inside = np.abs(ref.astype(np.float32)) <= SW_TOL
    assert inside.mean() < 0.01, inside.mean()                            # the oracle alone: fewer than 1 % of the logits lie inside the band
    p = HIPnnUNetPredictor(tile_step_size=0.5, use_mirroring=True)
    p.initialize_from_trained_model_folder(str(tmp_path), (0,), 'checkpoint_final.pth')
    try:
        assert p.arch == arch
        got = p.predict_logits_from_preprocessed_data(data).cpu().numpy()
        images, tiles = _plan(data, patch, 0.5)
        seg = p.engines[0].predict_tiled_batch(images, patch, tiles, (0, 1), sw.compute_gaussian(patch), want_logits=False, want_seg=True)[1][0]
    finally:
        p.close()
    assert got.shape == ref.shape and got.dtype == np.float16
    err = float(np.abs(got.astype(np.float32) - ref.astype(np.float32)).max())
    print(f'surface: max |logits - oracle| {err:.3e} (bound {SW_TOL}), {inside.mean():.4%} of the logits inside the band')
    assert err <= SW_TOL
    off = (seg.shape[2] - ref.shape[3]) // 2                              # (the image is padded to the patch along W, symmetrically)
    seg = seg[:, :ref.shape[2], off:off + ref.shape[3]]
    want_seg = O.logits_to_mask(torch.from_numpy(ref)).numpy()[:, 0]
    cmp = ~inside[:, 0]
    assert cmp.mean() >= 0.99 and np.array_equal(seg[cmp], want_seg[cmp])


def test_the_16_bit_mode_is_refused_and_the_engine_keeps_running():
    with _engine('res_min') as e:
        with pytest.raises(RuntimeError, match=r'\(-1\).*TS2D_PRECISION_F16'):
            e.set_precision('f16')
        _parity('res_min', e, what='split after the refusal')
