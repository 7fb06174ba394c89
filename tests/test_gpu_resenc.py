"""ResidualEncoderUNet on the device: the residual blocks (res_join, pool_proj1x1 - csrc/kernels_resblock.h) around the engine's ordinary
3x3 kernels, against the float32 torch restatement of tests/resenc_util.py, per layer against float64 blocks fed with the engine's own
inputs, on both sides of the dispatch options, through the sliding window and through a model folder.

Yardsticks: the logits within max(1e-4, 2 E), E = the float32 oracle's own error against its float64 evaluation of the same case (1e-4:
tests/test_gpu_parity.py TOL); per layer SPLIT_LAYER_TOL (tests/layer_check.py); a join element-wise within 4 * 2^-23 * max(1, |c2|, |r|) of
lrelu(c2 + r) on the values the accessor shows (one unit for each input's accessor rounding against the kernel's fused form, one for the
sum, one for the slope product: derived, not measured).

Measured on an MI355X (worst over the seven cases; bound in brackets):
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


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(R.RES_CASES))
def test_every_tensor_of_the_encoder_against_a_float64_block_on_the_engines_own_inputs(name, mode):
    arch, B, H, W, seed = R.RES_CASES[name]
    sd = blob_for(arch, seed)[0]
    x = R.case_input(name)
    worst = {'act': 0.0, 'c2': 0.0, 'proj': 0.0, 'join': 0.0}
    bad = []
    with _engine(name, mode) as e:
        e.keep_activations(True)
        e.forward(x)
        assert e.materialised('stem')                                   # the fused first block is off: the first join reads the stem's output
        T = lambda n: e.debug_tensor(n)
        from oracle import torch_oracle as O
        k = 'encoder.stem.convs.0'
        with torch.no_grad():
            want = O.conv_block(_f64(x), *(_f64(sd[f'{k}.{p}']) for p in ('conv.weight', 'conv.bias', 'norm.weight', 'norm.bias')), 1,
                                arch.norm_eps, arch.leaky_slope).numpy()
        cur, cur_name = T('stem'), 'stem'
        d = float(np.abs(cur - want).max())
        worst['act'] = max(worst['act'], d)
        if not d <= SPLIT_LAYER_TOL:
            bad.append(('stem', d))
        for s in range(arch.n_stages):
            for b in range(arch.n_blocks_per_stage[s]):
                nm = f'enc{s}.b{b}'
                stride, pool, proj = R.skip_layout(arch, s, b)
                c1, c2, out = T(f'{nm}.c1'), T(f'{nm}.c2'), T(nm)
                # conv1 from the block's input, conv2 from the engine's conv1, the projection from the block's input: float64 blocks
                ref = R.block_forward(arch, sd, s, b, cur, dtype=torch.float64)
                d1 = float(np.abs(c1 - ref['c1'].numpy()).max())
                k2 = f'{R.block_keys(s, b)}.conv2'
                with torch.no_grad():
                    want2 = O.conv_block(_f64(c1), *(_f64(sd[f'{k2}.{p}']) for p in ('conv.weight', 'conv.bias', 'norm.weight', 'norm.bias')), 1,
                                         arch.norm_eps, 1.0).numpy()
                d2 = float(np.abs(c2 - want2).max())
                worst['act'], worst['c2'] = max(worst['act'], d1), max(worst['c2'], d2)
                bad += [(f'{nm}.c1', d1)] * (not d1 <= SPLIT_LAYER_TOL) + [(f'{nm}.c2', d2)] * (not d2 <= SPLIT_LAYER_TOL)
                if proj:
                    pj = T(f'{nm}.proj')
                    dp = float(np.abs(pj - ref['proj'].numpy()).max())
                    worst['proj'] = max(worst['proj'], dp)
                    bad += [(f'{nm}.proj', dp)] * (not dp <= SPLIT_LAYER_TOL)
                    r = pj.astype(np.float64)
                elif pool:                                               # float32, ATen's own average of the values the accessor shows
                    r = torch.nn.functional.avg_pool2d(torch.from_numpy(cur), pool, pool).numpy().astype(np.float64)
                else:
                    r = cur.astype(np.float64)
                t = c2.astype(np.float64) + r
                wantj = np.where(t > 0, t, t * np.float64(np.float32(arch.leaky_slope)))
                bound = 4 * 2.0 ** -23 * np.maximum(1.0, np.maximum(np.abs(c2), np.abs(r)))
                ratio = float((np.abs(out - wantj) / bound).max())
                worst['join'] = max(worst['join'], ratio)
                bad += [(nm, ratio)] * (not ratio <= 1.0)
                assert out.shape == c2.shape == c1.shape
                cur, cur_name = out, nm
    print(f'{name} {mode}: worst stem / c1 {worst["act"]:.3e}  c2 {worst["c2"]:.3e}  proj {worst["proj"]:.3e}  (bound {SPLIT_LAYER_TOL:.0e});  '
          f'join {worst["join"]:.3f} of its bound')
    assert not bad, (name, mode, bad)


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
