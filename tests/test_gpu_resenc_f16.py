"""The 16-bit mode (TS2D_PRECISION_F16) on a ResidualEncoderUNet: res_join<_Float16> and pool_proj1x1_h (csrc/kernels_resblock.h) between the
16-bit kernels every other op already had, behind the opt-in option "resf16".  Reference: the contract of include/ts2d_engine.h restated in
tests/resenc_f16_util.py (checked on the CPU by tests/test_resenc_f16_cpu.py).

Bounds, none of them measured on the code under test:
  conv1 / conv2 / projection / decoder blocks, each fed with the engine's own inputs of that op (storage views): F16_LAYER_MAX, F16_LAYER_RMS,
    F16_LAYER_RMS_COMPOSED of tests/test_gpu_parity.py at levels of >= 64 pixels (single half flips of stored values), finiteness below;
    a stand-alone transposed conv and the head: F16_UP_RTOL / HEAD_RTOL['f16'] of tests/layer_check.py;
  a join, at every level, element-wise: both sides add the same two fp32 addends up to an fp32 ulp or two, so an element agrees or flips one
    half rounding: |got - want| <= 2^-10 max(|t|, 2^-14) (x slope where t < 0: the accessor shows leaky_relu(t)) + 4 * 2^-23 |t|, and at most
    1 % of a join's elements may differ at all (a flip needs the fp32 sum within a couple of ulps of a half tie: about 2^-12 of them).
    Where the join adds the STEM's operand (enc0.b0) that operand is h(n) of an fp32 n the accessor shows within an fp32 ulp or two of the
    kernel's own (the accessor multiplies and adds, the kernels use one fma): an n within NUDGE of a half tie is compatible with both
    neighbours, and an element passes if it passes against either (every other join adds a join's output or a projection: exact);
  end to end: F16E_MAX / F16E_RMS against the restatement on the cases tests/test_resenc_f16_cpu.py qualifies (all ten), F16_MAX / F16_RMS against
    the float32 restatement; the masks bit-exact as a function of the engine's own logits.
Measured on an MI355X (profiles/r24_resenc_f16_err.txt, scripts/gpu_resenc_f16_err.py; worst over the ten cases and both dispatches):
  joins                              0 of the bound, no element differs: bit-identical to the restatement on the engine's own inputs
  stem / conv1 / decoder blocks      2.8e-3 max, 4.8e-5 rms      conv2        3.2e-3 max, 7.6e-5 rms
  projection                         4.2e-3 max, 2.8e-5 rms      decoder entry 4.3e-3 max, 3.2e-4 rms
  transposed conv 5.8e-4, head 4.3e-4 relative
  logits vs the restatement          1.0e-2 max, 1.8e-3 rms      vs float32   1.3e-2 max, 2.3e-3 rms
  model folder through the predictor 3.9e-3 on the aggregated float16 logits [1.6e-2]"""
import numpy as np
import pytest

from tests import layer_check as LC
from tests import resenc_f16_util as R16
from tests import resenc_util as R
from tests.conftest import blob_for
from tests.test_resenc_f16_cpu import E2E_CASES, JOIN_DIFFER_CAP
from totalsegmentator2d_amd import prng
from totalsegmentator2d_amd.engine import Engine, unpack_mask

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

NUDGE = 2.0 ** -22              # 2 fp32 ulps at 1: how far the accessor's n of a conv block may lie from the kernel's own
SW_TOL = 1.6e-2                 # the sliding-window tolerance: 2 half-ulps at |x| <= 8 (tests/test_gpu_predictor.py, tests/test_gpu_resenc.py)


def _bounds():
    from tests import test_gpu_parity as P
    return P


def _engine(name, options=None, f16=True):
    arch, B, H, W, seed = R.RES_CASES[name]
    e = Engine(arch, blob_for(arch, seed)[1], options=options)
    if f16:
        e.set_option('resf16', 1)
        e.set_precision('f16')
    return e


_ref = {}


def ref_logits(name):
    """The restatement's logits of a case, computed once."""
    if name not in _ref:
        arch, B, H, W, seed = R.RES_CASES[name]
        _ref[name] = R16.resenc_forward_f16(arch, blob_for(arch, seed)[0], R.case_input(name)).numpy()
    return _ref[name]


# ------------------------------------------------------------------------------------------------------------------ 1. opt-in
def test_the_mode_is_opt_in_and_leaves_the_split_mode_as_it_was():
    x = R.case_input('res_min')
    want, E = R.oracle_logits('res_min')
    with _engine('res_min', f16=False) as fresh:
        split = fresh.forward(x)[0].copy()
    with _engine('res_min', f16=False) as e:
        with pytest.raises(RuntimeError, match=r'\(-1\).*TS2D_PRECISION_F16'):
            e.set_precision('f16')
        assert np.array_equal(e.forward(x)[0], split) and np.abs(split - want).max() <= max(1e-4, 2 * E)
        e.set_option('resf16', 1)
        e.set_precision('f16')
        e.set_profiling(True)
        lg = e.forward(x)[0].copy()
        kern = e.op_kernels()
        assert kern['enc1.b0.proj'] == 'pool_proj1x1_h' and kern['enc0.b0'] == 'res_join_h' and kern['enc1.b0'] == 'res_join_h', kern
        assert np.isfinite(lg).all() and not np.array_equal(lg, split)
        e.set_option('resf16', 0)                       # cleared with the mode still set: the forward fails, the mode is not changed silently
        with pytest.raises(RuntimeError, match='TS2D_PRECISION_F16'):
            e.forward(x)
        e.set_precision('split')
        assert np.array_equal(e.forward(x)[0], split)   # bit for bit the split logits of a fresh engine
        kern = e.op_kernels()
        assert kern['enc1.b0.proj'] == 'pool_proj1x1' and kern['enc0.b0'] == 'res_join', kern


def test_the_option_has_no_effect_on_a_plain_engine():
    from tests import cases
    arch, B, H, W, seed = cases.SMALL_CASES['k_min2']
    x = cases.make_input(arch, B, H, W, seed)
    blob = blob_for(arch, seed)[1]
    with Engine(arch, blob) as a, Engine(arch, blob, options={'resf16': 1}) as b:
        for mode in ('split', 'f16'):
            a.set_precision(mode)
            b.set_precision(mode)
            assert np.array_equal(a.forward(x)[0], b.forward(x)[0])


# ------------------------------------------------------------------------------------------------------------------ 2. per layer
def join_check(arch, sd, name, got, srcs):
    """(worst |got - want| in units of the join's bound, share of elements that differ at all) of join `name`."""
    prog = LC._program(arch)
    slope = float(np.float32(arch.leaky_slope))
    ambiguous = prog[prog[name]['res']]['op'] == LC.OP_CONV3X3         # the stem's operand, rebuilt from the accessor's view
    ratio, differ = None, None
    for nudge in ((-NUDGE, NUDGE) if ambiguous else (0.0,)):
        want, t = R16.op_reference(arch, sd, name, srcs, nudge=nudge)
        bound = 2.0 ** -10 * np.maximum(np.abs(t), 2.0 ** -14) * np.where(t < 0, slope, 1.0) + 4 * 2.0 ** -23 * np.abs(t)
        r, d = np.abs(got - want) / bound, got != want
        ratio, differ = (r, d) if ratio is None else (np.minimum(ratio, r), differ & d)
    return float(ratio.max()), float(differ.mean())


def check_ops(e, arch, sd, x, lg, tag, check=True):
    """Every op of the engine's last (profiled, keep-activations) forward against the restatement on the engine's own inputs of that op.
    Returns ({op: kernel}, {figure: worst value}); `check=False` (scripts/gpu_resenc_f16_err.py): measure only."""
    P = _bounds()
    prog = LC._program(arch)
    ran = {n: k for n, k in e.op_kernels().items() if k}
    rows = tuple(dict.fromkeys((0, x.shape[0] - 1)))
    cache = {}

    def tensor(n):
        if n not in cache:
            t = x if n == 'input' else (lg if n == 'head' else e.debug_tensor(n))
            cache[n] = np.ascontiguousarray(t[list(rows)])
        return cache[n]
    bad, lines, worst_join, fig = [], [], (0.0, 0.0), {}
    up = lambda k, v: fig.__setitem__(k, max(fig.get(k, 0.0), v))
    for o in arch.program():
        n = o['name']
        if n not in ran:
            assert o['op'] == LC.OP_CONVT2X2, (tag, n)                        # only a composed transposed conv has no launch of its own
            continue
        srcs = [tensor(s) for s in LC.op_sources(arch, n)]
        got = tensor(n).astype(np.float64)
        if not np.isfinite(got).all():
            bad.append(f'{n}: not finite')
            continue
        if o['op'] == LC.OP_JOIN:
            ratio, differ = join_check(arch, sd, n, got, srcs)
            worst_join = (max(worst_join[0], ratio), max(worst_join[1], differ))
            up('join, of its bound', ratio), up('join, share that differs', differ)
            lines.append(f'{n} {ran[n]} join {ratio:.3f} of its bound, {differ:.2e} differ')
            if ratio > 1.0 or differ > JOIN_DIFFER_CAP:
                bad.append(lines[-1])
            continue
        want = R16.op_reference(arch, sd, n, srcs)
        d = got - want
        mx, rms = float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))
        if o['op'] in (LC.OP_CONVT2X2, LC.OP_HEAD1X1):
            rel = mx / max(float(np.abs(want).max()), 1e-30)
            ok = rel <= (LC.HEAD_RTOL['f16'] if n == 'head' else LC.F16_UP_RTOL)
            lines.append(f'{n} {ran[n]} rel {rel:.2e}')
            up('head, relative' if n == 'head' else 'transposed conv, relative', rel)
        elif got.shape[2] * got.shape[3] >= 64:
            composed = o.get('skip') is not None
            ok = mx <= P.F16_LAYER_MAX and rms <= (P.F16_LAYER_RMS_COMPOSED if composed else P.F16_LAYER_RMS)
            lines.append(f'{n} {ran[n]} max {mx:.2e} rms {rms:.2e}')
            kind = 'decoder entry' if composed else ('projection' if o['op'] == LC.OP_PROJ1X1 else ('conv2' if o.get('linear') else 'stem / conv1 / decoder block'))
            up(f'{kind}, max', mx), up(f'{kind}, rms', rms)
        else:                                                                 # (statistics over a handful of pixels: finiteness only)
            ok = True
            lines.append(f'{n} {ran[n]} ({got.shape[2] * got.shape[3]} px) max {mx:.2e}')
        if not ok:
            bad.append(lines[-1])
    print(f'[resenc-f16] {tag}: ' + '; '.join(lines))
    print(f'[resenc-f16] {tag}: worst join {worst_join[0]:.3f} of its bound, largest share of differing elements {worst_join[1]:.2e}')
    assert not (bad and check), (tag, bad)
    return ran, fig


@pytest.mark.parametrize('sbk', [0, 1], ids=['full', 'default'])
@pytest.mark.parametrize('name', list(R.RES_CASES))
def test_every_op_on_the_engines_own_inputs(name, sbk):
    arch, B, H, W, seed = R.RES_CASES[name]
    sd = blob_for(arch, seed)[0]
    x = R.case_input(name)
    with _engine(name, options={'sbk': sbk}) as e:
        e.set_profiling(True)
        e.keep_activations(True)
        lg = e.forward(x)[0]
        ran, _ = check_ops(e, arch, sd, x, lg, f'{name} sbk={sbk}')
        split_k = e.op_ksplit()
    for o in arch.program():
        if o['op'] in (LC.OP_PROJ1X1, LC.OP_JOIN):
            assert ran[o['name']] == ('pool_proj1x1_h' if o['op'] == LC.OP_PROJ1X1 else 'res_join_h'), ran
    if name == 'res_deep':                               # split-K convs around the joins of the 16 x 16 level: under the default dispatch only
        assert any(s > 1 for n, s in split_k.items() if n.startswith('enc3.')) == bool(sbk), split_k


# ------------------------------------------------------------------------------------------------------------------ 3. end to end
@pytest.mark.parametrize('name', list(R.RES_CASES))
def test_logits_end_to_end(name):
    P = _bounds()
    from oracle import c_oracle as C
    arch, B, H, W, seed = R.RES_CASES[name]
    x = R.case_input(name)
    with _engine(name) as e:
        lg, mk = e.forward(x, logits=True, mask=(W % 32 == 0))
    assert np.isfinite(lg).all()
    d = lg - ref_logits(name)
    d32 = lg - R.oracle_logits(name)[0]
    mx, rms = float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))
    mx32, rms32 = float(np.abs(d32).max()), float(np.sqrt((d32 ** 2).mean()))
    print(f'[resenc-f16] {name}: logits vs the 16-bit restatement max {mx:.3e} rms {rms:.3e} (bounds {P.F16E_MAX} / {P.F16E_RMS}); '
          f'vs the float32 restatement max {mx32:.3e} rms {rms32:.3e} (bounds {P.F16_MAX} / {P.F16_RMS})')
    if name in E2E_CASES:
        assert mx <= P.F16E_MAX and rms <= P.F16E_RMS, (name, mx, rms)
    assert mx32 <= P.F16_MAX and rms32 <= P.F16_RMS, (name, mx32, rms32)
    if mk is not None:
        assert np.array_equal(unpack_mask(mk, W), C.logits_to_mask(lg))


# ------------------------------------------------------------------------------------------------------------------ 4. determinism
def test_a_rows_logits_do_not_depend_on_its_batch_mates():
    """The full-batch dispatch (what predict_tiled_batch runs): row 0 of res_pool at B = 3 and alone, bit for bit."""
    x = R.case_input('res_pool')
    assert x.shape[0] == 3
    with _engine('res_pool', options={'sbk': 0}) as e:
        three = e.forward(x)[0].copy()
        one = e.forward(np.ascontiguousarray(x[:1]))[0].copy()
    assert np.array_equal(three[0].view(np.uint32), one[0].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ 5. surface
SURFACE_SEED = 74                # tests/test_gpu_resenc.py


def test_a_model_folder_runs_through_the_predictor_in_the_16_bit_mode(tmp_path):
    from tests.host_predictor import HostLogicPredictor
    from totalsegmentator2d_amd import weights
    from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor
    arch = R.RES_CASES['res_min'][0]
    patch = (64, 64)
    R.write_model_folder(str(tmp_path), arch, SURFACE_SEED, patch)
    sd = weights.synthetic_state_dict(arch, SURFACE_SEED)
    data = prng.normal_f32(SURFACE_SEED, 999, (arch.input_channels, 1, 80, 52))
    twin = HostLogicPredictor(network=lambda b: R16.resenc_forward_f16(arch, sd, b).numpy(), tile_step_size=0.5, use_mirroring=True, precision='f16')
    twin.initialize_from_trained_model_folder(str(tmp_path), (0,), 'checkpoint_final.pth')
    ref = twin.predict_sliding_window_return_logits(data)
    p = HIPnnUNetPredictor(tile_step_size=0.5, use_mirroring=True, precision='f16')
    p.initialize_from_trained_model_folder(str(tmp_path), (0,), 'checkpoint_final.pth')
    try:
        assert p.arch == arch and p.tile_dtype == twin.tile_dtype == 'half'
        got = p.predict_logits_from_preprocessed_data(data).cpu().numpy()
        p.engines[0].set_profiling(True)
        p.engines[0].forward(np.zeros((1, arch.input_channels) + patch, np.float32))
        kern = p.engines[0].op_kernels()
    finally:
        p.close()
    assert kern['enc1.b0.proj'] == 'pool_proj1x1_h' and kern['enc1.b0'] == 'res_join_h', kern
    assert got.shape == ref.shape and got.dtype == np.float16
    err = float(np.abs(got.astype(np.float32) - ref.astype(np.float32)).max())
    print(f'[resenc-f16] surface: max |logits - restatement through the host twin| {err:.3e} (bound {SW_TOL})')
    assert err <= SW_TOL


def test_a_set_of_a_plain_and_a_residual_member_at_its_default_precision():
    from tests import cases
    from totalsegmentator2d_amd.submodels import SubModelSet
    parch, _, _, _, pseed = cases.SMALL_CASES['k_min2']
    rarch, B, H, W, rseed = R.RES_CASES['res_min']
    assert parch.input_channels == rarch.input_channels
    models = [('a_plain', parch, blob_for(parch, pseed)[1]), ('b_residual', rarch, blob_for(rarch, rseed)[1])]
    x = R.case_input('res_min')
    xt = torch.from_numpy(x).cuda()
    with SubModelSet(models) as ms:
        masks = [m.cpu().numpy() for m in ms.forward_masks(xt)]
        torch.cuda.synchronize()
        ms.engines[1].set_profiling(True)
        ms.forward_masks(xt)
        torch.cuda.synchronize()
        kern = ms.engines[1].op_kernels()
    assert kern['enc1.b0.proj'] == 'pool_proj1x1_h' and kern['enc0.b0'] == 'res_join_h', kern
    with Engine(parch, models[0][2]) as e:
        e.set_precision('f16')
        want_p = e.forward(x, logits=False, mask=True)[1]
    with _engine('res_min') as e:
        lg, want_r = e.forward(x, logits=True, mask=True)
    u32 = lambda m: np.ascontiguousarray(m).view(np.uint32)
    assert np.array_equal(u32(masks[0]), u32(want_p)) and np.array_equal(u32(masks[1]), u32(want_r))       # the members alone, bit for bit
    d = lg - ref_logits('res_min')
    P = _bounds()
    assert np.abs(d).max() <= P.F16E_MAX and np.sqrt((d ** 2).mean()) <= P.F16E_RMS
