"""The per-layer harness (tests/layer_check.py) proves its own sensitivity, without a GPU: torch on the CPU stands in for the engine.

Net: five stages (32, 32, 64, 64, 64), 128 x 128, B = 5 - blocks at 128 x 128 (level 0), 16 x 16 (level 3) and 8 x 8 pixels (level 4, where
the engine puts four images into one pixel tile).  ``got`` = the torch-fp32 block on the fp32 tensors the fp32 chain holds in front of it,
``want`` = ``layer_check.reference_block`` in float64 on the same tensors, judged by ``layer_check.layer_error``: every op of the program
passes, none excluded (measured worst: 3.2e-6 absolute on a block - dec1.c1, 288 terms; the bound is 8e-6 - 3.6e-7 relative on a
transposed conv, 2.1e-7 on the head; enc0.c1 from the network input through both blocks 2.6e-6; the 16-bit restatement 1.4e-6).  Then ONE
seeded defect at a time in ``got``'s computation; the same defect is pushed through the whole fp32 chain to the logits and compared with
the clean chain (``torch_oracle.unet_forward``) under ``TOL = 1e-4``, the end-to-end bound of tests/test_gpu_parity.py (the 16-bit
defect: under its ``F16E_MAX`` / ``F16E_RMS`` = 0.1 / 0.012).  Rows (0, B - 1) per layer, as the GPU module compares.

What was found (per-layer max against its bound of 8e-6 | logits against TOL = 1e-4):

  defect                                                                   per layer            end to end
  border        convT bias missing on the last image column, dec1.c0       1.9e-2   caught      2.4e-2   caught
  tap           one tap of one output channel, columns 32-63, enc0.c1      1.1e+0   caught      8.5e-1   caught
  tap_deep      the same on the 16 x 16 level (one tile), enc3.c1          1.2e+0   caught      2.8e-1   caught
  lohi          lo x hi product of the split left out for one 16-channel
                chunk, enc0.c1 (128 x 128)                                 1.1e-3   caught      4.5e-3   caught
  lohi_deep     ... enc3.c1 (16 x 16)                                      6.1e-4   caught      8.3e-4   caught
  unbiased      InstanceNorm with variance * n / (n - 1), enc3.c1          8.2e-3   caught      5.1e-3   caught
  eps_out       InstanceNorm with 1 / (sqrt(var) + eps), enc3.c1           2.0e-5   caught      1.8e-5   PASSES end to end
  tilerow       statistics without the last 8 of 128 rows, enc0.c1         2.9e-2   caught      7.5e-2   caught
  tilerow_deep  ... without the last 8 of 16 rows, enc3.c1                  5.7e-1   caught      3.8e-1   caught
  nextimg       8 x 8 level, B = 5: statistics of image 3 for image 4      1.3e+0   caught      4.0e-1   caught
  trunc         16-bit mode: stored conv output truncated, enc1.c1         rms 3.1e-4 (1e-4) caught    1.4e-2 max / 2.1e-3 rms  PASSES end to end

Every seeded defect is caught per layer; none of the list escapes.  Two of them stay below the end-to-end bound - ``eps_out`` and the
truncating 16-bit store: a kernel with one of these passes tests/test_gpu_parity.py.  The others are caught end to end as well ON THIS NET
(23 ops, synthetic weights whose blocks amplify a perturbation on the way to the logits); what the per-layer check adds for them is the
margin - 70x (lohi_deep) to 1e5x over the bound where the logits exceed theirs by 8x to 1e4x - and the name of the layer.
The narrowest per-layer margin is ``eps_out`` (2.0e-5 against 8e-6, a factor 2.4): on a channel whose standard deviation is near 0.5 that
defect vanishes to first order (sqrt(v + eps) - sqrt(v) - eps = eps (1 / (2 sigma) - 1)), so it is caught on the block as a whole and
not on every channel of it.

MANY-CLASS HEADS.  What tests/test_gpu_many_heads.py can see of a defective HEAD kernel (its checks a. and b.): two-stage nets of that module - K = 118 at
C = 32 and K = 40 at C = 64, weights and inputs seeded 300 + K - B = 3 of 16 x 32; ``nextimg`` on B = 3 of 4 x 32, the input whose first
256-pixel block holds the pixels of two images (that input is judged per layer only on the GPU).  ``got`` = the float32 torch head with ONE
seeded defect, on the float32 chain's own ``dec0.c0``; per layer against ``layer_check.reference_block('head')`` under ``HEAD_RTOL``, all
rows; end to end against the clean chain's logits at ``TOL`` (16-bit defect: ``F16E_MAX`` / ``F16E_RMS`` against the 16-bit oracle).

  defect                                                             net         per layer (of the largest logit)    end to end (max | rms)
  cols32   heads >= 32 computed with the weights of head k - 32      K=118 C=32  1.7e+0   caught                     1.1e+1 | 1.2e+0   caught
           (what a 32-column kernel would do)                        K=40  C=64  1.3e+0   caught                     6.0e+0 | 5.6e-1   caught
  bias32   the bias read at k mod 32                                 K=118 C=32  7.7e-3   caught                     4.7e-2 | 1.3e-2   caught
                                                                     K=40  C=64  1.8e-3   caught                     8.0e-3 | 2.4e-3   caught
  chan56   the last 8 of 64 channels left out                        K=40  C=64  5.7e-1   caught                     2.6e+0 | 3.8e-1   caught
  nextimg  image 0's scale and shift for the pixels of image 1,      K=118 C=32  1.1e-1   caught                     5.7e-1 | 5.8e-2   caught
           4 x 32: the block that holds both                         K=40  C=64  1.0e-1   caught                     4.9e-1 | 6.4e-2   caught
  trunc16  16-bit mode: the fp16 operand cut off, not rounded        K=118 C=32  6.0e-4   NOT caught (1.5e-3)        3.7e-3 | 5.0e-4   PASSES (0.1 | 0.012)
                                                                     K=40  C=64  6.4e-4   NOT caught (1.5e-3)        2.9e-3 | 4.9e-4   PASSES (0.1 | 0.012)

The first four are caught per layer with a margin of 1.8e3 (bias32 at K = 40) to 1.7e6 over HEAD_RTOL = 1e-6 (the clean float32 head: 2.0e-7
... 3.3e-7), and end to end as well: a defect of the LAST op reaches the logits undamped.  The fifth is NOT caught, per layer or end to end,
and is recorded as found: a truncated fp16 operand moves a logit by 6.0e-4 ... 6.4e-4 of the largest one - 32 or 64 terms of half an fp16 unit
each, whose signs follow the weights' and cancel - which is the size of a CORRECT kernel's distance from the 16-bit oracle (head_1x1 keeps fp32
weights and operands there: 3.2e-4 ... 4.7e-4 on the MI355X, tests/test_gpu_many_heads.py) and 0.4 of HEAD_RTOL['f16'] = 1.5e-3.  A check
that separates rounding from truncation of the head's operand would have to compare operands, not logits.

The numbers above are asserted as classifications (caught / passes), not as values; each case prints its figures (``pytest -s``)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_oracle as O
from tests import cases
from tests import layer_check as LC
from totalsegmentator2d_amd import weights
from totalsegmentator2d_amd.arch import UNetArch, OP_CONV3X3, OP_CONVT2X2

TOL = 1e-4                                   # tests/test_gpu_parity.py: TOL, F16E_MAX, F16E_RMS (restated: that module needs no import here)
F16E_MAX, F16E_RMS = 0.1, 0.012
B, HW, SEED = 5, 128, 13
NIMG = 4                                     # images per pixel tile on the 8 x 8 level (csrc/dispatch.cpp tile_geom)


@pytest.fixture(scope='module')
def net():
    arch = cases.unet(5, (32, 32, 64, 64, 64), 6)
    sd = weights.synthetic_state_dict(arch, SEED)
    x = cases.make_input(arch, B, HW, HW, SEED)
    logits, inter = O.unet_forward(arch, sd, x, return_intermediates=True)
    inter = {k: v.numpy() for k, v in inter.items()}
    inter['input'] = x
    inter['head'] = logits.numpy()
    return arch, sd, inter


# ------------------------------------------------------------------------------------------------------------------ the stand-in engine
def _split16(t):
    """hi / lo parts of the split mode (scripts/split_accuracy_experiment.py: split)."""
    hi = t.to(torch.float16).float()
    return hi, (t - hi).to(torch.float16).float()


def block32(arch, sd, name, srcs, defect=None, f16=False):
    """ONE op of the program in fp32 from the fp32 tensors `srcs` (layer_check.op_sources order), written out so that a defect can be
    seeded: conv -> statistics -> normalise -> LeakyReLU.  `defect`: None or the name of one defect, applied if this is its block.
    `f16`: the 16-bit contract of torch_oracle.conv_block in its storage view."""
    t = {k: O._t(v) for k, v in sd.items()}
    src = [O._t(s).float() for s in srcs]
    hit = defect is not None and DEFECTS[defect][0] == name
    with torch.no_grad():
        if name == 'head':
            k = f'decoder.seg_layers.{arch.n_stages - 2}'
            return F.conv2d(src[0], t[f'{k}.weight'], t[f'{k}.bias']).numpy()
        lvl = int(name[3:name.index('.')])
        j = arch.n_stages - 2 - lvl
        if name.endswith('.up'):
            return F.conv_transpose2d(src[0], t[f'decoder.transpconvs.{j}.weight'], t[f'decoder.transpconvs.{j}.bias'],
                                      stride=tuple(arch.strides[lvl + 1])).numpy()
        i = int(name[name.index('.c') + 2:])
        if name.startswith('enc'):
            k, stride = f'encoder.stages.{lvl}.0.convs.{i}', (tuple(arch.strides[lvl]) if (i == 0 and lvl > 0) else 1)
        else:
            k, stride = f'decoder.stages.{j}.convs.{i}', 1
        xin = src[0]
        if f16 and name != 'enc0.c0':
            src = [O._h(s) for s in src]
            xin = src[0]
        if name.startswith('dec') and i == 0:
            wt, bt = t[f'decoder.transpconvs.{j}.weight'], t[f'decoder.transpconvs.{j}.bias']
            up = F.conv_transpose2d(src[0], O._h(wt) if f16 else wt, bt, stride=tuple(arch.strides[lvl + 1]))
            if hit and defect == 'border':                   # the bias variant of the image's last column: the bias is not there
                up[:, :, :, -1] -= bt[None, :, None]
            xin = torch.cat((O._h(up) if f16 else up, src[1]), 1)
        w, b, g, be = (t[f'{k}.{s}'] for s in ('conv.weight', 'conv.bias', 'norm.weight', 'norm.bias'))
        if f16 and name != 'enc0.c0':
            w = O._h(w)
        y = F.conv2d(xin, w, b, stride=stride, padding=1)
        if hit and defect in ('tap', 'tap_deep'):            # tap (0, 2) of output channel 5 inside the second 32-column tile (or the only one)
            w1 = torch.zeros_like(w[5:6]); w1[:, :, 0, 2] = w[5:6, :, 0, 2]
            c0, c1 = (32, 64) if y.shape[3] > 32 else (0, y.shape[3])
            y[:, 5, :, c0:c1] -= F.conv2d(xin, w1, None, stride=stride, padding=1)[:, 0, :, c0:c1]
        if hit and defect in ('lohi', 'lohi_deep'):          # x = xh + xl, w = wh + wl: the product xl * wh of channels 16-31 is left out
            xl, wh = _split16(xin[:, 16:32])[1], _split16(w[:, 16:32])[0]
            y = y - F.conv2d(xl, wh, None, stride=stride, padding=1)
        if f16:
            if hit and defect == 'trunc':                    # the stored fp16 value cut off (towards zero) instead of rounded to nearest even
                h = y.to(torch.float16)
                over = h.float().abs() > y.abs()
                bits = h.view(torch.int16)
                y = torch.where(over, (bits - 1).view(torch.float16), h).float()
            else:
                y = O._h(y)
        n = y.shape[2] * y.shape[3]
        ys = y
        if hit and defect in ('tilerow', 'tilerow_deep'):    # the statistics miss the last row of 8-row tiles
            ys = y[:, :, :-8]
        mean = ys.mean((2, 3), keepdim=True)
        var = ((ys - mean) ** 2).mean((2, 3), keepdim=True)
        if hit and defect == 'unbiased':
            var = var * (n / (n - 1.0))
        if hit and defect == 'nextimg':                      # image 0 of the second tile normalised with the statistics of image 3 of the first
            mean, var = mean.clone(), var.clone()
            mean[NIMG], var[NIMG] = mean[NIMG - 1], var[NIMG - 1]
        rstd = 1.0 / (var.sqrt() + arch.norm_eps) if (hit and defect == 'eps_out') else 1.0 / (var + arch.norm_eps).sqrt()
        out = (y - mean) * rstd * g[None, :, None, None] + be[None, :, None, None]
        return F.leaky_relu(out, arch.leaky_slope).numpy()


def forward32(arch, sd, x, defect=None, f16=False):
    """The whole chain through :func:`block32`; returns the logits."""
    have = {'input': x}
    for op in arch.program():
        n = op['name']
        if op['op'] == OP_CONVT2X2:
            continue                                         # (evaluated inside decL.c0, as layer_forward does)
        have[n] = block32(arch, sd, n, [have[s] for s in LC.op_sources(arch, n)], defect, f16)
    return have['head']


# defect -> (the block it sits in, mode of the per-layer check, caught per layer?, stays under the end-to-end bound?)
DEFECTS = {
    'border': ('dec1.c0', 'split', True, False),
    'tap': ('enc0.c1', 'split', True, False),
    'tap_deep': ('enc3.c1', 'split', True, False),
    'lohi': ('enc0.c1', 'split', True, False),
    'lohi_deep': ('enc3.c1', 'split', True, False),
    'unbiased': ('enc3.c1', 'split', True, False),
    'eps_out': ('enc3.c1', 'split', True, True),
    'tilerow': ('enc0.c1', 'split', True, False),
    'tilerow_deep': ('enc3.c1', 'split', True, False),
    'nextimg': ('enc4.c1', 'split', True, False),
    'trunc': ('enc1.c1', 'f16', True, True),
}


# ------------------------------------------------------------------------------------------------------------------ the clean chain passes
def test_the_net_has_the_levels_the_defects_need(net):
    arch, _, inter = net
    assert inter['enc0.c1'].shape[2:] == (128, 128) and inter['enc3.c1'].shape[2:] == (16, 16) and inter['enc4.c1'].shape[2:] == (8, 8)
    assert inter['enc4.c1'].shape[0] == B == NIMG + 1


@pytest.mark.parametrize('mode', ['split', 'exact', 'f16'])
def test_clean_fp32_blocks_pass_the_layer_bound_none_excluded(net, mode):
    """got = torch's own fp32 block (``layer_forward``; 16-bit: the written-out restatement, another summation order of the statistics) on
    the fp32 chain's tensors; every op of the program, the transposed convs and the head included."""
    arch, sd, inter = net
    bad, worst = [], {}
    for op in arch.program():
        n = op['name']
        srcs = [inter[s] for s in LC.op_sources(arch, n)]
        if mode == 'f16':
            got = O._h(O._t(block32(arch, sd, n, srcs)).float()).numpy() if n.endswith('.up') else (
                O.layer_forward(arch, sd, 'head', srcs[0], emulate='f16').numpy() if n == 'head' else block32(arch, sd, n, srcs, f16=True))
        elif n.endswith('.up'):
            got = block32(arch, sd, n, srcs)
        else:
            got = O.layer_forward(arch, sd, n, *srcs).numpy()
        ok, w, text = LC.layer_error(n, got, LC.reference_block(arch, sd, n, srcs, mode), mode)
        worst[n] = w
        if not ok:
            bad.append(text)
    print(f'[layer-check-cpu] clean {mode}: ' + ', '.join(f'{n} {w:.2e}' for n, w in worst.items()))
    assert not bad, bad
    assert len(worst) == len(arch.program())


def test_the_written_out_block_is_torchs_block(net):
    """block32 without a defect against layer_forward (F.instance_norm): the same block to fp32 rounding, so that what a seeded defect
    changes is the defect alone."""
    arch, sd, inter = net
    for op in arch.program():
        n = op['name']
        if op['op'] != OP_CONV3X3:
            continue
        srcs = [inter[s] for s in LC.op_sources(arch, n)]
        assert np.abs(block32(arch, sd, n, srcs) - O.layer_forward(arch, sd, n, *srcs).numpy()).max() <= 2e-6, n
    lg = forward32(arch, sd, inter['input'])
    assert np.abs(lg - inter['head']).max() <= 3e-5                # (two fp32 chains: the bound tests/test_gpu_parity.py uses between two paths)


def test_the_first_block_through_the_second_from_the_network_input(net):
    """``reference_block(.., from_input=True)``: enc0.c1 from the network input through both blocks in float64 - what judges an engine
    that materialises no enc0.c0.  The fp32 chain passes it; a defect inside the FIRST block (bias of channel 3 left out) fails it."""
    arch, sd, inter = net
    want = LC.reference_block(arch, sd, 'enc0.c1', [inter['input']], 'split', from_input=True)
    ok, w, text = LC.layer_error('enc0.c1', inter['enc0.c1'], want, 'split')
    print(f'[layer-check-cpu] enc0.c1 from the input: {w:.2e}')
    assert ok, text
    two = LC.reference_block(arch, sd, 'enc0.c1', [inter['enc0.c0']], 'split')
    assert np.abs(two - want).max() <= LC.SPLIT_LAYER_TOL          # (the two references differ by the fp32 rounding of enc0.c0 only)
    sd2 = dict(sd)
    sd2['encoder.stages.0.0.convs.0.norm.bias'] = sd['encoder.stages.0.0.convs.0.norm.bias'].copy()
    sd2['encoder.stages.0.0.convs.0.norm.bias'][3] += np.float32(1e-3)
    c0 = O.layer_forward(arch, sd2, 'enc0.c0', inter['input']).numpy()
    got = O.layer_forward(arch, sd, 'enc0.c1', c0).numpy()
    ok, w, text = LC.layer_error('enc0.c1', got, want, 'split')
    assert not ok, text


# ------------------------------------------------------------------------------------------------------------------ the seeded defects
@pytest.mark.parametrize('defect', list(DEFECTS))
def test_seeded_defect(net, defect):
    arch, sd, inter = net
    name, mode, caught, passes_e2e = DEFECTS[defect]
    f16 = mode == 'f16'
    srcs = [inter[s] for s in LC.op_sources(arch, name)]
    if f16:                                                  # the 16-bit chain's own tensors in front of the block
        _, i16 = O.unet_forward(arch, sd, inter['input'], return_intermediates=True, emulate='f16')
        srcs = [i16[s].numpy() for s in LC.op_sources(arch, name)]
    want = LC.reference_block(arch, sd, name, srcs, mode)
    rows = (0, B - 1)                                        # what the GPU module compares
    clean = block32(arch, sd, name, srcs, None, f16)
    ok0, w0, text0 = LC.layer_error(name, clean[list(rows)], want[list(rows)], mode)
    assert ok0, ('the clean block must pass', text0)
    got = block32(arch, sd, name, srcs, defect, f16)
    assert not np.array_equal(got, clean), 'the defect changed nothing'
    ok, w, text = LC.layer_error(name, got[list(rows)], want[list(rows)], mode)
    # ... and to the logits, against the clean chain
    if f16:
        ref = O.unet_forward(arch, sd, inter['input'], emulate='f16').numpy()
        d = forward32(arch, sd, inter['input'], defect, f16=True) - ref
        e2e, e2e_rms = float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))
        under = e2e <= F16E_MAX and e2e_rms <= F16E_RMS
        print(f'[layer-check-cpu] {defect} in {name}: per layer {text} (clean {w0:.2e}) -> {"caught" if not ok else "NOT caught"}; '
              f'logits max {e2e:.2e} rms {e2e_rms:.2e} -> {"passes" if under else "caught"} end to end')
    else:
        e2e = float(np.abs(forward32(arch, sd, inter['input'], defect) - inter['head']).max())
        under = e2e <= TOL
        print(f'[layer-check-cpu] {defect} in {name}: per layer {text} (clean {w0:.2e}) -> {"caught" if not ok else "NOT caught"}; '
              f'logits {e2e:.2e} -> {"passes" if under else "caught"} end to end')
    assert (not ok) == caught, text
    assert under == passes_e2e, e2e


def test_the_argument_for_per_layer_bounds():
    """At least one seeded defect is caught per layer and passes end to end - and none of the list escapes the per-layer bound."""
    assert all(v[2] for v in DEFECTS.values())
    assert sum(v[3] for v in DEFECTS.values()) >= 2


# ------------------------------------------------------------------------------------------------------------------ two descriptions of one graph
@pytest.mark.parametrize('which', ['canonical', 'aniso_21', 'xr_1ch'])
def test_op_sources_agrees_with_the_program(which):
    """``layer_check.op_sources`` against the ``src`` / ``skip`` fields of ``arch.program()``: a decoder entry reads what its transposed
    conv reads, and its skip."""
    arch = UNetArch.canonical() if which == 'canonical' else cases.SMALL_CASES[which][0]
    prog = {o['name']: o for o in arch.program()}
    for n, o in prog.items():
        if o['skip'] is not None:
            assert prog[o['src']]['op'] == OP_CONVT2X2
            want = (prog[o['src']]['src'], o['skip'])
        else:
            want = (o['src'],)
        assert LC.op_sources(arch, n) == want, (n, LC.op_sources(arch, n), want)


# ------------------------------------------------------------------------------------------------------------------ many-class heads
# (the table of these defects is in the module docstring: MANY-CLASS HEADS)
HEAD_NETS = {'K118_C32': ((32, 32), 118), 'K40_C64': ((64, 64), 40)}
# defect -> (mode, extent of the input, nets, caught per layer?, stays under the end-to-end bound?)
HEAD_DEFECTS = {
    'cols32': ('split', (16, 32), ('K118_C32', 'K40_C64'), True, False),
    'bias32': ('split', (16, 32), ('K118_C32', 'K40_C64'), True, False),
    'chan56': ('split', (16, 32), ('K40_C64',), True, False),
    'nextimg': ('split', (4, 32), ('K118_C32', 'K40_C64'), True, False),
    'trunc16': ('f16', (16, 32), ('K118_C32', 'K40_C64'), False, True),
}
_head_cases = {}


def _head_case(net, hw):
    """(arch, sd, x, the float32 chain's tensors, the 16-bit chain's tensors) of a head net on B = 3 of `hw`, made once."""
    if (net, hw) not in _head_cases:
        feats, K = HEAD_NETS[net]
        arch = cases.unet(2, feats, K, nconv=1)
        sd = weights.synthetic_state_dict(arch, 300 + K)
        x = cases.make_input(arch, 3, hw[0], hw[1], 300 + K)
        out = []
        for emulate in (None, 'f16'):
            lg, inter = O.unet_forward(arch, sd, x, return_intermediates=True, emulate=emulate)
            inter = {k: v.numpy() for k, v in inter.items()}
            inter['head'] = lg.numpy()
            out.append(inter)
        _head_cases[(net, hw)] = (arch, sd, x, out[0], out[1])
    return _head_cases[(net, hw)]


def _trunc16(t):
    """float32 -> fp16 cut off towards zero (the defect ``trunc`` above, on an operand) -> float32."""
    h = t.to(torch.float16)
    over = h.float().abs() > t.abs()
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h).float()


def head32(arch, sd, inter, defect=None, f16=False):
    """The head in float32 from the chain's tensors, written out so that a defect can be seeded: ``dec0.c0`` = conv -> statistics ->
    scale / shift -> LeakyReLU (what the head kernels apply on load), then the 1x1 conv.  `f16`: fp16 weights and operand, fp32 sums - from
    the storage view of ``dec0.c0``, as ``layer_check`` feeds the 16-bit head."""
    t = {k: O._t(v) for k, v in sd.items()}
    w, b = t['decoder.seg_layers.0.weight'].clone(), t['decoder.seg_layers.0.bias'].clone()
    K = w.shape[0]
    with torch.no_grad():
        if defect == 'nextimg':                              # dec0.c0 once more with image 0's statistics for image 1
            k = 'decoder.stages.0.convs.0'
            up = F.conv_transpose2d(O._t(inter['enc1.c0']), t['decoder.transpconvs.0.weight'], t['decoder.transpconvs.0.bias'], stride=tuple(arch.strides[1]))
            y = F.conv2d(torch.cat((up, O._t(inter['enc0.c0'])), 1), t[f'{k}.conv.weight'], t[f'{k}.conv.bias'], padding=1)
            mean = y.mean((2, 3), keepdim=True)
            rstd = 1.0 / (((y - mean) ** 2).mean((2, 3), keepdim=True) + arch.norm_eps).sqrt()
            clean = F.leaky_relu((y - mean) * rstd * t[f'{k}.norm.weight'][None, :, None, None] + t[f'{k}.norm.bias'][None, :, None, None], arch.leaky_slope)
            assert float((clean - O._t(inter['dec0.c0'])).abs().max()) <= 2e-6            # the written-out block is torch's block
            mean, rstd = mean.clone(), rstd.clone()
            mean[1], rstd[1] = mean[0], rstd[0]
            xin = F.leaky_relu((y - mean) * rstd * t[f'{k}.norm.weight'][None, :, None, None] + t[f'{k}.norm.bias'][None, :, None, None], arch.leaky_slope)
        else:
            xin = O._t(inter['dec0.c0']).float()
        if defect == 'cols32':
            w[32:] = t['decoder.seg_layers.0.weight'][:K - 32]
        if defect == 'bias32':
            b = b[torch.arange(K) % 32]
        if defect == 'chan56':
            assert w.shape[1] == 64
            w[:, 56:] = 0
        if f16:
            xin, w = (_trunc16(xin) if defect == 'trunc16' else O._h(xin)), O._h(w)
        return F.conv2d(xin, w, b).numpy()


def test_the_head_nets_are_those_of_the_gpu_module():
    for net, (feats, K) in HEAD_NETS.items():
        arch = _head_case(net, (16, 32))[0]
        assert arch.features_per_stage == tuple(feats) and arch.num_classes == K > 32 and [o['name'] for o in arch.program()][-2:] == ['dec0.c0', 'head']
    assert _head_case('K118_C32', (4, 32))[2].shape == (3, 2, 4, 32)               # 384 pixels: the first 256-pixel block holds images 0 and 1


@pytest.mark.parametrize('defect,net', [(d, n) for d, v in HEAD_DEFECTS.items() for n in v[2]])
def test_seeded_head_defect(defect, net):
    mode, hw, _, caught, passes_e2e = HEAD_DEFECTS[defect]
    f16 = mode == 'f16'
    arch, sd, x, inter32, inter16 = _head_case(net, hw)
    inter = inter16 if f16 else inter32
    src = inter['dec0.c0']
    if f16:                                                  # what the accessor shows: the stored fp16 conv output normalised and activated in fp32
        src = O.layer_forward(arch, sd, 'dec0.c0', inter['enc1.c0'], inter['enc0.c0'], emulate='f16', storage_view=True).numpy()
    want = LC.reference_block(arch, sd, 'head', [src], mode)
    feed = dict(inter, **{'dec0.c0': src})
    clean = head32(arch, sd, feed, None, f16)
    ok0, w0, text0 = LC.layer_error('head', clean, want, mode)
    assert ok0, ('the clean head must pass', text0)
    got = head32(arch, sd, feed, defect, f16)
    assert not np.array_equal(got, clean), 'the defect changed nothing'
    ok, w, text = LC.layer_error('head', got, want, mode)
    d = got - inter['head']                                  # the head is the last op: its output IS the logits of the defective chain
    e2e, e2e_rms = float(np.abs(d).max()), float(np.sqrt((d.astype(np.float64) ** 2).mean()))
    under = (e2e <= F16E_MAX and e2e_rms <= F16E_RMS) if f16 else e2e <= TOL
    print(f'[layer-check-cpu] head {defect} {net} {hw}: per layer {text} (clean {w0:.2e}, bound {LC.HEAD_RTOL[mode]:.1e}) -> '
          f'{"caught" if not ok else "NOT caught"}; logits max {e2e:.2e} rms {e2e_rms:.2e} -> {"passes" if under else "caught"} end to end')
    assert (not ok) == caught, text
    assert under == passes_e2e, (e2e, e2e_rms)


def test_the_first_four_head_defects_are_caught_per_layer():
    assert [d for d, v in HEAD_DEFECTS.items() if not v[3]] == ['trunc16'] and len(HEAD_DEFECTS) == 5
