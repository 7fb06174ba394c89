"""The residual rules of the per-layer harness (tests/layer_check.py) prove their own sensitivity, without a GPU: torch fp32 on the CPU
stands in for the engine, as tests/test_layer_check_cpu.py does for the plain net.

Cases (tests/resenc_util.py): ``res_win12`` (B = 3: a pool-only join behind a (1, 2) window, a projection behind a (2, 1) window, a
pool-only (2, 2) join) and ``res_span`` (B = 3: the projection of level 1 has M = 576 rows of 192-pixel images - 4.5 tiles of 128 rows).
The stand-in holds what the engine holds: a join tensor is the PRE-activation sum and whoever reads it applies the block's LeakyReLU;
``shown`` is what ``Engine.debug_tensor`` shows (the activated value).  ``got`` = the written-out fp32 op on the shown fp32 tensors of the clean
chain, ``want`` / bound = ``layer_check.reference_block`` / ``_res_terms`` on the same tensors, judged by ``layer_check.layer_error``, rows
(0, B - 1) as the GPU module compares.  Every op of the clean chain passes, none excluded (worst 3.0e-6 on a block against 8e-6, joins at
most 0.25 of their bound).  Then ONE seeded defect at a time; the same defect is pushed through the whole chain to the logits and compared
with the clean chain under max(1e-4, 2 E), the end-to-end bound of tests/test_gpu_resenc.py (E <= 7.9e-6: 1e-4 everywhere).

What was found (per layer: max against max(8e-6, 2 E_op), a join in units of its bound | logits against 1e-4):

  defect                                                                           per layer           end to end
  dec_noact     dec1.c0 reads its skip (the join enc1.b0) without the LeakyReLU    1.5e+0   caught     1.3e+0   caught
  c1_noact      enc1.b0.c1 reads the join enc0.b0 without the LeakyReLU            1.8e+0   caught     1.9e+0   caught
  join_raw      the join enc1.b0 adds the un-activated block input                 3.4e+6   caught     1.3e+0   caught
  img_stride    the join enc1.b0, (1, 2) window: image b reads its residual at
                b * HW instead of b * HW * 2 (B = 1: changes NOTHING)              8.6e+6   caught     2.7e+0   caught
  pool_T        the join enc1.b0 averages (y, 2x), (y + 1, 2x): (2, 1) for (1, 2)  6.1e+6   caught     2.7e+0   caught
  tile_stats    enc1.b0.proj of res_span: statistics per 128-row tile              8.6e-1   caught     6.6e-1   caught
  tail_zero     ... rows 512-575 (the partial last tile) left at zero              4.9e+0   caught     2.2e+0   caught
  c2_act        enc2.b0.c2 is activated                                            4.6e+0   caught     1.1e+0   caught
  eps_out       enc2.b0.proj normalised with 1 / (sqrt(var) + eps)                 2.3e-5   caught     1.5e-5   PASSES end to end
  c2_unbiased   enc3.b0.c2: InstanceNorm with variance * n / (n - 1), n = 32       1.6e-2   caught     7.1e-3   caught

Every seeded defect is caught per layer.  One stays below the end-to-end bound - ``eps_out`` on the projection's norm, by a factor 7: a kernel
with it passes tests/test_gpu_resenc.py; per layer it is caught by a factor 2.8, the narrowest margin of the list (on a channel whose
standard deviation is near 0.5 the defect vanishes to first order: tests/test_layer_check_cpu.py).  The others are caught end to end as well
on these nets; what the per-layer check adds for them is the name of the op - and, for ``img_stride``, the statement that the defect cannot be
seen at all with one image: rows (0, B - 1) of a B = 3 forward see it, row 0 alone does not.

(the figures of the table are printed by every case: ``pytest -s``; the classifications are what is asserted - DEFECTS below)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_oracle as O
from tests import layer_check as LC
from tests import resenc_util as R
from totalsegmentator2d_amd import weights
from totalsegmentator2d_amd.arch import OP_CONV3X3, OP_CONVT2X2, OP_HEAD1X1, OP_PROJ1X1, OP_JOIN

TOL = 1e-4                                   # tests/test_gpu_resenc.py: the logits within max(TOL, 2 E)
TILE = 128                                   # rows of the batch's pixels per M tile of pool_proj1x1 (csrc/dispatch.cpp, K_PROJ)


def _setup(case, B=None):
    arch, B0, H, W, seed = R.RES_CASES[case]
    return arch, weights.synthetic_state_dict(arch, seed), R.case_input(case, B)


@pytest.fixture(scope='module')
def nets():
    """case -> (arch, sd, shown tensors of the clean chain, E of the case)."""
    out = {}
    for case in ('res_win12', 'res_span'):
        arch, sd, x = _setup(case)
        out[case] = (arch, sd, chain32(arch, sd, x), R.oracle_logits(case)[1])
    return out


# ------------------------------------------------------------------------------------------------------------------ the stand-in engine
def _lrelu(t, slope):
    return F.leaky_relu(t, slope)


def op32(arch, sd, o, srcs, raw, defect=None):
    """ONE op of the program in fp32, written out so that a defect can be seeded.  `srcs`: the SHOWN tensors in ``layer_check.op_sources``
    order; `raw`: the stored (pre-activation) form of those of them that are joins, by the same index.  Returns (stored, shown) - they
    differ for a join only."""
    t = lambda k: O._t(sd[k])
    name, slope, eps = o['name'], arch.leaky_slope, arch.norm_eps
    hit = defect is not None and DEFECTS[defect][1] == name
    src = [O._t(s).float() for s in srcs]
    read = lambda i, act=True: src[i] if (act or raw[i] is None) else O._t(raw[i]).float()       # a reader that forgets the LeakyReLU of a join
    with torch.no_grad():
        if o['op'] == OP_HEAD1X1:
            y = F.conv2d(src[0], t(f'{o["key"]}.weight'), t(f'{o["key"]}.bias'))
            return y, y
        if o['op'] == OP_CONVT2X2:
            y = F.conv_transpose2d(src[0], t(f'{o["key"]}.weight'), t(f'{o["key"]}.bias'), stride=tuple(o['stride']))
            return y, y
        if o['op'] == OP_JOIN:
            c2 = src[0]
            r = read(1, act=not (hit and defect == 'join_raw'))
            sy, sx = o['stride']
            if (sy, sx) != (1, 1):
                Bn, C, Hi, Wi = r.shape
                if hit and defect == 'img_stride':       # pixel-major source, image b starts at b * HW (the stride of a (1, 1) window) instead of b * HW * sy * sx
                    HWo = (Hi // sy) * (Wi // sx)
                    flat = r.permute(0, 2, 3, 1).reshape(Bn * Hi * Wi, C)
                    r = torch.stack([flat[b * HWo:b * HWo + Hi * Wi].reshape(Hi, Wi, C).permute(2, 0, 1) for b in range(Bn)])
                if hit and defect == 'pool_T':           # the window's offsets transposed: (y, 2x) and (y + 1, 2x) instead of (y, 2x) and (y, 2x + 1)
                    assert (sy, sx) == (1, 2)
                    a = r[:, :, :, 0::2]
                    r = 0.5 * (a + torch.cat((a[:, :, 1:], a[:, :, -1:]), 2))
                else:
                    r = F.avg_pool2d(r, (sy, sx), (sy, sx))
            pre = c2 + r
            return pre, _lrelu(pre, slope)
        k = o['key']
        if o['op'] == OP_PROJ1X1:
            r = src[0]
            if tuple(o['stride']) != (1, 1):
                r = F.avg_pool2d(r, tuple(o['stride']), tuple(o['stride']))
            y = F.conv2d(r, t(f'{k}.conv.weight'))
            act = 1.0
        else:
            assert o['op'] == OP_CONV3X3
            if o['skip'] is not None:                    # a decoder entry: transposed conv of the coarse tensor, then cat((up, skip), 1)
                up_op = LC._program(arch)[o['src']]
                up = F.conv_transpose2d(src[0], t(f'{up_op["key"]}.weight'), t(f'{up_op["key"]}.bias'), stride=tuple(up_op['stride']))
                xin = torch.cat((up, read(1, act=not (hit and defect == 'dec_noact'))), 1)
            else:
                xin = read(0, act=not (hit and defect == 'c1_noact'))
            y = F.conv2d(xin, t(f'{k}.conv.weight'), t(f'{k}.conv.bias'), stride=tuple(o['stride']), padding=1)
            act = 1.0 if (o.get('linear') and not (hit and defect == 'c2_act')) else slope
        Bn, C, Hh, Ww = y.shape
        n = Hh * Ww
        if hit and defect == 'tail_zero':                # the rows of the partial last M tile are never written
            flat = y.permute(0, 2, 3, 1).reshape(Bn * n, C).clone()
            flat[(Bn * n) // TILE * TILE:] = 0
            y = flat.reshape(Bn, Hh, Ww, C).permute(0, 3, 1, 2)
        mean = y.mean((2, 3), keepdim=True)
        var = ((y - mean) ** 2).mean((2, 3), keepdim=True)
        if hit and defect == 'tile_stats':               # statistics per M tile (the batch's pixels numbered straight through) instead of per image
            flat = y.permute(0, 2, 3, 1).reshape(Bn * n, C)
            m_, v_ = torch.empty_like(flat), torch.empty_like(flat)
            for r0 in range(0, Bn * n, TILE):
                seg = flat[r0:r0 + TILE]
                m_[r0:r0 + TILE] = seg.mean(0, keepdim=True)
                v_[r0:r0 + TILE] = ((seg - seg.mean(0, keepdim=True)) ** 2).mean(0, keepdim=True)
            mean, var = (a.reshape(Bn, Hh, Ww, C).permute(0, 3, 1, 2) for a in (m_, v_))
        if hit and defect == 'c2_unbiased':
            var = var * (n / (n - 1.0))
        rstd = 1.0 / (var.sqrt() + eps) if (hit and defect == 'eps_out') else 1.0 / (var + eps).sqrt()
        out = (y - mean) * rstd * t(f'{k}.norm.weight')[None, :, None, None] + t(f'{k}.norm.bias')[None, :, None, None]
        out = _lrelu(out, act)
        return out, out


def chain32(arch, sd, x, defect=None):
    """The whole program through :func:`op32`: {name: shown tensor} with 'input' and 'head'; a composed-away ``.up`` is evaluated inside
    its ``decL.c0`` (as ``layer_forward`` does) and on its own."""
    shown, stored = {'input': x}, {}
    for o in arch.program():
        n = o['name']
        names = LC.op_sources(arch, n)
        st, sh = op32(arch, sd, o, [shown[s] for s in names], [stored.get(s) for s in names], defect)
        shown[n] = sh.numpy()
        if o['op'] == OP_JOIN:
            stored[n] = st.numpy()
    return shown


def _judge(arch, sd, name, got, srcs, rows):
    want = LC.reference_block(arch, sd, name, srcs, 'split')
    bound, e_op = LC._res_terms(arch, sd, name, srcs, want)
    r = list(rows)
    return LC.layer_error(name, got[r], want[r], 'split', bound=None if bound is None else bound[r], e_op=e_op)


# defect -> (case, the op it sits in, caught per layer?, stays under the end-to-end bound?)
DEFECTS = {
    'dec_noact': ('res_win12', 'dec1.c0', True, False),
    'c1_noact': ('res_win12', 'enc1.b0.c1', True, False),
    'join_raw': ('res_win12', 'enc1.b0', True, False),
    'img_stride': ('res_win12', 'enc1.b0', True, False),
    'pool_T': ('res_win12', 'enc1.b0', True, False),
    'tile_stats': ('res_span', 'enc1.b0.proj', True, False),
    'tail_zero': ('res_span', 'enc1.b0.proj', True, False),
    'c2_act': ('res_win12', 'enc2.b0.c2', True, False),
    'eps_out': ('res_win12', 'enc2.b0.proj', True, True),
    'c2_unbiased': ('res_win12', 'enc3.b0.c2', True, False),
}


# ------------------------------------------------------------------------------------------------------------------ the clean chain passes
def test_the_cases_have_the_shapes_the_defects_need(nets):
    arch, _, shown, _ = nets['res_win12']
    prog = LC._program(arch)
    assert shown['input'].shape[0] == 3
    assert prog['enc1.b0']['stride'] == (1, 2) and prog['enc1.b0']['res'] == 'enc0.b0'           # a pool-only join behind (1, 2), reading a join
    assert prog['enc2.b0.proj']['stride'] == (2, 1) and prog['enc3.b0']['stride'] == (2, 2) and prog['enc3.b0']['res'] == 'enc2.b0'
    assert LC.op_sources(arch, 'dec1.c0') == ('dec2.c1', 'enc1.b0') and LC.op_sources(arch, 'head') == ('dec0.c1',)
    assert LC.op_sources(arch, 'dec2.c0') == ('enc3.b0', 'enc2.b0') and LC.op_sources(arch, 'enc1.b0.c1') == ('enc0.b0',)
    arch, _, shown, _ = nets['res_span']
    p = shown['enc1.b0.proj']
    M = p.shape[0] * p.shape[2] * p.shape[3]
    assert p.shape[2] * p.shape[3] == 192 and M == 576 and M % TILE == 64 and 192 % TILE != 0    # seams inside tiles, a partial last tile


@pytest.mark.parametrize('case', ['res_win12', 'res_span'])
def test_clean_fp32_ops_pass_the_layer_bound_none_excluded(nets, case):
    arch, sd, shown, _ = nets[case]
    B = shown['input'].shape[0]
    bad, worst = [], {}
    for o in arch.program():
        n = o['name']
        ok, w, text = _judge(arch, sd, n, shown[n], [shown[s] for s in LC.op_sources(arch, n)], (0, B - 1))
        worst[n] = w
        if not ok:
            bad.append(text)
    print(f'[layer-check-resenc-cpu] clean {case}: ' + ', '.join(f'{n} {w:.2e}' for n, w in worst.items()))
    assert not bad, bad
    assert len(worst) == len(arch.program())


@pytest.mark.parametrize('case', ['res_win12', 'res_span'])
def test_the_written_out_chain_is_the_torch_restatement(nets, case):
    """chain32 without a defect against resenc_forward (F.instance_norm): the same net to fp32 rounding, so that what a seeded defect
    changes is the defect alone."""
    arch, sd, shown, _ = nets[case]
    lg, inter = R.resenc_forward(arch, sd, shown['input'], return_intermediates=True)
    for n, v in inter.items():
        assert np.abs(shown[n] - v.numpy()).max() <= 3e-5, n     # (two fp32 chains: the bound tests/test_gpu_parity.py uses between two paths)
    assert np.abs(shown['head'] - lg.numpy()).max() <= 3e-5


# ------------------------------------------------------------------------------------------------------------------ the seeded defects
@pytest.mark.parametrize('defect', list(DEFECTS))
def test_seeded_defect(nets, defect):
    case, name, caught, passes_e2e = DEFECTS[defect]
    arch, sd, shown, E = nets[case]
    B = shown['input'].shape[0]
    prog = LC._program(arch)
    names = LC.op_sources(arch, name)
    srcs = [shown[s] for s in names]
    raw = [None] * len(names)
    for i, s in enumerate(names):                         # the stored form of a join: the pre-activation sum (the inverse of an exact LeakyReLU product
        if s in prog and prog[s]['op'] == OP_JOIN:        # is not exact - take it from the chain's own join)
            raw[i] = op32(arch, sd, prog[s], [shown[q] for q in LC.op_sources(arch, s)], [None, None])[0].numpy()
    clean = op32(arch, sd, prog[name], srcs, raw)[1].numpy()
    ok0, w0, text0 = _judge(arch, sd, name, clean, srcs, (0, B - 1))
    assert ok0, ('the clean op must pass', text0)
    got = op32(arch, sd, prog[name], srcs, raw, defect)[1].numpy()
    assert not np.array_equal(got, clean), 'the defect changed nothing'
    ok, w, text = _judge(arch, sd, name, got, srcs, (0, B - 1))
    e2e = float(np.abs(chain32(arch, sd, shown['input'], defect)['head'] - shown['head']).max())
    under = e2e <= max(TOL, 2 * E)
    print(f'[layer-check-resenc-cpu] {defect} in {case} {name}: per layer {text} (clean {w0:.2e}) -> {"caught" if not ok else "NOT caught"}; '
          f'logits {e2e:.2e} (bound {max(TOL, 2 * E):.1e}) -> {"passes" if under else "caught"} end to end')
    assert (not ok) == caught, text
    assert under == passes_e2e, e2e


def test_the_image_stride_defect_is_invisible_with_one_image_and_caught_with_three(nets):
    """Why the anisotropic windows run at B = 3: with one image the term ``b * HW * (sy * sx)`` is 0 whatever the factor."""
    arch, sd, x1 = _setup('res_win12', B=1)
    clean, bad = chain32(arch, sd, x1), chain32(arch, sd, x1, 'img_stride')
    assert all(np.array_equal(clean[n], bad[n]) for n in clean)                 # B = 1: every tensor, bit for bit
    _, _, shown, _ = nets['res_win12']
    bad3 = chain32(arch, sd, shown['input'], 'img_stride')
    assert np.array_equal(bad3['enc1.b0'][0], shown['enc1.b0'][0]) and not np.array_equal(bad3['enc1.b0'][2], shown['enc1.b0'][2])
    ok, _, text = _judge(arch, sd, 'enc1.b0', bad3['enc1.b0'], [shown['enc1.b0.c2'], shown['enc0.b0']], (0, 2))
    assert not ok, text
    ok, _, text = _judge(arch, sd, 'enc1.b0', bad3['enc1.b0'], [shown['enc1.b0.c2'], shown['enc0.b0']], (0,))
    assert ok, text                                                              # row 0 alone would not see it: rows (0, B - 1)


def test_the_argument_for_per_layer_bounds():
    """Every seeded defect is caught per layer; at least one of them passes end to end."""
    assert all(v[2] for v in DEFECTS.values())
    assert sum(v[3] for v in DEFECTS.values()) >= 1
