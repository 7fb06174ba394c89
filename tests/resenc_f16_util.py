"""TEST INFRASTRUCTURE (never imported by the product): the 16-bit contract of a ResidualEncoderUNet (include/ts2d_engine.h, beside
``TS2D_PRECISION_F16``) restated in torch on the CPU, mirroring tests/resenc_util.py.  Built from ``oracle.torch_oracle.conv_block(emulate='f16')``,
``O._h``, ``F.avg_pool2d``, ``F.conv2d`` and ``F.instance_norm``; oracle/ is imported, never edited.

Notation: ``h(.)`` = ``O._h`` rounds to IEEE half and back; :func:`act16` ``(y) = max(y, h(y * h(slope)))`` for a half value y.

* stem, conv1, decoder blocks: ``conv_block(emulate='f16')`` (the stem with ``round_w=False``); the operand the next op multiplies is
  ``a = act16(h(n))``, n = the fp32 normalisation of the STORED half conv output.  (The block is asked for n itself - its storage view under
  slope 1, which is the identity - and the operand rounding is applied here, so that both roundings go through ``O._h`` and :func:`act16`
  of THIS module: tests/test_resenc_f16_cpu.py replaces them by the identity and ``leaky_relu`` and gets tests/resenc_util.resenc_forward back.)
* conv2: stored ``y2 = h(conv(a, h(w)) + b)``, statistics in fp32 over the stored values, ``n2`` kept in fp32.
* residual r, fp32: identity ``r = a``; pooled ``F.avg_pool2d(a)``; projection ``p = h(conv1x1(h(pool(a)), h(w)))``, ``r = instance_norm(p)``.
* join: ``t = h(n2 + r)``, one rounding; every consumer multiplies ``act16(t)``.
* transposed conv: ``h(convT(a, h(w)) + b)``, multiplied as stored; head: ``conv1x1(a, h(w)) + b`` in fp32.

Two views of a tensor, as in ``conv_block``: the OPERAND (what a consumer multiplies: ``act16(h(n))``, ``act16(t)``) and the STORAGE VIEW (what
``Engine.debug_tensor`` shows: ``leaky_relu(n)`` / ``leaky_relu(t)`` in fp32; a linear tensor - conv2, projection - is n in both).
:func:`operand_from_view` goes from the second to the first.

``acc64=True`` is the bounds twin of tests/test_resenc_f16_cpu.py: every conv (3x3, 1x1, transposed, head) accumulates in float64 before the half
rounding, and a join pools and sums in float64 before its one rounding - another correct summation order of the same contract."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import resenc_util as R                           # noqa: E402


def act16(y, slope):
    """LeakyReLU of a half value as the 16-bit consumers do it at load time: ``max(y, h(y * h(slope)))``."""
    import torch
    from oracle import torch_oracle as O
    s16 = float(torch.tensor(slope, dtype=torch.float16))
    return torch.maximum(y, O._h(y * s16))


def operand(n, slope):
    """The operand a consumer multiplies, from the fp32 normalised value n of a conv block (or the half sum t of a join: h(t) = t)."""
    from oracle import torch_oracle as O
    return act16(O._h(n), slope)


def pre_activation(view, slope):
    """n (or t) from the storage view ``leaky_relu(n)``: the view itself where it is positive, else view / slope in fp32.  Exact for a join
    (t is a half: h() of the quotient snaps back onto it); for a conv block within an fp32 ulp or two of the engine's own n."""
    import torch
    from oracle import torch_oracle as O
    v = O._t(np.asarray(view, np.float32) if not isinstance(view, torch.Tensor) else view).to(torch.float32)
    return torch.where(v >= 0, v, v / torch.tensor(slope, dtype=torch.float32))


def operand_from_view(view, slope, nudge=0.0):
    """The operand of a tensor from its storage view.  `nudge`: n is moved by ``nudge * max(1, |n|)`` first - the two operands an accessor
    value within that distance of a half rounding tie is compatible with (tests/test_gpu_resenc_f16.py, joins)."""
    import torch
    n = pre_activation(view, slope)
    if nudge:
        n = n + nudge * torch.clamp(n.abs(), min=1.0)
    return operand(n, slope)


def _conv(x, w, b, stride, padding, acc64):
    import torch.nn.functional as F
    if acc64:
        return F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=stride, padding=padding).float()
    return F.conv2d(x, w, b, stride=stride, padding=padding)


def conv_norm16(t, key, a, stride, eps, round_w=True, acc64=False):
    """n of ``ConvDropoutNormReLU`` under prefix `key` from the operand `a`: the fp32 InstanceNorm of the stored half conv output."""
    import torch.nn.functional as F
    from oracle import torch_oracle as O
    w, b, g, be = (t[f'{key}.conv.weight'], t[f'{key}.conv.bias'], t[f'{key}.norm.weight'], t[f'{key}.norm.bias'])
    if not acc64:       # (slope 1: the block's storage view is the normalised value itself, bit for bit)
        return O.conv_block(a, w, b, g, be, stride, eps, 1.0, emulate='f16', round_w=round_w, storage_view=True)
    y = O._h(_conv(a, O._h(w) if round_w else w, b, stride, 1, True))
    return F.instance_norm(y, None, None, g, be, use_input_stats=True, momentum=0.1, eps=eps)


def pool_proj16(t, key, a, pool, eps, acc64=False):
    """The normalised projection (fp32, not rounded) from the block input's operand: AvgPool2d -> h -> Conv 1x1 with h(w), no bias -> h -> norm."""
    import torch.nn.functional as F
    from oracle import torch_oracle as O
    r = a
    if pool and tuple(pool) != (1, 1):
        r = F.avg_pool2d(r, tuple(pool), tuple(pool))
    p = O._h(_conv(O._h(r), O._h(t[f'{key}.conv.weight']), None, 1, 0, acc64))
    return F.instance_norm(p, None, None, t[f'{key}.norm.weight'], t[f'{key}.norm.bias'], use_input_stats=True, momentum=0.1, eps=eps)


def _tensors(sd):
    import torch
    from oracle import torch_oracle as O
    return {k: O._t(v).to(torch.float32) for k, v in sd.items()}


def block_forward_f16(arch, sd, s, b, x=None, c1=None, c2=None, proj=None, storage_view=False, acc64=False, nudge=0.0,
                      ops=('c1', 'c2', 'proj', 'out')):
    """One BasicBlockD under the 16-bit contract: dict with c1, c2, proj (None without a projection), r (what the join adds, fp32), out, and
    t (the join's stored half sum) and n1 (conv1 normalised, fp32).  `ops`: the ops to evaluate (the entries of the others are None; r and t go with 'out').
    `x`: the block's input.  `c1`, `c2`, `proj`: given, they stand for the block's own value of that tensor in every op that READS it (c2 from a
    given c1, the join from given c2 / proj - each op of the engine fed with the engine's own inputs; `x` may then be None where no evaluated
    op reads it); the returned entries are always this function's own results.
    ``storage_view=False``: `x` and a given `c1` are operands, and c1 / out are returned as operands.
    ``storage_view=True``: `x` and a given `c1` are storage views (``Engine.debug_tensor``) and c1 / out are returned as storage views.
    c2 and proj are normalised fp32 values in both.  `nudge`: see :func:`operand_from_view` (applies to `x` where the join adds it)."""
    import torch
    import torch.nn.functional as F
    from oracle import torch_oracle as O
    t = _tensors(sd)
    k = R.block_keys(s, b)
    stride, pool, pk = R.skip_layout(arch, s, b)
    eps, slope = arch.norm_eps, arch.leaky_slope
    f32 = lambda v: O._t(np.asarray(v, np.float32) if not isinstance(v, torch.Tensor) else v).to(torch.float32)
    res = dict(c1=None, c2=None, proj=None, r=None, out=None, t=None, n1=None)
    with torch.no_grad():
        a = None if x is None else (operand_from_view(x, slope) if storage_view else f32(x))
        a1 = None if c1 is None else (operand_from_view(c1, slope) if storage_view else f32(c1))
        if 'c1' in ops:
            n1 = conv_norm16(t, f'{k}.conv1', a, stride, eps, acc64=acc64)
            res['c1'], res['n1'] = F.leaky_relu(n1, slope) if storage_view else operand(n1, slope), n1
            a1 = operand(n1, slope) if a1 is None else a1
        if 'c2' in ops:
            res['c2'] = conv_norm16(t, f'{k}.conv2', a1, 1, eps, acc64=acc64)
        if 'proj' in ops and pk:
            res['proj'] = pool_proj16(t, pk, a, pool, eps, acc64=acc64)
        if 'out' in ops:
            n2 = res['c2'] if c2 is None else f32(c2)
            if pk:
                r = res['proj'] if proj is None else f32(proj)
            else:
                r = operand_from_view(x, slope, nudge) if (storage_view and nudge) else a
                if pool:
                    r = F.avg_pool2d(r.double(), pool, pool).float() if acc64 else F.avg_pool2d(r, pool, pool)
            # (the twin: the sum formed in float64 and rounded to half once - numpy's float64 -> float16 is one rounding, torch's goes through float32)
            tt = torch.from_numpy((n2.double() + r.double()).numpy().astype(np.float16).astype(np.float32)) if acc64 else O._h(n2 + r)
            res.update(r=r, t=tt, out=F.leaky_relu(tt, slope) if storage_view else act16(tt, slope))
    return res


def up16(t, key, a, stride, acc64=False):
    """The transposed conv: ``h(convT(a, h(w)) + b)`` - stored as half, multiplied as stored."""
    import torch.nn.functional as F
    from oracle import torch_oracle as O
    w, b = O._h(t[f'{key}.weight']), t[f'{key}.bias']
    if acc64:
        return O._h(F.conv_transpose2d(a.double(), w.double(), b.double(), stride=stride).float())
    return O._h(F.conv_transpose2d(a, w, b, stride=stride))


def resenc_forward_f16(arch, sd, x, return_intermediates=False, acc64=False):
    """``ResidualEncoderUNet.forward`` under the 16-bit contract.  x: [B, C, H, W] fp32.  Intermediates by the engine's tensor names, in the
    storage view; a join also as ``<name>.t`` (the stored half sum) and ``<name>.x`` (the operand of the block's
    input)."""
    import torch
    import torch.nn.functional as F
    from oracle import torch_oracle as O
    t = _tensors(sd)
    x = O._t(x).to(torch.float32)
    inter, skips = {}, []
    eps, slope = arch.norm_eps, arch.leaky_slope
    with torch.no_grad():
        n = conv_norm16(t, 'encoder.stem.convs.0', x, 1, eps, round_w=False, acc64=acc64)
        inter['stem'] = F.leaky_relu(n, slope)
        a = operand(n, slope)
        for s in range(arch.n_stages):
            for b in range(arch.n_blocks_per_stage[s]):
                blk = block_forward_f16(arch, t, s, b, a, acc64=acc64)
                nm = f'enc{s}.b{b}'
                inter[f'{nm}.x'], inter[f'{nm}.c1'] = a, F.leaky_relu(blk['n1'], slope)
                inter[f'{nm}.c2'], inter[f'{nm}.t'], inter[nm] = blk['c2'], blk['t'], F.leaky_relu(blk['t'], slope)
                if blk['proj'] is not None:
                    inter[f'{nm}.proj'] = blk['proj']
                a = blk['out']
            skips.append(a)
        for j in range(arch.n_stages - 1):
            lvl = arch.n_stages - 2 - j
            u = up16(t, f'decoder.transpconvs.{j}', a, tuple(arch.strides[lvl + 1]), acc64)
            inter[f'dec{lvl}.up'] = u
            a = torch.cat((u, skips[lvl]), 1)
            for i in range(arch.n_conv_per_stage_decoder[j]):
                n = conv_norm16(t, f'decoder.stages.{j}.convs.{i}', a, 1, eps, acc64=acc64)
                inter[f'dec{lvl}.c{i}'] = F.leaky_relu(n, slope)
                a = operand(n, slope)
        k = f'decoder.seg_layers.{arch.n_stages - 2}'
        y = _conv(a, O._h(t[f'{k}.weight']), t[f'{k}.bias'], 1, 0, acc64)
    return (y, inter) if return_intermediates else y


def op_reference(arch, sd, name, srcs, nudge=0.0):
    """Op `name` of ``arch.program()`` under the 16-bit contract from the storage views `srcs` of the tensors it reads (tests/layer_check.py
    ``op_sources`` order: (src,), a join (conv2, what it adds), ``decL.c0`` (coarse, skip)), in the storage view, as float64 numpy.  The network
    input enters the stem as it is.  For a join also its stored half sum: (view, t)."""
    import torch
    import torch.nn.functional as F
    from oracle import torch_oracle as O
    from tests import layer_check as LC
    prog = {o['name']: o for o in arch.program()}
    o = prog[name]
    t = _tensors(sd)
    eps, slope = arch.norm_eps, arch.leaky_slope
    out = lambda v: v.numpy().astype(np.float64)
    with torch.no_grad():
        if name == 'stem':
            x = O._t(np.asarray(srcs[0], np.float32)).to(torch.float32)
            return out(F.leaky_relu(conv_norm16(t, o['key'], x, 1, eps, round_w=False), slope))
        if name.startswith('enc'):                      # an op of a block: block_forward_f16 on the engine's own inputs of that op
            sb = (int(name[3:name.index('.')]), int(name.split('.')[1][1:]))
            blk = lambda **kw: block_forward_f16(arch, t, *sb, storage_view=True, **kw)
            if o['op'] == LC.OP_JOIN:
                lin = prog[o['res']]['op'] == LC.OP_PROJ1X1
                r = blk(x=None if lin else srcs[1], c2=srcs[0], proj=srcs[1] if lin else None, nudge=nudge, ops=('out',))
                return out(r['out']), out(r['t'])
            if o['op'] == LC.OP_PROJ1X1:
                return out(blk(x=srcs[0], ops=('proj',))['proj'])
            return out(blk(c1=srcs[0], ops=('c2',))['c2'] if o['linear'] else blk(x=srcs[0], ops=('c1',))['c1'])
        a = operand_from_view(srcs[0], slope)
        if o['op'] == LC.OP_CONVT2X2:
            return out(up16(t, o['key'], a, tuple(o['stride'])))
        if o['op'] == LC.OP_HEAD1X1:
            return out(_conv(a, O._h(t[f"{o['key']}.weight"]), t[f"{o['key']}.bias"], 1, 0, False))
        if o['skip'] is not None:                       # decoder entry: (coarse, skip) -> transposed conv -> cat -> block
            up = prog[o['src']]
            a = torch.cat((up16(t, up['key'], a, tuple(up['stride'])), operand_from_view(srcs[1], slope)), 1)
        return out(F.leaky_relu(conv_norm16(t, o['key'], a, 1, eps), slope))
