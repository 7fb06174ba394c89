"""TEST INFRASTRUCTURE (never imported by the product): nnU-Net's ``ResidualEncoderUNet`` (2-D, ``BasicBlockD``) restated twice, and the
parity cases of the residual encoder.

Upstream's ``dynamic_network_architectures`` is not a dependency of this repository, so the network is pinned here:

* :func:`resenc_forward` - functional torch, built on ``oracle.torch_oracle.conv_block`` (Conv 3x3 -> InstanceNorm -> LeakyReLU) and
  ``F.avg_pool2d`` / ``F.conv2d`` / ``F.instance_norm`` for the skip path, with the decoder loop of ``oracle.torch_oracle.unet_forward``;
* :func:`build_replica` - an ``nn.Module`` tree with upstream's attribute names (``encoder.stem.convs``, ``encoder.stages[s].blocks[b]
  .conv1 / conv2 / skip``, ``decoder.transpconvs / stages / seg_layers``), built from ``torch.nn`` layers only, so that
  ``load_state_dict(strict=True)`` checks every key ``UNetArch.param_specs`` names and nothing else.

A block: ``out = lrelu(conv2(conv1(x)) + skip(x))``; conv1 = Conv 3x3 (stride) + bias, norm, LeakyReLU; conv2 = Conv 3x3 + bias, norm, no
non-linearity; skip = identity, or ``AvgPool2d(stride)`` where a stride differs from 1, then Conv 1x1 (no bias) + norm where the widths differ."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from totalsegmentator2d_amd.arch import UNetArch             # noqa: E402
from tests import cases                                      # noqa: E402


def resunet(feats, blocks, K, cin=2, nconv_dec=2, strides=None):
    n = len(feats)
    strides = ((1, 1),) + ((2, 2),) * (n - 1) if strides is None else tuple(tuple(s) for s in strides)
    return UNetArch(input_channels=cin, num_classes=K, n_stages=n, features_per_stage=tuple(feats), kernel_sizes=((3, 3),) * n,
                    strides=strides, n_conv_per_stage=(1,) * n, n_conv_per_stage_decoder=(nconv_dec,) * (n - 1),
                    encoder='residual', n_blocks_per_stage=tuple(blocks))


# name -> (arch, B, H, W, seed); inputs: cases.make_input
RES_CASES = {
    # stem, identity join, pool + projection
    'res_min': (resunet((32, 64), (1, 1), 3), 2, 32, 64, 31),
    # pool-only skip (64 -> 64 under a stride), identity joins in a strided stage, odd batch
    'res_pool': (resunet((32, 64, 64), (1, 2, 2), 5), 3, 32, 48, 32),
    # (1, 2) window, pool-only 64 -> 64, a projection without a pool (64 -> 96 at stride (1, 1))
    'res_aniso': (resunet((32, 64, 64, 96), (2, 1, 1, 1), 4, strides=((1, 1), (1, 2), (2, 2), (1, 1))), 1, 16, 64, 33),
    # (2, 1) window, pool-only
    'res_aniso21': (resunet((32, 64, 128, 128), (1, 1, 1, 1), 5, strides=((1, 1), (2, 2), (2, 2), (2, 1))), 1, 32, 64, 34),
    # 2 x 4 bottleneck: several images per tile in both new kernels
    'res_tiny': (resunet((32, 64, 64, 96), (1, 1, 1, 1), 4), 5, 16, 32, 35),
    # widths that are no multiple of 32 (the caller's blob is widened segment by segment), one input channel, non-power-of-two extent
    'res_pad': (resunet((24, 40, 72), (1, 2, 1), 26, cin=1), 1, 48, 80, 36),
    # K = 256 -> 512 projection; the 16 x 32-tile and the composed kernels read join outputs
    'res_deep': (resunet((32, 64, 128, 256, 512), (1, 2, 2, 2, 2), 18, nconv_dec=1), 2, 128, 128, 37),
    # projection tiles that span images: level 1 is 8 x 24 = 192 pixels (M = 576: 4.5 tiles of 128 rows, the image seams inside tiles, a partial
    # last tile, 64 columns, pooled), level 2 is 4 x 12 = 48 pixels (M = 144: two tiles, 32 columns); statistics by stats_direct
    'res_span': (resunet((32, 64, 96), (1, 1, 1), 4), 3, 16, 48, 41),
    # per-axis windows at B = 3: a pool-only join behind a (1, 2) window, a projection behind a (2, 1) window, a pool-only (2, 2) join
    'res_win12': (resunet((32, 32, 64, 64), (1, 1, 1, 1), 5, strides=((1, 1), (1, 2), (2, 1), (2, 2))), 3, 32, 64, 42),
    # ... the other way round at B = 2: pool-only (2, 1), a projection behind (1, 2), identity joins inside a (2, 1) stage
    'res_win21': (resunet((32, 32, 64, 64), (1, 2, 1, 1), 5, strides=((1, 1), (2, 1), (1, 2), (2, 2))), 2, 32, 64, 43),
}


def case_input(name, B=None):
    """The input of a case; `B`: at another batch size (the same PRNG stream, so that the first rows agree)."""
    arch, B0, H, W, seed = RES_CASES[name]
    return cases.make_input(arch, B0 if B is None else B, H, W, seed)


def block_keys(s, b):
    return f'encoder.stages.{s}.blocks.{b}'


def skip_layout(arch, s, b):
    """(pool window or None, key of the projection or None) of block b of stage s."""
    stride = tuple(int(v) for v in arch.strides[s]) if (b == 0 and s > 0) else (1, 1)
    cin = arch.features_per_stage[s - 1] if (b == 0 and s > 0) else arch.features_per_stage[s]
    pool = stride if stride != (1, 1) else None
    proj = f'{block_keys(s, b)}.skip.{1 if pool else 0}' if cin != arch.features_per_stage[s] else None
    return stride, pool, proj


def conv_norm(sd, key, x, stride, eps, slope, dtype=None):
    """``ConvDropoutNormReLU`` under state-dict prefix `key` from its (activated) input: Conv 3x3 (stride) + bias -> InstanceNorm ->
    LeakyReLU(slope); slope 1.0: no non-linearity (a LeakyReLU of slope 1 is the identity, bit for bit).  ``dtype=torch.float64``: every
    operation in double precision."""
    import torch
    from oracle import torch_oracle as O
    t = lambda k: O._t(sd[k]) if dtype is None else O._t(sd[k]).to(dtype)
    x = O._t(x) if dtype is None else O._t(x).to(dtype)
    with torch.no_grad():
        return O.conv_block(x, t(f'{key}.conv.weight'), t(f'{key}.conv.bias'), t(f'{key}.norm.weight'), t(f'{key}.norm.bias'), stride, eps, slope)


def pool_proj(sd, key, x, pool, eps, dtype=None):
    """The skip path where the widths differ, from the block's (activated) input: ``AvgPool2d(pool)`` (None or (1, 1): no pool) -> Conv 1x1
    without bias under prefix `key` -> InstanceNorm, no non-linearity."""
    import torch
    import torch.nn.functional as F
    from oracle import torch_oracle as O
    t = lambda k: O._t(sd[k]) if dtype is None else O._t(sd[k]).to(dtype)
    r = O._t(x) if dtype is None else O._t(x).to(dtype)
    with torch.no_grad():
        if pool and tuple(pool) != (1, 1):
            r = F.avg_pool2d(r, tuple(pool), tuple(pool))
        p = F.conv2d(r, t(f'{key}.conv.weight'))
        return F.instance_norm(p, None, None, t(f'{key}.norm.weight'), t(f'{key}.norm.bias'), use_input_stats=True, momentum=0.1, eps=eps)


def block_forward(arch, sd, s, b, x, dtype=None):
    """One BasicBlockD from its (activated) input: dict with c1 (activated), c2 and proj (normalised, not activated; proj None without a
    projection), r (what the join adds) and out.  ``dtype=torch.float64``: every operation in double precision."""
    import torch
    import torch.nn.functional as F
    from oracle import torch_oracle as O
    k = block_keys(s, b)
    stride, pool, proj = skip_layout(arch, s, b)
    x = O._t(x) if dtype is None else O._t(x).to(dtype)
    eps, slope = arch.norm_eps, arch.leaky_slope
    with torch.no_grad():
        c1 = conv_norm(sd, f'{k}.conv1', x, stride, eps, slope, dtype)
        c2 = conv_norm(sd, f'{k}.conv2', c1, 1, eps, 1.0, dtype)
        r = x
        if pool:
            r = F.avg_pool2d(r, pool, pool)
        p = None
        if proj:
            p = pool_proj(sd, proj, x, pool, eps, dtype)
            r = p
        out = F.leaky_relu(c2 + r, slope)
    return dict(c1=c1, c2=c2, proj=p, r=r, out=out)


def resenc_forward(arch, sd, x, return_intermediates=False, dtype=None):
    """``ResidualEncoderUNet.forward`` (deep supervision off).  x: [B, C, H, W].  Intermediates by the engine's tensor names."""
    import torch
    import torch.nn.functional as F
    from oracle import torch_oracle as O
    dt = torch.float32 if dtype is None else dtype
    t = {k: O._t(v).to(dt) for k, v in sd.items()}
    x = O._t(x).to(dt)
    inter, skips = {}, []
    eps, slope = arch.norm_eps, arch.leaky_slope
    with torch.no_grad():
        k = 'encoder.stem.convs.0'
        x = O.conv_block(x, t[f'{k}.conv.weight'], t[f'{k}.conv.bias'], t[f'{k}.norm.weight'], t[f'{k}.norm.bias'], 1, eps, slope)
        inter['stem'] = x
        for s in range(arch.n_stages):
            for b in range(arch.n_blocks_per_stage[s]):
                blk = block_forward(arch, t, s, b, x, dtype=dt)
                nm = f'enc{s}.b{b}'
                inter[f'{nm}.c1'], inter[f'{nm}.c2'], inter[nm] = blk['c1'], blk['c2'], blk['out']
                if blk['proj'] is not None:
                    inter[f'{nm}.proj'] = blk['proj']
                x = blk['out']
            skips.append(x)
        for j in range(arch.n_stages - 1):
            lvl = arch.n_stages - 2 - j
            k = f'decoder.transpconvs.{j}'
            x = F.conv_transpose2d(x, t[f'{k}.weight'], t[f'{k}.bias'], stride=tuple(arch.strides[lvl + 1]))
            inter[f'dec{lvl}.up'] = x
            x = torch.cat((x, skips[lvl]), 1)
            for i in range(arch.n_conv_per_stage_decoder[j]):
                k = f'decoder.stages.{j}.convs.{i}'
                x = O.conv_block(x, t[f'{k}.conv.weight'], t[f'{k}.conv.bias'], t[f'{k}.norm.weight'], t[f'{k}.norm.bias'], 1, eps, slope)
                inter[f'dec{lvl}.c{i}'] = x
        k = f'decoder.seg_layers.{arch.n_stages - 2}'
        x = F.conv2d(x, t[f'{k}.weight'], t[f'{k}.bias'])
    return (x, inter) if return_intermediates else x


_memo = {}


def oracle_logits(name):
    """(float32 logits, E) of a case: the float32 oracle on the CPU, and its own error against the float64 evaluation.  Computed once."""
    if name not in _memo:
        from totalsegmentator2d_amd import weights
        arch, B, H, W, seed = RES_CASES[name]
        sd = weights.synthetic_state_dict(arch, seed)
        x = case_input(name)
        y32 = resenc_forward(arch, sd, x).numpy()
        import torch
        y64 = resenc_forward(arch, sd, x, dtype=torch.float64).numpy()
        _memo[name] = (y32, float(np.abs(y32.astype(np.float64) - y64).max()))
    return _memo[name]


# ------------------------------------------------------------------------------------------------ the module replica
def build_replica(arch):
    """``nn.Module`` with upstream's attribute names, from ``torch.nn`` layers only."""
    import torch
    from torch import nn
    eps, slope = arch.norm_eps, arch.leaky_slope

    class ConvNormAct(nn.Module):                       # upstream ConvDropoutNormReLU: attributes conv, norm, nonlin
        def __init__(self, ci, co, k, stride, bias, act):
            super().__init__()
            self.conv = nn.Conv2d(ci, co, k, stride, padding=(k - 1) // 2, bias=bias)
            self.norm = nn.InstanceNorm2d(co, eps=eps, affine=True)
            self.nonlin = nn.LeakyReLU(slope) if act else None

        def forward(self, x):
            x = self.norm(self.conv(x))
            return self.nonlin(x) if self.nonlin is not None else x

    class BasicBlockD(nn.Module):
        def __init__(self, ci, co, stride):
            super().__init__()
            self.conv1 = ConvNormAct(ci, co, 3, stride, True, True)
            self.conv2 = ConvNormAct(co, co, 3, 1, True, False)
            self.nonlin2 = nn.LeakyReLU(slope)
            ops = []
            if tuple(stride) != (1, 1):
                ops.append(nn.AvgPool2d(stride, stride))
            if ci != co:
                ops.append(ConvNormAct(ci, co, 1, 1, False, False))
            self.skip = nn.Sequential(*ops) if ops else (lambda x: x)

        def forward(self, x):
            return self.nonlin2(self.conv2(self.conv1(x)) + self.skip(x))

    class Stage(nn.Module):                              # upstream StackedResidualBlocks: attribute blocks
        def __init__(self, ci, co, stride, n):
            super().__init__()
            self.blocks = nn.Sequential(*[BasicBlockD(ci if b == 0 else co, co, stride if b == 0 else (1, 1)) for b in range(n)])

        def forward(self, x):
            return self.blocks(x)

    class Stacked(nn.Module):                            # upstream StackedConvBlocks: attribute convs
        def __init__(self, ci, co, n):
            super().__init__()
            self.convs = nn.Sequential(*[ConvNormAct(ci if i == 0 else co, co, 3, 1, True, True) for i in range(n)])

        def forward(self, x):
            return self.convs(x)

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            f = arch.features_per_stage
            self.stem = Stacked(arch.input_channels, f[0], 1)
            self.stages = nn.Sequential(*[Stage(f[s - 1] if s else f[0], f[s], tuple(arch.strides[s]) if s else (1, 1), arch.n_blocks_per_stage[s])
                                          for s in range(arch.n_stages)])

        def forward(self, x):
            x = self.stem(x)
            out = []
            for st in self.stages:
                x = st(x)
                out.append(x)
            return out

    class Decoder(nn.Module):
        def __init__(self):
            super().__init__()
            f, n = arch.features_per_stage, arch.n_stages
            self.transpconvs = nn.ModuleList([nn.ConvTranspose2d(f[n - 1 - j], f[n - 2 - j], tuple(arch.strides[n - 1 - j]), tuple(arch.strides[n - 1 - j]))
                                              for j in range(n - 1)])
            self.stages = nn.ModuleList([Stacked(2 * f[n - 2 - j], f[n - 2 - j], arch.n_conv_per_stage_decoder[j]) for j in range(n - 1)])
            # (deep supervision off: only the last head has parameters in the engine's blob)
            self.seg_layers = nn.ModuleList([nn.Identity() for _ in range(n - 2)] + [nn.Conv2d(f[0], arch.num_classes, 1)])

        def forward(self, skips):
            x = skips[-1]
            for j in range(len(self.stages)):
                x = self.transpconvs[j](x)
                x = self.stages[j](torch.cat((x, skips[-(j + 2)]), 1))
            return self.seg_layers[-1](x)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = Encoder()
            self.decoder = Decoder()

        def forward(self, x):
            return self.decoder(self.encoder(x))

    return Net().eval()


def plans_for(arch, patch=(64, 64), extra=None):
    """A ``plans.json`` dictionary as nnU-Net's ResEnc planner writes it, for `arch`."""
    n = arch.n_stages
    kw = {'n_stages': n, 'features_per_stage': list(arch.features_per_stage), 'conv_op': 'torch.nn.modules.conv.Conv2d',
          'kernel_sizes': [[3, 3]] * n, 'strides': [list(s) for s in arch.strides], 'n_blocks_per_stage': list(arch.n_blocks_per_stage),
          'n_conv_per_stage_decoder': list(arch.n_conv_per_stage_decoder), 'conv_bias': True,
          'norm_op': 'torch.nn.modules.instancenorm.InstanceNorm2d', 'norm_op_kwargs': {'eps': 1e-05, 'affine': True},
          'dropout_op': None, 'dropout_op_kwargs': None, 'nonlin': 'torch.nn.LeakyReLU', 'nonlin_kwargs': {'inplace': True}}
    kw.update(extra or {})
    return {'configurations': {'2d': {'patch_size': list(patch), 'spacing': [1.0, 1.0], 'architecture': {
        'network_class_name': 'dynamic_network_architectures.architectures.unet.ResidualEncoderUNet', 'arch_kwargs': kw,
        '_kw_requires_import': ['conv_op', 'norm_op', 'dropout_op', 'nonlin']}}}}


def write_model_folder(root, arch, seed, patch, duplicates=True):
    """A model folder as nnU-Net's ResEnc trainer leaves it (one fold): dataset.json, plans.json, fold_0/checkpoint_final.pth.  `duplicates`:
    the checkpoint also carries the alias keys of the training-time module tree (``decoder.encoder.*``, ``*.all_modules.*``) and the
    deep-supervision heads.  Returns the blob the loader must pack."""
    import json
    import torch
    from totalsegmentator2d_amd import weights
    labels = {'background': 0, **{f'organ_{i + 1}': i + 1 for i in range(arch.num_classes)}}
    with open(os.path.join(root, 'dataset.json'), 'w') as f:
        json.dump({'channel_names': {str(i): n for i, n in enumerate(['mean', 'max'][:arch.input_channels])}, 'labels': labels,
                   'file_ending': '.nrrd', 'multilabel': True, 'numTraining': 1}, f)
    plans = plans_for(arch, patch)
    plans.update({'plans_name': 'nnUNetResEncUNetMPlans', 'transpose_forward': [0, 1, 2], 'transpose_backward': [0, 1, 2]})
    plans['configurations']['2d'].update({'normalization_schemes': ['ZScoreNormalization'] * arch.input_channels,
                                          'use_mask_for_norm': [False] * arch.input_channels})
    with open(os.path.join(root, 'plans.json'), 'w') as f:
        json.dump(plans, f)
    sd = weights.synthetic_state_dict(arch, seed)
    full = {}
    for k, v in sd.items():
        t = torch.from_numpy(np.array(v))
        full[k] = t
        if duplicates and k.startswith('encoder.'):
            full['decoder.' + k] = t                                                          # the decoder holds a reference to the encoder
            if '.conv.' in k or '.norm.' in k:
                full[k.replace('.conv.', '.all_modules.0.').replace('.norm.', '.all_modules.1.')] = t
    if duplicates:
        n = arch.n_stages
        for j in range(n - 2):                                                                # deep-supervision heads (unused at inference)
            full[f'decoder.seg_layers.{j}.weight'] = torch.zeros(arch.num_classes, arch.features_per_stage[n - 2 - j], 1, 1)
            full[f'decoder.seg_layers.{j}.bias'] = torch.zeros(arch.num_classes)
    os.makedirs(os.path.join(root, 'fold_0'), exist_ok=True)
    torch.save({'network_weights': full, 'inference_allowed_mirroring_axes': (0, 1), 'trainer_name': 'nnUNetTrainer',
                'init_args': {'configuration': '2d', 'fold': 0}}, os.path.join(root, 'fold_0', 'checkpoint_final.pth'))
    return weights.pack_blob(arch, sd)
