"""TEST INFRASTRUCTURE (never imported by the product): ONE block of the engine against ONE block of the torch oracle, fed with the
engine's OWN inputs of that block (``Engine.debug_tensor``), so that an error of a layer cannot hide behind the InstanceNorm layers in
front of it or behind it.  The engine must have run its forward with ``keep_activations(True)``.

Split / exact mode: the reference block is evaluated in float64 (``layer_forward(dtype=torch.float64)``), so its own rounding is no
part of the bound; the engine's inputs are fp32 values and enter the reference exactly.  16-bit mode: the 16-bit oracle block in its
storage view and the bounds of tests/test_gpu_parity.py (``_f16_layer_ok``)."""
from __future__ import annotations

import numpy as np

# Bounds, each at most 4x the worst value measured on an MI355X (the numbers are in the docstring of tests/test_gpu_default_dispatch.py):
# |engine - float64 block| of a normalised, activated O(1) output in the split / exact mode (worst seen 2.0e-6 split, 3.1e-6 exact) ...
SPLIT_LAYER_TOL = 8e-6
# ... and a stand-alone transposed conv - un-normalised output, judged relative to the largest value of the reference (worst 6.9e-7; 16-bit
# mode 6.2e-4: fp16 weights and fp16 storage of the result)
SPLIT_UP_RTOL = 2e-6
F16_UP_RTOL = 2e-3


def op_sources(arch, name):
    """Names of the tensors block `name` reads: (src,) for a plain block, (coarse, skip) for ``decL.c0``, (coarse,) for ``decL.up``."""
    kind, lvl = name[:3], int(name[3:name.index('.')])
    what = name[name.index('.') + 1:]
    n_enc, n_dec = arch.n_conv_per_stage, arch.n_conv_per_stage_decoder
    last_enc = lambda s: f'enc{s}.c{n_enc[s] - 1}'
    below = lambda l: last_enc(l + 1) if l + 1 == arch.n_stages - 1 else f'dec{l + 1}.c{n_dec[arch.n_stages - 3 - l] - 1}'
    if what == 'up':
        return (below(lvl),)
    i = int(what[1:])
    if i > 0:
        return (f'{kind}{lvl}.c{i - 1}',)
    if kind == 'enc':
        return (last_enc(lvl - 1),)
    return (below(lvl), last_enc(lvl))


def reference_block(arch, sd, name, srcs, mode):
    """The oracle's value of block `name` from the tensors `srcs` (in :func:`op_sources` order), as float64 numpy."""
    import torch
    from oracle import torch_oracle as O
    f16 = mode == 'f16'
    if name.endswith('.up'):
        lvl = int(name[3:name.index('.')])
        j = arch.n_stages - 2 - lvl
        w, b = O._t(sd[f'decoder.transpconvs.{j}.weight']), O._t(sd[f'decoder.transpconvs.{j}.bias'])
        x = O._t(srcs[0]).to(torch.float32)
        st = tuple(arch.strides[lvl + 1])
        with torch.no_grad():
            if f16:      # the 16-bit contract: operand and weights rounded to fp16, fp32 accumulation, the result stored as fp16
                return O._h(O.F.conv_transpose2d(O._h(x), O._h(w), b, stride=st)).numpy().astype(np.float64)
            return O.F.conv_transpose2d(x.double(), w.double(), b.double(), stride=st).numpy()
    skip = srcs[1] if len(srcs) > 1 else None
    if f16:
        return O.layer_forward(arch, sd, name, srcs[0], skip, emulate='f16', storage_view=True).numpy().astype(np.float64)
    return O.layer_forward(arch, sd, name, srcs[0], skip, dtype=torch.float64).numpy()


def layer_error(name, got, want, mode):
    """(ok, worst, text): the comparison of one block under the bound of its mode."""
    got = np.asarray(got, np.float64)
    d = got - want
    mx, rms = float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))
    if got.shape != want.shape or not np.isfinite(got).all():
        return False, float('inf'), f'{name}: shape {got.shape} vs {want.shape}, finite {bool(np.isfinite(got).all())}'
    if name.endswith('.up'):
        rel = mx / max(float(np.abs(want).max()), 1e-30)
        return rel <= (F16_UP_RTOL if mode == 'f16' else SPLIT_UP_RTOL), rel, f'{name}: max rel {rel:.3e}'
    if mode == 'f16':
        from tests.test_gpu_parity import _f16_layer_ok
        return _f16_layer_ok(name, got, want), mx, f'{name}: max {mx:.3e} rms {rms:.3e}'
    return mx <= SPLIT_LAYER_TOL, mx, f'{name}: max {mx:.3e} rms {rms:.3e}'


def check_layers(e, arch, sd, mode, names, rows=None):
    """Every block in `names` of the engine's last forward against the oracle block on the engine's own inputs.  `rows`: batch rows to
    compare (default all).  Asserts the bound of `mode`; returns {name: worst value} (absolute; relative for ``.up``)."""
    cache, worst, bad = {}, {}, []

    def tensor(n):
        if n not in cache:
            t = e.debug_tensor(n)
            cache[n] = t if rows is None else t[list(rows)]
        return cache[n]
    for name in names:
        want = reference_block(arch, sd, name, [tensor(s) for s in op_sources(arch, name)], mode)
        ok, w, text = layer_error(name, tensor(name), want, mode)
        worst[name] = w
        if not ok:
            bad.append(text)
    assert not bad, (mode, bad)
    return worst
