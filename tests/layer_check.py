"""TEST INFRASTRUCTURE (never imported by the product): ONE block of the engine against ONE block of the torch oracle, fed with the
engine's OWN inputs of that block (``Engine.debug_tensor``), so that an error of a layer cannot hide behind the InstanceNorm layers in
front of it or behind it.  The engine must have run its forward with ``keep_activations(True)``.

Split / exact mode: the reference block is evaluated in float64 (``layer_forward(dtype=torch.float64)``), so its own rounding is no
part of the bound; the engine's inputs are fp32 values and enter the reference exactly.  16-bit mode: the 16-bit oracle block in its
storage view and the bounds of tests/test_gpu_parity.py (``_f16_layer_ok``).

Residual encoders (``arch.encoder == 'residual'``, split / exact mode only): the graph comes from the ``src`` / ``skip`` / ``res`` / ``key`` /
``linear`` fields of ``arch.program()``, the float64 blocks from tests/resenc_util.py (``conv_norm``: stem, ``.c1``, ``.c2`` with slope 1;
``pool_proj``: ``.proj``).  A join is judged by a derived rule (:func:`join_reference`).  The other blocks of such a net - ``.c2`` and
``.proj`` are normalised but not activated - are judged under ``max(SPLIT_LAYER_TOL, 2 E_op)``, ``E_op`` = the error of the float32 torch
block against the float64 block on the same inputs (:func:`reference_error`): the reference sets the bound, the engine never does.  ``E_op``
stays at or below 3.5e-6 for every conv block of the cases of tests/resenc_util.py, so SPLIT_LAYER_TOL is their bound.  The second term is
the active one in ONE place: ``enc4.b0.proj`` of ``res_deep`` (a 256 -> 512 projection over 8 x 8 pixels whose un-activated outputs reach 40:
E_op 4.9e-6 on one host, 5.6e-6 ... 6.4e-6 on another - torch's summation order follows the thread count - so the bound there is up to 1.3e-5;
the engine measures 5.6e-6 ... 6.6e-6).  The plain-net paths are untouched."""
from __future__ import annotations

import numpy as np

# Bounds, each at most 4x the worst value measured on an MI355X (the numbers are in the docstring of tests/test_gpu_default_dispatch.py):
# |engine - float64 block| of a normalised, activated O(1) output in the split / exact mode (worst seen 2.0e-6 split, 3.1e-6 exact) ...
SPLIT_LAYER_TOL = 8e-6
# ... and a stand-alone transposed conv - un-normalised output, judged relative to the largest value of the reference (worst 6.9e-7; 16-bit
# mode 6.2e-4: fp16 weights and fp16 storage of the result)
SPLIT_UP_RTOL = 2e-6
F16_UP_RTOL = 2e-3
# ... and the head - un-normalised logits, judged like the transposed conv, relative to the largest value of the reference, against the head
# of the oracle on the engine's own dec0.c{last} (float64; 16-bit mode: fp16 weights and operand, fp32 sums).  Per mode, at most 4x the worst
# value measured under the full-batch dispatch (the numbers are in the docstring of tests/test_gpu_full_batch_layers.py)
HEAD_RTOL = {'split': 1e-6, 'exact': 1e-6, 'f16': 1.5e-3}          # (worst 3.0e-7 split, 2.9e-7 exact, 4.5e-4 16-bit mode)


OP_CONV3X3, OP_CONVT2X2, OP_HEAD1X1, OP_PROJ1X1, OP_JOIN = 0, 1, 2, 3, 4          # totalsegmentator2d_amd/arch.py (asserted in _program)
JOIN_UNITS = 4           # a join: |out - lrelu(c2 + r)| <= JOIN_UNITS * 2^-23 * max(1, |c2|, |r|) element-wise (:func:`join_reference`)


def _residual(arch):
    return getattr(arch, 'encoder', 'plain') == 'residual'


_programs = {}


def _program(arch):
    """{op name: op} of ``arch.program()``, made once per arch."""
    key = repr(arch)
    if key not in _programs:
        from totalsegmentator2d_amd import arch as A
        assert (A.OP_CONV3X3, A.OP_CONVT2X2, A.OP_HEAD1X1, A.OP_PROJ1X1, A.OP_JOIN) == (OP_CONV3X3, OP_CONVT2X2, OP_HEAD1X1, OP_PROJ1X1, OP_JOIN)
        _programs[key] = {o['name']: o for o in arch.program()}
    return _programs[key]


def _res_sources(arch, name):
    """:func:`op_sources` of a residual net, from the program's fields: (src,) for stem / ``.c1`` / ``.c2`` / ``.proj`` / ``.up`` / head,
    (conv2, what the join adds) for a join ``encS.bB``, (coarse, skip) for ``decL.c0`` - the skip is the last JOIN of level L."""
    prog = _program(arch)
    o = prog[name]
    if o['op'] == OP_JOIN:
        return (o['src'], o['res'])
    if o['skip'] is not None:
        up = prog[o['src']]
        assert up['op'] == OP_CONVT2X2, (name, up['name'])
        return (up['src'], o['skip'])
    return (o['src'],)


def join_reference(arch, c2, res, pool):
    """(want, bound) of a join, float64, from the values the accessor shows: ``lrelu(c2 + r)``; r = `res` itself (the projection, or the
    block's input) or - `pool` != (1, 1) - ATen's float32 average of `res` over the window.  Element-wise bound
    ``JOIN_UNITS * 2^-23 * max(1, |c2|, |r|)``: one unit for each input's accessor rounding against the kernel's fused form, one for the
    sum, one for the slope product - derived, not measured."""
    import torch
    c2 = np.asarray(c2, np.float32)
    r = np.asarray(res, np.float32)
    if tuple(pool) != (1, 1):
        r = torch.nn.functional.avg_pool2d(torch.from_numpy(np.ascontiguousarray(r)), tuple(pool), tuple(pool)).numpy()
    r = r.astype(np.float64)
    t = c2.astype(np.float64) + r
    want = np.where(t > 0, t, t * np.float64(np.float32(arch.leaky_slope)))
    return want, JOIN_UNITS * 2.0 ** -23 * np.maximum(1.0, np.maximum(np.abs(c2), np.abs(r)))


def _res_block(arch, sd, name, srcs, dtype):
    """Block `name` of a residual net from `srcs` in `dtype` (None: torch's float32), as a tensor; None for the ops whose reference has one
    form only (join, transposed conv, head)."""
    from oracle import torch_oracle as O
    from tests import resenc_util as R
    o = _program(arch)[name]
    if o['op'] == OP_PROJ1X1:
        return R.pool_proj(sd, o['key'], srcs[0], o['stride'], arch.norm_eps, dtype)
    if o['op'] != OP_CONV3X3:
        return None
    if o['key'].startswith('decoder.'):                            # the decoder is the plain net's: the oracle's own block
        return O.layer_forward(arch, sd, name, srcs[0], srcs[1] if len(srcs) > 1 else None, dtype=dtype)
    return R.conv_norm(sd, o['key'], srcs[0], tuple(o['stride']), arch.norm_eps, 1.0 if o['linear'] else arch.leaky_slope, dtype)


def reference_error(arch, sd, name, srcs, want):
    """``E_op`` of a normalised block of a residual net: max |float32 torch block - `want`| on the same inputs (None: the op has no such term)."""
    got = _res_block(arch, sd, name, srcs, None)
    return None if got is None else float(np.abs(got.numpy().astype(np.float64) - want).max())


def op_sources(arch, name):
    """Names of the tensors block `name` reads: (src,) for a plain block, (coarse, skip) for ``decL.c0``, (coarse,) for ``decL.up``;
    ``'input'`` (the network input) for ``enc0.c0``; the last block of level 0 for ``head``.  Residual nets: :func:`_res_sources`."""
    if _residual(arch):
        return _res_sources(arch, name)
    if name == 'head':
        return (f'dec0.c{arch.n_conv_per_stage_decoder[-1] - 1}',)
    if name == 'enc0.c0':
        return ('input',)
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


def reference_block(arch, sd, name, srcs, mode, from_input=False):
    """The oracle's value of block `name` from the tensors `srcs` (in :func:`op_sources` order), as float64 numpy.
    ``from_input`` (``enc0.c1`` of the split / exact mode only): `srcs` holds the NETWORK INPUT and both blocks of level 0 are evaluated in
    float64, the first one never rounded to fp32 - for an engine that recomputes the first block inside the second and materialises no
    ``enc0.c0`` (conv3x3_first_stats + conv3x3_res32f)."""
    import torch
    from oracle import torch_oracle as O
    f16 = mode == 'f16'
    if _residual(arch):
        assert not f16 and not from_input, (name, mode)                     # (the 16-bit mode is refused for such nets; no fused first block)
        o = _program(arch)[name]
        if o['op'] == OP_JOIN:
            return join_reference(arch, srcs[0], srcs[1], o['stride'])[0]
        y = _res_block(arch, sd, name, srcs, torch.float64)
        if y is not None:
            return y.numpy()
    if from_input:
        assert name == 'enc0.c1' and not f16, (name, mode)
        t = {k: O._t(v).double() for k, v in sd.items() if k.startswith('encoder.stages.0.0.convs.')}
        y = O._t(srcs[0]).to(torch.float32).double()
        with torch.no_grad():
            for i in (0, 1):
                k = f'encoder.stages.0.0.convs.{i}'
                y = O.conv_block(y, t[f'{k}.conv.weight'], t[f'{k}.conv.bias'], t[f'{k}.norm.weight'], t[f'{k}.norm.bias'], 1,
                                 arch.norm_eps, arch.leaky_slope)
        return y.numpy()
    if name == 'head':
        if f16:
            return O.layer_forward(arch, sd, 'head', srcs[0], emulate='f16').numpy().astype(np.float64)
        return O.layer_forward(arch, sd, 'head', srcs[0], dtype=torch.float64).numpy()
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


def _digest(t):
    import hashlib
    a = np.ascontiguousarray(t)
    return hashlib.blake2b(a.view(np.uint8).reshape(-1), digest_size=16).digest() + repr(a.shape).encode()


def _capacity(e, arch, n, x):
    """Floats of tensor `n` for the batch of `x` (0 without `x`: the accessor's default capacity serves)."""
    if x is None:
        return 0
    lvl = _program(arch)[n]['level'] if _residual(arch) else int(n[3:n.index('.')])
    h, w = arch.extent(lvl, x.shape[2], x.shape[3])
    return x.shape[0] * arch.features_per_stage[lvl] * h * w


def layer_error(name, got, want, mode, bound=None, e_op=None):
    """(ok, worst, text): the comparison of one block under the bound of its mode.  Residual nets: `bound` - the element-wise bound of a
    join (worst: in units of it); `e_op` - ``E_op`` of a normalised block, judged under ``max(SPLIT_LAYER_TOL, 2 E_op)``."""
    got = np.asarray(got, np.float64)
    if got.shape != want.shape or not np.isfinite(got).all():
        return False, float('inf'), f'{name}: shape {got.shape} vs {want.shape}, finite {bool(np.isfinite(got).all())}'
    d = got - want
    mx, rms = float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))
    if bound is not None:
        ratio = float((np.abs(d) / bound).max())
        return ratio <= 1.0, ratio, f'{name}: join {ratio:.3f} of its bound (max {mx:.3e})'
    if e_op is not None:
        tol = max(SPLIT_LAYER_TOL, 2 * e_op)
        return mx <= tol, mx, f'{name}: max {mx:.3e} rms {rms:.3e} (E_op {e_op:.2e}, bound {tol:.1e})'
    if name.endswith('.up') or name == 'head':
        rel = mx / max(float(np.abs(want).max()), 1e-30)
        tol = HEAD_RTOL[mode] if name == 'head' else (F16_UP_RTOL if mode == 'f16' else SPLIT_UP_RTOL)
        return rel <= tol, rel, f'{name}: max rel {rel:.3e}'
    if mode == 'f16':
        from tests.test_gpu_parity import _f16_layer_ok
        return _f16_layer_ok(name, got, want), mx, f'{name}: max {mx:.3e} rms {rms:.3e}'
    return mx <= SPLIT_LAYER_TOL, mx, f'{name}: max {mx:.3e} rms {rms:.3e}'


def _res_terms(arch, sd, name, srcs, want):
    """(bound, e_op) of :func:`layer_error` for op `name` of a residual net."""
    o = _program(arch)[name]
    if o['op'] == OP_JOIN:
        return join_reference(arch, srcs[0], srcs[1], o['stride'])[1], None
    return None, reference_error(arch, sd, name, srcs, want)


def check_layers(e, arch, sd, mode, names, rows=None, x=None, logits=None, exempt=(), memo=None, e_ops=None):
    """Every block in `names` of the engine's last forward against the oracle block on the engine's own inputs.  `rows`: batch rows to
    compare (default all).  `x`, `logits`: the input and the logits of that forward (all rows), needed for ``enc0.c0`` / ``head``; a
    first block that was not materialised is judged through ``enc0.c1`` from `x` (:func:`reference_block`, ``from_input``).  `exempt`:
    names whose value is measured and returned but not asserted.  `memo`: a dict that keeps reference blocks by the bytes of their inputs
    (forwards that differ in one kernel share every block in front of it).  Asserts the bound of `mode`; returns {name: worst value} (absolute;
    relative for ``.up`` and ``head``; a join of a residual net: in units of its bound).  `e_ops`: a dict that receives {name: E_op} of the
    normalised blocks of a residual net."""
    cache, worst, bad = {}, {}, []
    res = _residual(arch)
    fused_first = None

    def tensor(n):
        if n not in cache:
            t = x if n == 'input' else (logits if n == 'head' else e.debug_tensor(n, capacity=max(1 << 26, _capacity(e, arch, n, x))))
            assert t is not None, f'check_layers: {n} needs the x= / logits= of the forward'
            cache[n] = t if rows is None else np.ascontiguousarray(t[list(rows)])
        return cache[n]
    for name in names:
        srcs, from_input = op_sources(arch, name), False
        if name in ('enc0.c0', 'enc0.c1') and mode != 'f16':
            if fused_first is None:
                fused_first = not e.materialised('enc0.c0')
            if fused_first and name == 'enc0.c0':
                continue                                     # no tensor: judged through enc0.c1 from the network input
            if fused_first:
                srcs, from_input = ('input',), True
        ins = [tensor(s) for s in srcs]
        key = None if memo is None else (id(sd), name, mode, from_input) + tuple(_digest(t) for t in ins)
        if key is None or key not in memo:
            want = reference_block(arch, sd, name, ins, mode, from_input=from_input)
            if res:
                want = (want,) + _res_terms(arch, sd, name, ins, want)
            if key is not None:
                memo[key] = want
        want = want if key is None else memo[key]
        if res:
            want, bound, e_op = want
            if e_ops is not None and e_op is not None:
                e_ops[name] = e_op
            ok, w, text = layer_error(name, tensor(name), want, mode, bound=bound, e_op=e_op)
        else:
            ok, w, text = layer_error(name, tensor(name), want, mode)
        ok = ok or name in exempt
        worst[name] = w
        if not ok:
            bad.append(text)
    assert not bad, (mode, bad)
    return worst
