"""The 16-bit restatement of a ResidualEncoderUNet (tests/resenc_f16_util.py) checked on the CPU, without the engine:

1. it is the same network: with every half rounding replaced by the identity and ``act16`` by ``leaky_relu`` it gives the float32 restatement
   of tests/resenc_util.py back;
2. which cases may carry the end-to-end assertion of tests/test_gpu_resenc_f16.py: two correct evaluations of the contract that differ in
   summation order only (convs accumulated in float32 by ATen, or in float64 before the half rounding) must stay within HALF of the
   end-to-end bounds ``F16E_MAX`` / ``F16E_RMS`` of tests/test_gpu_parity.py, and their joins, fed with the same inputs, within half of the 1 %
   cap on the share of join elements that differ - a case whose own rounding flips amplify beyond that cannot judge a third evaluation (the
   engine) under the full bounds.  ``E2E_CASES`` is the list that qualified; the per-layer checks of the GPU test run on every case;
3. ``UNetArch.program()`` knows no precision: the mode adds no op and renames none."""
import numpy as np
import pytest

from tests import resenc_util as R
from tests import resenc_f16_util as R16

torch = pytest.importorskip('torch')

F16E_MAX, F16E_RMS = 0.1, 0.012             # tests/test_gpu_parity.py (asserted equal below: importing that module needs no GPU)
JOIN_DIFFER_CAP = 0.01                      # tests/test_gpu_resenc_f16.py: share of a join's elements that may differ at all

# The cases whose twin stays within half of the bounds (measured here, printed by the test; the others and their figures are in its docstring)
E2E_CASES = ('res_min', 'res_pool', 'res_aniso', 'res_aniso21', 'res_tiny', 'res_pad', 'res_deep', 'res_span', 'res_win12', 'res_win21')


def _case(name):
    from totalsegmentator2d_amd import weights
    arch, B, H, W, seed = R.RES_CASES[name]
    return arch, weights.synthetic_state_dict(arch, seed), R.case_input(name)


def test_the_bounds_are_the_projects():
    from tests import test_gpu_parity as P
    assert (P.F16E_MAX, P.F16E_RMS) == (F16E_MAX, F16E_RMS)


@pytest.mark.parametrize('name', list(R.RES_CASES))
def test_without_the_roundings_it_is_the_float32_network(name, monkeypatch):
    from oracle import torch_oracle as O
    arch, sd, x = _case(name)
    monkeypatch.setattr(O, '_h', lambda t: t)
    monkeypatch.setattr(R16, 'act16', lambda y, slope: torch.nn.functional.leaky_relu(y, slope))
    got, gi = R16.resenc_forward_f16(arch, sd, x, return_intermediates=True)
    want, wi = R.resenc_forward(arch, sd, x, return_intermediates=True)
    # the same ATen calls on the same values in the same order: fp32 noise is the bound, zero is what the construction gives
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
    for n, w in wi.items():
        assert n in gi and float((gi[n] - w).abs().max()) <= 1e-6 * max(1.0, float(w.abs().max())), n


_twin = {}


def twin_figures(name):
    """(max, rms) of |logits - twin logits| and the largest share of differing elements over the case's joins (same inputs, two summation orders)."""
    if name not in _twin:
        arch, sd, x = _case(name)
        y, inter = R16.resenc_forward_f16(arch, sd, x, return_intermediates=True)
        y64 = R16.resenc_forward_f16(arch, sd, x, acc64=True)
        d = (y - y64).double()
        share = 0.0
        for s in range(arch.n_stages):
            for b in range(arch.n_blocks_per_stage[s]):
                nm = f'enc{s}.b{b}'
                tw = R16.block_forward_f16(arch, sd, s, b, x=inter[f'{nm}.x'], c2=inter[f'{nm}.c2'], proj=inter.get(f'{nm}.proj'), acc64=True, ops=('out',))
                share = max(share, float((tw['t'] != inter[f'{nm}.t']).double().mean()))
        _twin[name] = (float(d.abs().max()), float(d.pow(2).mean().sqrt()), share)
    return _twin[name]


@pytest.mark.parametrize('name', list(R.RES_CASES))
def test_which_cases_carry_the_end_to_end_bound(name):
    """Measured (float32 ATen against float64 accumulation, this file's twin): see the printed line of every case; E2E_CASES holds exactly the
    cases within half of the bounds."""
    mx, rms, share = twin_figures(name)
    ok = mx <= F16E_MAX / 2 and rms <= F16E_RMS / 2 and share <= JOIN_DIFFER_CAP / 2
    print(f'{name}: twin max {mx:.3e} (half bound {F16E_MAX / 2}) rms {rms:.3e} (half bound {F16E_RMS / 2}) join share {share:.3e} '
          f'(half cap {JOIN_DIFFER_CAP / 2}) -> {"qualifies" if ok else "does NOT qualify"}')
    assert ok == (name in E2E_CASES), (name, mx, rms, share)


def test_the_program_knows_no_precision():
    assert [o['name'] for o in R.RES_CASES['res_min'][0].program()] == ['stem', 'enc0.b0.c1', 'enc0.b0.c2', 'enc0.b0', 'enc1.b0.c1', 'enc1.b0.c2',
                                                                      'enc1.b0.proj', 'enc1.b0', 'dec0.up', 'dec0.c0', 'dec0.c1', 'head']
    for name, (arch, *_rest) in R.RES_CASES.items():
        prog = arch.program()
        assert [o['name'] for o in prog] == [o['name'] for o in arch.program()]
        assert not any('f16' in o['name'] or 'half' in o['name'] for o in prog)
        joins = [o for o in prog if o['op'] == 4]
        assert len(joins) == sum(arch.n_blocks_per_stage) and all(o['key'] is None for o in joins)


@pytest.mark.parametrize('name', ['res_min', 'res_pool', 'res_aniso'])
def test_the_per_op_reference_reproduces_the_restatement_from_its_own_views(name):
    """What tests/test_gpu_resenc_f16.py does with the engine's tensors, done with the restatement's: every op from the storage views of its
    inputs.  A join must come back exactly (its inputs are exact in the view); an op that reads a conv block's view may see single operands
    flip at half ties (view -> n -> h(n)), far inside the per-layer bounds."""
    from tests import layer_check as LC
    from tests import test_gpu_parity as P
    arch, sd, x = _case(name)
    y, inter = R16.resenc_forward_f16(arch, sd, x, return_intermediates=True)
    view = dict({k: v.numpy() for k, v in inter.items()}, input=x, head=y.numpy())
    for o in arch.program():
        n = o['name']
        want = R16.op_reference(arch, sd, n, [view[s] for s in LC.op_sources(arch, n)])
        if o['op'] == LC.OP_JOIN:
            lo, hi = (R16.op_reference(arch, sd, n, [view[s] for s in LC.op_sources(arch, n)], nudge=g) for g in (-2.0 ** -22, 2.0 ** -22))
            assert np.array_equal(want[0], view[n]) and np.array_equal(want[1], view[f'{n}.t']), n
            assert ((lo[0] == view[n]) | (hi[0] == view[n])).all(), n
            continue
        d = want - view[n]
        assert np.abs(d).max() <= P.F16_LAYER_MAX / 10 and np.sqrt((d ** 2).mean()) <= P.F16_LAYER_RMS / 10, (n, float(np.abs(d).max()))
