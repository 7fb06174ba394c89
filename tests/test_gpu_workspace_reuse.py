"""The workspace plan is what runs: small batches inside a workspace that was reserved for a larger one under the FULL dispatch, at pairs the
three older reuse tests (test_gpu_small_batch.py, test_gpu_default_dispatch.py) do not visit.  tests/test_workspace_plan_cpu.py proves, on the
CPU, that every such (layout, run) pair of its sweep writes no live tensor and overruns no region; here a few of them run on the card and must
give the bits of an engine that never saw the larger batch.

The construction: ``predict_tiled_batch`` on B one-tile images of the network's extent - one chunk of B rows, the workspace reserved for B under
the full dispatch (every decoder entry composed, the deep levels without split-K) - then ``forward`` at b < B under the by-size dispatch in the
same engine (split-K partials, un-composed upsampled tensors in the scratch region).  Every case first asserts, from ``op_kernels()`` /
``op_ksplit()``, that the run's decoder differs from the reserved plan's: otherwise it would test nothing.

The last two cases are the tiles of several tiny images that the CPU sweep found above the kernels' staging budget (csrc/dispatch.cpp, tile_geom):
the last images of such a tile against the oracle of the mode."""
import numpy as np
import pytest

from tests import cases
from tests.conftest import blob_for
from tests.resenc_util import RES_CASES
from tests.test_gpu_default_dispatch import EDGE, _ran
from tests.test_gpu_parity import TOL, F16E_MAX, F16E_RMS
from totalsegmentator2d_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _reserve_full(e, x):
    """x: [B, C, H, W].  One sliding-window call whose only chunk is the B images, one tile each: the workspace is reserved for B rows of
    H x W under the full dispatch.  Returns the half logits of the call and what ran."""
    B, _, H, W = x.shape
    l16, _ = e.predict_tiled_batch([np.ascontiguousarray(x[i]) for i in range(B)], (H, W), [[(0, 0)]] * B, None, None, want_logits=True)
    return [a.copy() for a in l16], _ran(e)


def _decoder(ran):
    return {n: v for n, v in ran.items() if n.startswith('dec')}


def _small_in_large(arch, blob, x, small, mode, keep=False):
    """Reserve for len(x) under the full dispatch, run every batch of `small` by size in the same engine and alone in a fresh one."""
    with Engine(arch, blob) as e:
        e.set_precision(mode)
        e.set_profiling(True)
        if keep:
            e.keep_activations(True)
        big, reserved = _reserve_full(e, x)
        for b in small:
            xb = np.ascontiguousarray(x[1:1 + b])
            got, _ = e.forward(xb, logits=True)
            ran = _ran(e)
            assert _decoder(ran) != _decoder(reserved), (b, 'the run takes the reserved plan: the case tests nothing', _decoder(ran))
            kept = _tensors(e, ran) if keep else None
            with Engine(arch, blob) as fresh:
                fresh.set_precision(mode)
                fresh.set_profiling(True)
                if keep:
                    fresh.keep_activations(True)
                want, _ = fresh.forward(xb, logits=True)
                assert _ran(fresh) == ran, b
                assert np.array_equal(got, want), (mode, b, float(np.abs(got - want).max()))
                if keep:
                    alone = _tensors(fresh, ran)
                    assert kept.keys() == alone.keys() and any(v is not None for v in kept.values())
                    for name in kept:
                        assert (kept[name] is None) == (alone[name] is None), name
                        assert kept[name] is None or np.array_equal(kept[name], alone[name]), (name, mode, b)
        again, _ = _reserve_full(e, x)
        for a, b16 in zip(again, big):                                   # and back: the reserved batch is unchanged
            assert np.array_equal(a.view(np.uint16), b16.view(np.uint16))


def _tensors(e, ran):
    """Every activation of the last forward that an op of `ran` wrote (None: not materialised - the first block recomputed inside the second)."""
    out = {}
    for name in ran:
        if name in ('head', 'input.nhwc'):
            continue
        try:
            out[name] = e.debug_tensor(name, capacity=1 << 22)
        except RuntimeError as ex:
            if 'not materialised' not in str(ex):
                raise
            out[name] = None
    return out


@pytest.mark.parametrize('mode', ['split', 'f16'])
def test_edge_net_one_and_three_slices_inside_a_full_reservation_for_five(mode):
    """96 x 160: the deep levels (24 x 40, 12 x 20) are ragged - extent-following tiles, the generic split-K reduction."""
    arch = cases.unet(EDGE['n_stages'], EDGE['feats'], EDGE['K'])
    _small_in_large(arch, blob_for(arch, 81)[1], cases.make_input(arch, 5, 96, 160, 83), (1, 3), mode)


def test_residual_encoder_one_slice_inside_a_full_reservation_for_three():
    """res_deep: split-K convs around the joins under the default dispatch, composed entries under the full one."""
    arch, _, H, W, seed = RES_CASES['res_deep']
    _small_in_large(arch, blob_for(arch, seed)[1], cases.make_input(arch, 3, H, W, seed), (1,), 'split')


def test_per_axis_stage_two_slices_inside_a_full_reservation_for_four():
    """The widths (16, 48, 80, 100) with a (2, 1) stage: the generic kernels beside split-K levels."""
    arch = cases.unet(4, (16, 48, 80, 100), 5, cin=2, nconv=2, strides=[(1, 1), (2, 2), (2, 2), (2, 1)])
    dy, dx = arch.divisors
    _small_in_large(arch, blob_for(arch, 77)[1], cases.make_input(arch, 4, 8 * dy, 32 * dx, 77), (2,), 'split')


def test_kept_activations_of_one_slice_inside_a_full_reservation_for_five():
    """keep_activations on: every tensor of the b = 1 run, bit for bit the fresh engine's."""
    arch = cases.unet(EDGE['n_stages'], EDGE['feats'], EDGE['K'])
    _small_in_large(arch, blob_for(arch, 81)[1], cases.make_input(arch, 5, 96, 160, 83), (1,), 'split', keep=True)


@pytest.mark.parametrize('mode,B,H,W', [('exact', 16, 16, 64), ('exact', 16, 64, 16), ('split', 8, 8, 256), ('f16', 8, 8, 256)])
def test_the_last_images_of_a_tile_of_several_tiny_images(mode, B, H, W):
    """The 4-stage (32, 64, 128, 128) net on extents whose bottleneck is 2 x 8, 8 x 2 or 1 x 32 pixels: 16 (8) images of it were one tile whose
    patch the kernel staged only in part, so the last images of the batch read LDS nobody wrote (tests/test_workspace_plan_cpu.py, W4).  Every
    row of the batch against the float64 oracle (the 16-bit mode: against its own oracle), and the last row equal to that slice alone, bit for bit."""
    from oracle import torch_oracle as O
    arch = cases.unet(4, (32, 64, 128, 128), 6, cin=2)
    sd, blob = blob_for(arch, 31)
    x = cases.make_input(arch, B, H, W, 31)
    with Engine(arch, blob, options={'sbk': 0}) as e:
        e.set_precision(mode)
        lg, _ = e.forward(x, logits=True)
        last, _ = e.forward(np.ascontiguousarray(x[B - 1:]), logits=True)
    if mode == 'f16':      # the mode's own oracle and the suite's end-to-end bounds of it (tests/test_gpu_parity.py: about twice the worst case of the canonical nets)
        d = lg - O.unet_forward(arch, sd, x, emulate='f16').numpy()
        worst, rms = np.abs(d).reshape(B, -1).max(axis=1), np.sqrt((d ** 2).reshape(B, -1).mean(axis=1))
        print(mode, H, W, 'max per row', worst, 'rms per row', rms)
        assert worst.max() <= F16E_MAX and rms.max() <= F16E_RMS, (worst, rms)
    else:
        ref = O.unet_forward(arch, sd, x).numpy()
        err = np.abs(lg - ref).reshape(B, -1).max(axis=1)
        print(mode, H, W, 'max per row', err)
        assert err.max() <= TOL, err
    assert np.array_equal(lg[B - 1:], last), float(np.abs(lg[B - 1:] - last).max())
