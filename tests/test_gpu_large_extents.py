"""The forward path at the sizes where its 32-bit quantities end: bytes past 2^32 and elements past 2^31 in one activation, the un-run branch of
``split_epilogue``, a residual encoder past 2^26 pixels, and the largest single image ``reserve_checked`` accepts ("32-bit quantities of the
forward path", has the audit these cases belong to).

Every case
  * pins, through ``op_kernels()`` / ``op_ksplit()``, the op -> kernel table of the batch AND of the rows run alone (``TABLES``), as
    tests/test_gpu_full_batch_layers.py does;
  * holds selected rows of the large batch - the first, the last and the two on either side of the boundary it crosses - bit for bit against the same
    rows run alone on an engine with option ``'sbk': 0`` (the full-batch dispatch makes a row a function of its own pixels and the weights);
  * holds one or two of those rows against the torch-CPU oracle at the suite's end-to-end bounds: 1e-4 in the split and the exact mode, ``F16E_MAX`` /
    ``F16E_RMS`` of tests/test_gpu_parity.py against the 16-bit oracle in the 16-bit mode, ``assert_flips_are_tolerance_flips`` for the mask;
  * checks the whole batch on the device: finite, the packed mask is the predicate of the logits, a second run gives the same bytes.
The batch runs on an engine with the default options (what the benchmark and a caller run); inputs come from a seeded generator on the device.

Cases (the smallest shapes that cross each boundary):
  a. canonical net, 512 x 512, B = 136, split and exact mode: a level-0 activation is 136 * 2^18 * 32 * 4 = 4.56e9 bytes, byte 2^32 at row 128.
  b. 16-bit mode, (32, 64, 128), 256 x 256, B = 1032: 67.6e6 pixels, a level-0 tensor has 2.16e9 elements, element 2^31 (pixel 2^26) at row 1024
     (B = 264 at 512 x 512 crosses it too and needs 2 % more workspace).
  c. (32, 512) with one conv at level 0 and two at level 1, 16 x 16 inputs: level 1 is 8 x 8, four whole images per tile.  ``enc1.c0``
     (conv3x3s2_f16x3, S = 1) and ``enc1.c1`` (conv3x3_f16x3, S = 8 by geometry) end in ``split_epilogue`` (csrc/kernels_f16x3.h) with a.part == nullptr:
     the flat whole-batch form while B * 64 * 512 * size < 2^31, the general form beyond.  Float32 storage: B = 16376 (both flat) and 16392 (both
     general; the partials of S = 8 are floats in every mode).  16-bit mode: B = 32760 and 32776 - ``enc1.c0`` stores halves and changes form there,
     ``enc1.c1`` is general at both.  W = 16 has no packed mask (it needs W % 32 == 0): these cases check the logits only.
  d. ResidualEncoderUNet ``res_min`` of tests/resenc_util.py, split mode, 256 x 256, B = 1032: ``pix`` of res_join passes 2^26 at level 0 (elements past
     2^31), pool_proj1x1 reads its level-0 source past element 2^31.  Oracle: ``resenc_forward``.
  e. the largest single image: (32, 32), one conv per stage, K = 1, one input channel, B = 1, split mode.  The per-image limit is 2^31 - 1 bytes for the
     widest plane at four bytes per element (include/ts2d_engine.h), 16 777 215 pixels here: 4094 x 4096 is the largest accepted extent with a packed mask
     (plane 2^31 - 2^20 bytes; ragged level 0: conv3x3_first, the FLEX composed entry), 4088 x 4096 the largest on complete 8 x 32 tiles
     (conv3x3_first_split, the fixed-tile entry).  4096 x 4096, 8192 x 4096 and 32768 x 32768 - accepted before the limit existed - are refused by name
     before anything is allocated.  The oracle took 8.1 s for one such image on 8 CPU cores (15.9 GB peak).
  f. (none) the sliding-window side: every per-call offset of csrc/tiled.hip / kernels_sw.h is 64 bits wide (the table in DESIGN.md), so a call past
     2^31 half outputs crosses nothing.

Each case computes what it needs (``workspace_bytes`` + input + logits + mask + the check's transients) before it allocates and skips only when
``torch.cuda.mem_get_info()`` shows less; engines are freed before the next case.

Measured on an MI355X (256 CUs, 288 GB; ``pytest -s`` prints every figure): no case skipped, every pinned table held for the batch and for the rows
alone, every selected row bit-identical to the row alone.  Need, time of the case (engine, batch, checks, rows alone, oracle), worst error against the oracle:
  a split   17.0 GiB  3.4 - 4.7 s  6.3e-5 (row 0: 5.0e-5, row 128: 6.3e-5; bound 1e-4)        a exact   19.1 GiB  2.5 - 2.7 s  4.7e-5
  b f16     27.0 GiB  0.6 s        6.8e-3 max / 1.1e-3 rms (bounds 0.1 / 0.012)
  c split   20.7 GiB  1.2 s (B = 16376, the weights generated here) / 0.1 s (B = 16392)      2.9e-6 / 3.3e-6
  c f16     41.4 / 41.5 GiB  2.3 - 4.0 s  2.7e-3 max / 7.4e-4 rms at both B
  d resenc  27.4 GiB  0.2 s        8.9e-6
  e         5.3 GiB   6.3 - 7.8 s, nearly all of it the oracle on 16 host cores               3.0e-6 at both extents
The whole module: 29 s.
"""
import time

import numpy as np
import pytest

from tests import cases
from tests import resenc_util as R
from tests.conftest import blob_for
from tests.test_gpu_default_dispatch import _ran
from tests.test_gpu_full_batch_layers import _table
from tests.test_gpu_parity import F16E_MAX, F16E_RMS, THR, TOL, assert_flips_are_tolerance_flips
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.engine import Engine, unpack_mask

pytestmark = pytest.mark.gpu

CHUNK = 1 << 25          # logits per slab of the on-device mask check (int64 transients: 0.8 GB)


def _arch_c():
    return UNetArch(input_channels=1, num_classes=2, n_stages=2, features_per_stage=(32, 512), kernel_sizes=((3, 3),) * 2, strides=((1, 1), (2, 2)),
                    n_conv_per_stage=(1, 2), n_conv_per_stage_decoder=(1,))


# op -> (kernel, S), written down from csrc/dispatch.cpp for a chip of 256 CUs; the canonical net's are those of tests/test_gpu_full_batch_layers.py
TABLES = {
    'b': {'enc0.c0': ('conv3x3_first_split', 1), 'enc0.c1': ('conv3x3_res32', 1), 'enc1.c0': ('conv3x3s2_v2<64,k32>', 1), 'enc1.c1': ('conv3x3_h2', 1),
          'enc2.c0': ('conv3x3s2_v2<128,k32>', 1), 'enc2.c1': ('conv3x3_h2', 1), 'dec1.c0': ('conv3x3_upc_h2', 1), 'dec1.c1': ('conv3x3_h2', 1),
          'dec0.c0': ('conv3x3_up0', 1), 'dec0.c1': ('conv3x3_res32', 1), 'head': ('head', 1)},
    'c split': {'enc0.c0': ('conv3x3_first_split', 1), 'enc1.c0': ('conv3x3s2_f16x3', 1), 'enc1.c1': ('conv3x3_f16x3', 8), 'dec0.c0': ('conv3x3_upc<32>', 1),
                'head': ('head', 1)},
    'c f16': {'enc0.c0': ('conv3x3_first_split', 1), 'enc1.c0': ('conv3x3s2_f16x3', 1), 'enc1.c1': ('conv3x3_f16x3', 8), 'dec0.c0': ('conv3x3_upc_h<32>', 1),
              'head': ('head', 1)},
    'd': {'stem': ('conv3x3_first_split', 1), 'enc0.b0.c1': ('conv3x3_res32', 1), 'enc0.b0.c2': ('conv3x3_res32', 1), 'enc0.b0': ('res_join', 1),
          'enc1.b0.c1': ('conv3x3s2_v2<64>', 1), 'enc1.b0.c2': ('conv3x3_f16x3_qp', 1), 'enc1.b0.proj': ('pool_proj1x1', 1), 'enc1.b0': ('res_join', 1),
          'dec0.c0': ('conv3x3_up0', 1), 'dec0.c1': ('conv3x3_res32', 1), 'head': ('head', 1)},
    'e 4094': {'enc0.c0': ('conv3x3_first', 1), 'enc1.c0': ('conv3x3s2_f16x3_one', 1), 'dec0.c0': ('conv3x3_upc<32>', 1), 'head': ('head', 1)},
    'e 4088': {'enc0.c0': ('conv3x3_first_split', 1), 'enc1.c0': ('conv3x3s2_f16x3_one', 1), 'dec0.c0': ('conv3x3_upc<32>', 1), 'head': ('head', 1)},
}


def _need(e, x_shape, K, mask):
    """Bytes the case allocates: the workspace, the input, the logits twice (the second run), the masks twice, the slabs of the mask check."""
    B, C, H, W = x_shape
    lg = B * K * H * W * 4
    return e.workspace_bytes(B, H, W) + B * C * H * W * 4 + 2 * lg + (2 * lg // 32 if mask else 0) + (4 * 8 * min(CHUNK, lg // 4) if mask else 0)


def _mask_is_predicate(lg, mk):
    """On the device, in slabs of whole rows: bit j of a packed word is logit[.., 32 w + j] > THR."""
    import torch
    W = lg.shape[-1]
    lgf, mkf = lg.reshape(-1, W // 32, 32), mk.reshape(-1, W // 32)
    step = max(1, CHUNK // W)
    shifts = torch.arange(32, device=lg.device)
    for r0 in range(0, lgf.shape[0], step):
        packed = ((lgf[r0:r0 + step] > THR).to(torch.int64) << shifts).sum(-1)
        if not torch.equal(packed, mkf[r0:r0 + step].to(torch.int64) & 0xFFFFFFFF):
            return False
    return True


def _oracle(kind, arch, sd, x, mode):
    from oracle import torch_oracle as O
    if kind == 'resenc':
        return R.resenc_forward(arch, sd, x).numpy()
    return O.unet_forward(arch, sd, x, emulate='f16').numpy() if mode == 'f16' else O.unet_forward(arch, sd, x).numpy()


def _run_case(tag, arch, sd, blob, mode, shape, rows, oracle_rows, table, seed, kind='unet'):
    """The batch on a default engine, its whole-batch checks, then the rows alone under 'sbk': 0 and the oracle.  Returns the worst oracle error."""
    import torch
    from oracle import torch_oracle as O
    B, H, W = shape
    C, K = arch.input_channels, arch.num_classes
    mask = W % 32 == 0
    t0 = time.time()
    torch.cuda.empty_cache()
    with Engine(arch, blob) as e:
        if mode != 'split':
            e.set_precision(mode)
        need, free = _need(e, (B, C, H, W), K, mask), torch.cuda.mem_get_info()[0]
        if free < need:
            pytest.skip(f'{tag}: needs {need} bytes of device memory, {free} are free')
        gen = torch.Generator(device='cuda').manual_seed(seed)
        x = torch.randn(B, C, H, W, device='cuda', generator=gen)
        e.set_profiling(True)
        lg, mk = e.forward(x, logits=True, mask=mask)
        torch.cuda.synchronize()
        e.check()
        ran = _ran(e)
        e.set_profiling(False)
        assert ran == table, (tag, {n: (ran.get(n), table.get(n)) for n in set(ran) | set(table) if ran.get(n) != table.get(n)})
        lg2, mk2 = e.forward(x, logits=True, mask=mask)
        torch.cuda.synchronize()
        assert torch.equal(lg, lg2) and (not mask or torch.equal(mk, mk2)), f'{tag}: a second run gives other bytes'
        del lg2, mk2
        assert bool(torch.isfinite(lg).all()), tag
        if mask:
            assert _mask_is_predicate(lg, mk), f'{tag}: the packed mask is not the predicate of the logits'
        t_batch = time.time() - t0
    rows = tuple(dict.fromkeys(rows))
    got = {i: (lg[i].cpu().numpy(), mk[i].cpu().numpy() if mask else None) for i in rows}
    xr = {i: x[i:i + 1].contiguous() for i in rows}
    del lg, mk, x
    torch.cuda.empty_cache()
    with Engine(arch, blob, options={'sbk': 0}) as e1:
        if mode != 'split':
            e1.set_precision(mode)
        e1.set_profiling(True)
        for i in rows:
            li, mi = e1.forward(xr[i], logits=True, mask=mask)
            torch.cuda.synchronize()
            assert _ran(e1) == table, (tag, 'row alone', _ran(e1))
            assert np.array_equal(li[0].cpu().numpy(), got[i][0]), f'{tag}: row {i} of the batch of {B} differs from the row alone'
            assert not mask or np.array_equal(mi[0].cpu().numpy(), got[i][1]), f'{tag}: mask row {i} of the batch of {B} differs from the row alone'
    worst = 0.0
    for i in oracle_rows:
        ref = _oracle(kind, arch, sd, xr[i].cpu().numpy(), mode)
        d = got[i][0][None] - ref
        err, rms = float(np.abs(d).max()), float(np.sqrt((d.astype(np.float64) ** 2).mean()))
        print(f'[large] {tag} row {i}: max |logits - oracle| {err:.3e} rms {rms:.3e}')
        if mode == 'f16':
            assert err <= F16E_MAX and rms <= F16E_RMS, (tag, i, err, rms)
        else:
            assert err <= TOL, (tag, i, err)
        if mask:
            assert_flips_are_tolerance_flips(got[i][0][None], ref, unpack_mask(got[i][1][None].view(np.uint32), W), O.logits_to_mask(ref).numpy())
        worst = max(worst, err)
    print(f'[large] {tag}: needs {need / 2 ** 30:.1f} GiB, batch part {t_batch:.1f} s, all {time.time() - t0:.1f} s, worst oracle error {worst:.3e}')
    return worst


# ------------------------------------------------------------------------------------------------------------------ a. bytes past 2^32
@pytest.mark.parametrize('mode', ['split', 'exact'])
def test_a_canonical_net_batch_136_bytes_past_2_32(mode):
    arch = UNetArch.canonical()
    sd, blob = blob_for(arch, 1)
    assert 127 * 512 * 512 * 32 * 4 < 2 ** 32 <= 128 * 512 * 512 * 32 * 4 < 136 * 512 * 512 * 32 * 4
    _run_case(f'a {mode}', arch, sd, blob, mode, (136, 512, 512), (0, 127, 128, 135), (0, 128), _table(('twins base', mode), arch), 0)


# ------------------------------------------------------------------------------------------------------------------ b. elements past 2^31
def test_b_f16_three_stages_batch_1032_elements_past_2_31():
    arch = cases.unet(3, (32, 64, 128), 2, cin=1)
    sd, blob = blob_for(arch, 3)
    assert 1023 * 256 * 256 < 2 ** 26 <= 1024 * 256 * 256 < 1032 * 256 * 256 and 1032 * 256 * 256 * 32 > 2 ** 31
    _run_case('b f16', arch, sd, blob, 'f16', (1032, 256, 256), (0, 1023, 1024, 1031), (0, 1024), TABLES['b'], 1)


# ------------------------------------------------------------------------------------------------------------------ c. split_epilogue
# (mode, B, rows): the first and the last row, and the rows on either side of byte 2^31 of the level-1 output (row 16384 of floats, 32768 of halves)
C_RUNS = (('split', 16376, (0, 8191, 8192, 16375)), ('split', 16392, (0, 16383, 16384, 16391)),
          ('f16', 32760, (0, 16383, 16384, 32759)), ('f16', 32776, (0, 16383, 16384, 32767, 32768, 32775)))


@pytest.mark.parametrize('mode,B,rows', C_RUNS, ids=[f'{m}-{b}' for m, b, _ in C_RUNS])
def test_c_both_forms_of_split_epilogue_on_whole_image_tiles(mode, B, rows):
    arch = _arch_c()
    sd, blob = blob_for(arch, 5)
    size = 4 if mode == 'split' else 2
    flat_c0, flat_c1 = B * 64 * 512 * size < 2 ** 31, B * 64 * 512 * 4 < 2 ** 31       # (enc1.c1 splits K: float partials in every mode)
    assert (flat_c0, flat_c1) == {16376: (True, True), 16392: (False, False), 32760: (True, False), 32776: (False, False)}[B]
    # the table: conv3x3s2_f16x3 / conv3x3_f16x3 at level 1, whose 4 x 8 x 8 tile (four whole images, 256 rows) is what the branch tests for -
    # tests/test_workspace_plan_cpu.py holds the tile of these kernels to NIMG * TH * TW <= 256 and TH x TW to the image at NIMG > 1 (W4)
    _run_case(f'c {mode} B={B}', arch, sd, blob, mode, (B, 16, 16), rows, (rows[0], rows[-2]), TABLES[f'c {mode}'], 2)


# ------------------------------------------------------------------------------------------------------------------ d. residual encoder
def test_d_residual_encoder_batch_1032_pixels_past_2_26():
    from totalsegmentator2d_amd import weights
    arch = R.RES_CASES['res_min'][0]
    sd = weights.synthetic_state_dict(arch, 31)
    blob = weights.pack_blob(arch, sd)
    _run_case('d resenc', arch, sd, blob, 'split', (1032, 256, 256), (0, 1023, 1024, 1031), (0, 1024), TABLES['d'], 3, kind='resenc')


# ------------------------------------------------------------------------------------------------------------------ e. the largest single image
def _arch_e():
    return cases.unet(2, (32, 32), 1, cin=1, nconv=1)


@pytest.mark.parametrize('H,W', [(4094, 4096), (4088, 4096)])
def test_e_the_largest_accepted_single_image(H, W):
    """The oracle of one such image: 8.1 s on 8 CPU cores."""
    arch = _arch_e()
    sd, blob = blob_for(arch, 9)
    assert H * W * 32 * 4 <= 2 ** 31 - 1 < (H + 2) * W * 32 * 4 or H % 8 == 0
    _run_case(f'e {H}x{W}', arch, sd, blob, 'split', (1, H, W), (0,), (0,), TABLES[f'e {H}'], 4)


# extents the pixel cap alone (B * H * W < 2^31) accepted: each is refused by name, before any allocation
REFUSED = ((4096, 4096), (4098, 4096), (8192, 4096), (4096, 8192), (32768, 32768))


def test_e_extents_above_the_per_image_limit_are_refused_by_name_without_allocating():
    arch = _arch_e()
    _, blob = blob_for(arch, 9)
    for mode in ('split', 'exact', 'f16'):
        with Engine(arch, blob) as e:
            e.set_precision(mode)
            e.reserve(1, 64, 64)
            before = e.device_bytes()
            for H, W in REFUSED:
                assert H * W < 2 ** 31 and H * W * 32 * 4 > 2 ** 31 - 1
                with pytest.raises(RuntimeError, match=rf'image extent {H}x{W} exceeds the per-image limit.*{H * W * 128} bytes.*2147483647 bytes'):
                    e.reserve(1, H, W)
                assert e.device_bytes() == before, (mode, H, W)
            e.reserve(1, 4094, 4096)                                    # ... and the extent below is reserved
            assert e.device_bytes() > before
    # a residual encoder: 2^29 - 32 pixels per call (res_join launches 8 threads per pixel; the pixel cap alone accepted up to 2^31 - 1)
    from totalsegmentator2d_amd import weights
    arch = R.RES_CASES['res_min'][0]
    with Engine(arch, weights.pack_blob(arch, weights.synthetic_state_dict(arch, 31))) as e:
        e.reserve(1, 64, 64)
        before = e.device_bytes()
        for B, H, W in ((8192, 256, 256), (2048, 512, 512), (32767, 256, 256), (2 ** 25 - 1, 4, 4)):
            with pytest.raises(RuntimeError, match=rf'B\*H\*W = {B * H * W} exceeds the 2\^29 - 32 pixels per call of a residual-encoder engine'):
                e.reserve(B, H, W)
            assert e.device_bytes() == before, (B, H, W)
