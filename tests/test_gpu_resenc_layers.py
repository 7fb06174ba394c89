"""Whole ResidualEncoderUNet programs under per-layer oracles, on both sides of the small-batch dispatch.

tests/test_gpu_resenc.py judges the decoder and the head of a residual net end to end at 1e-4 only; here EVERY op that ran in a forward -
stem, conv1, conv2, projection, join, the decoder entries that read join outputs, the decoder blocks and the head - is compared with ONE
float64 block on the engine's OWN inputs of that op (tests/layer_check.py, the residual rules of its module docstring), rows (0, B - 1), in
the split and the exact mode (the 16-bit mode is refused for such nets).  Every case first pins the op -> (kernel, S) table it means to test
(``TABLES``, written down from an MI355X with 256 CUs), so that a change of the dispatch fails loudly instead of testing something else.
tests/test_layer_check_resenc_cpu.py shows, without a GPU, which seeded defects these bounds catch.

  a. the full-batch dispatch ("sbk" = 0: what ``predict_tiled_batch`` and the predictor run): the ten cases of tests/resenc_util.py, and
     res_aniso / res_aniso21 at B = 3 (the image stride of a (1, 2) projection with fused partial statistics, of a 128-channel (2, 1) join).
  b. the default dispatch: the same cases at their own B, and res_deep at B = 1 - split-K on a linear conv2, on a stride-2 conv1 that reads
     a join, the un-composed decoder entry that reads a join, the three reduction forms of launch_stats.
  c. the option twins on res_deep under the full-batch dispatch, one engine, one option at a time.
  d. (last) every conv kernel name a residual program can reach was seen READING A JOIN OR THE STEM and passed.
  e. res_win12: every kept tensor of row 1 of the B = 3 full-batch forward is, byte for byte, that row run alone.

What the MI355X reports for res_deep (128 x 128, B = 2) under the full dispatch is what csrc/dispatch.cpp leads one to expect, line by line:
the level-0 32 -> 32 blocks on conv3x3_res32; the stride-2 conv1 of levels 1 / 2 / 3 on conv3x3s2_v2<64> / <128> / <128>; levels 1 and 2 on
conv3x3_f16x3_qp; level 3 (16 x 16) on conv3x3_f16x3_one<64>; the 8 x 8 level on conv3x3_f16x3 / conv3x3s2_f16x3 with S = 8 (four images per
tile: choose_ksplit); dec3.c0 on the FLEX instance of conv3x3_upc<64> (16 x 16 is no multiple of 8 x 32), dec2.c0 on conv3x3_upq, dec1.c0 on
conv3x3_upc<64> (128 coarse channels < kUpqMin), dec0.c0 on conv3x3_up0.  No difference to explain.  Under the default dispatch levels 2 and 3
move to the one-image kernels with S = 2 / 4 (conv2 and the stride-2 conv1 alike), dec3 / dec2 / dec1 run un-composed (convT2x2_f16x3 + a split-K
conv with S = 8 / 4 / 2), and the three reduction forms of launch_stats are all reached on res_deep alone: HW = 256 at level 3, HW = 1024 at level
2, the generic one at the 8 x 8 level (S = 8 by geometry); the smaller cases add the generic form at 48 ... 240 pixels.  B = 1 and B = 2 give the
same table.

Measured worst per-layer values (MI355X, 256 CUs; printed by every case and, per kernel name and op kind, by the last test: ``pytest -s``).
Every op of every case stayed under SPLIT_LAYER_TOL = 8e-6 itself; ``max(SPLIT_LAYER_TOL, 2 E_op)`` exceeds it for ONE op, res_deep's
enc4.b0.proj (E_op 5.6e-6 ... 6.4e-6 on the test host, bound 1.1e-5 ... 1.3e-5; the engine: 5.6e-6 ... 6.6e-6).  Absolute on the normalised
output against the float64 block, over both dispatches and the twins (kernel, worst, case, op):
  conv3x3_up0            4.7e-6  res_deep s2v2=0 dec0.c0           conv_mfma_f32 (exact)  3.5e-6  res_win21 enc0.b0.c1
  conv3x3_res32          3.4e-6  res_aniso21 B=3 full enc0.b0.c1   conv3x3_f16x3_qp       2.8e-6  res_min full enc1.b0.c2
  conv3x3_f16x3          2.4e-6  res_deep one=0 enc3.b1.c2         conv3x3_upc<64>        2.2e-6  res_deep res=0 dec3.c0 (FLEX tile)
  conv3x3s2_f16x3_one    2.2e-6  res_deep s2v2=0 enc3.b0.c1        conv3x3_f16x3_one<64>  2.1e-6  res_deep q=0 enc3.b1.c2
  conv3x3s2_v2<128>      2.1e-6  res_deep q=0 enc3.b0.c1           conv3x3s2_v2<64>       2.0e-6  res_deep full enc1.b0.c1
  conv3x3_f16x3_one<32>  2.0e-6  res_deep res=0 enc0.b0.c1         conv3x3_upq            1.7e-6  res_deep s2v2=0 dec2.c0
  conv3x3_upc<32>        1.6e-6  res_pad default dec0.c0           conv3x3s2_f16x3        1.5e-6  res_deep one=0 enc3.b0.c1
  conv3x3_first_split    1.2e-6  / conv3x3_first 1.1e-6 (stem)     pool_proj1x1           6.4e-6 split, 6.6e-6 exact  res_deep enc4.b0.proj
  convT2x2_f16x3         4.7e-7 of the largest value (res_deep default dec3.up, reading a join); convT_mfma_f32 2.3e-7; head 3.0e-7 split, 3.5e-7 exact
  res_join               0.50 of its derived bound (res_deep enc0.b0; 0.25 where the residual is pooled or projected)
Per op kind (split / exact): stem and conv1 3.4e-6 / 3.5e-6, conv2 (not activated) 3.2e-6 / 3.1e-6, projection (not activated) 6.4e-6 / 6.6e-6,
decoder blocks 4.7e-6 / 2.9e-6; worst E_op per kind 3.0e-6 / 3.5e-6, 2.8e-6 / 3.1e-6, 6.4e-6 / 6.2e-6, 2.9e-6 / 2.8e-6.  The projection's
figure and its E_op agree to three digits on the same element: both are the fp32 rounding of an un-activated output near 40, not a kernel's
error.  The windows at B = 3 (res_win12, res_win21, res_aniso, res_aniso21) and the spanning tiles (res_span) give the values of their B = 1 / 2
neighbours to the second digit.  The whole module takes about ten seconds, float64 references included; its slowest case two."""
import json

import numpy as np
import pytest

from tests import layer_check as LC
from tests import resenc_util as R
from tests.conftest import blob_for
from tests.test_gpu_default_dispatch import _ran, _reduction
from tests.test_gpu_full_batch_layers import FLOAT_NAMES
from totalsegmentator2d_amd.engine import Engine

pytestmark = pytest.mark.gpu

MODES = ('split', 'exact')
SEEN = {}            # kernel -> [(case, op, worst, reads a join or the stem)]: filled by the cases, read by the last test
KINDS = {}           # (op kind, mode) -> [(worst, E_op or None, case, op)]
REDUCTIONS = {}      # reduction form of launch_stats -> [(case, op, S)] of split-K ops that passed under the default dispatch
MEMO = {}            # reference blocks by the bytes of their inputs (the exact mode gives the same bits under both dispatches; the twins share a prefix)

# ------------------------------------------------------------------------------------------------------------------ the pinned tables
# (case, dispatch) -> (base (case, dispatch) or None, {op: (kernel, S) that differs from the base; None: the op did not run}); split mode
TABLES = {
    ('res_min', 'full'): (None, {'stem': ('conv3x3_first_split', 1), 'enc0.b0.c1': ('conv3x3_res32', 1),
                                 'enc0.b0.c2': ('conv3x3_res32', 1), 'enc0.b0': ('res_join', 1), 'enc1.b0.c1': ('conv3x3s2_v2<64>', 1),
                                 'enc1.b0.c2': ('conv3x3_f16x3_qp', 1), 'enc1.b0.proj': ('pool_proj1x1', 1), 'enc1.b0': ('res_join', 1),
                                 'dec0.c0': ('conv3x3_up0', 1), 'dec0.c1': ('conv3x3_res32', 1), 'head': ('head', 1)}),
    ('res_pool', 'full'): (None, {'stem': ('conv3x3_first', 1), 'enc0.b0.c1': ('conv3x3_f16x3_one<32>', 1),
                                  'enc0.b0.c2': ('conv3x3_f16x3_one<32>', 1), 'enc0.b0': ('res_join', 1),
                                  'enc1.b0.c1': ('conv3x3s2_v2<64>', 1), 'enc1.b0.c2': ('conv3x3_f16x3_one<64>', 1),
                                  'enc1.b0.proj': ('pool_proj1x1', 1), 'enc1.b0': ('res_join', 1),
                                  'enc1.b1.c1': ('conv3x3_f16x3_one<64>', 1), 'enc1.b1.c2': ('conv3x3_f16x3_one<64>', 1),
                                  'enc1.b1': ('res_join', 1), 'enc2.b0.c1': ('conv3x3s2_f16x3', 1), 'enc2.b0.c2': ('conv3x3_f16x3', 1),
                                  'enc2.b0': ('res_join', 1), 'enc2.b1.c1': ('conv3x3_f16x3', 1), 'enc2.b1.c2': ('conv3x3_f16x3', 1),
                                  'enc2.b1': ('res_join', 1), 'dec1.c0': ('conv3x3_upc<64>', 1), 'dec1.c1': ('conv3x3_f16x3_one<64>', 1),
                                  'dec0.c0': ('conv3x3_upc<32>', 1), 'dec0.c1': ('conv3x3_f16x3_one<32>', 1), 'head': ('head', 1)}),
    ('res_aniso', 'full'): (None, {'stem': ('conv3x3_first_split', 1), 'enc0.b0.c1': ('conv3x3_res32', 1),
                                   'enc0.b0.c2': ('conv3x3_res32', 1), 'enc0.b0': ('res_join', 1), 'enc0.b1.c1': ('conv3x3_res32', 1),
                                   'enc0.b1.c2': ('conv3x3_res32', 1), 'enc0.b1': ('res_join', 1), 'enc1.b0.c1': ('conv_mfma_f32', 1),
                                   'enc1.b0.c2': ('conv3x3_f16x3_qp', 1), 'enc1.b0.proj': ('pool_proj1x1', 1), 'enc1.b0': ('res_join', 1),
                                   'enc2.b0.c1': ('conv3x3s2_f16x3', 1), 'enc2.b0.c2': ('conv3x3_f16x3', 1), 'enc2.b0': ('res_join', 1),
                                   'enc3.b0.c1': ('conv3x3_f16x3', 1), 'enc3.b0.c2': ('conv3x3_f16x3', 1),
                                   'enc3.b0.proj': ('pool_proj1x1', 1), 'enc3.b0': ('res_join', 1), 'dec2.up': ('convT_mfma_f32', 1),
                                   'dec2.c0': ('conv3x3_f16x3', 1), 'dec2.c1': ('conv3x3_f16x3', 1), 'dec1.c0': ('conv3x3_upc<64>', 1),
                                   'dec1.c1': ('conv3x3_f16x3_qp', 1), 'dec0.up': ('convT_mfma_f32', 1),
                                   'dec0.c0': ('conv3x3_f16x3_one<32>', 1), 'dec0.c1': ('conv3x3_res32', 1), 'head': ('head', 1)}),
    ('res_aniso21', 'full'): (None, {'stem': ('conv3x3_first_split', 1), 'enc0.b0.c1': ('conv3x3_res32', 1),
                                     'enc0.b0.c2': ('conv3x3_res32', 1), 'enc0.b0': ('res_join', 1), 'enc1.b0.c1': ('conv3x3s2_v2<64>', 1),
                                     'enc1.b0.c2': ('conv3x3_f16x3_qp', 1), 'enc1.b0.proj': ('pool_proj1x1', 1),
                                     'enc1.b0': ('res_join', 1), 'enc2.b0.c1': ('conv3x3s2_f16x3', 1), 'enc2.b0.c2': ('conv3x3_f16x3', 1),
                                     'enc2.b0.proj': ('pool_proj1x1', 1), 'enc2.b0': ('res_join', 1), 'enc3.b0.c1': ('conv_mfma_f32', 1),
                                     'enc3.b0.c2': ('conv3x3_f16x3', 2), 'enc3.b0': ('res_join', 1), 'dec2.up': ('convT_mfma_f32', 1),
                                     'dec2.c0': ('conv3x3_f16x3', 1), 'dec2.c1': ('conv3x3_f16x3', 1), 'dec1.c0': ('conv3x3_upc<64>', 1),
                                     'dec1.c1': ('conv3x3_f16x3_qp', 1), 'dec0.c0': ('conv3x3_up0', 1), 'dec0.c1': ('conv3x3_res32', 1),
                                     'head': ('head', 1)}),
    ('res_tiny', 'full'): (None, {'stem': ('conv3x3_first_split', 1), 'enc0.b0.c1': ('conv3x3_res32', 1),
                                  'enc0.b0.c2': ('conv3x3_res32', 1), 'enc0.b0': ('res_join', 1), 'enc1.b0.c1': ('conv3x3s2_f16x3', 1),
                                  'enc1.b0.c2': ('conv3x3_f16x3', 1), 'enc1.b0.proj': ('pool_proj1x1', 1), 'enc1.b0': ('res_join', 1),
                                  'enc2.b0.c1': ('conv3x3s2_f16x3', 2), 'enc2.b0.c2': ('conv3x3_f16x3', 1), 'enc2.b0': ('res_join', 1),
                                  'enc3.b0.c1': ('conv3x3s2_f16x3', 2), 'enc3.b0.c2': ('conv3x3_f16x3', 1),
                                  'enc3.b0.proj': ('pool_proj1x1', 1), 'enc3.b0': ('res_join', 1), 'dec2.up': ('convT2x2_f16x3', 1),
                                  'dec2.c0': ('conv3x3_f16x3', 2), 'dec2.c1': ('conv3x3_f16x3', 1), 'dec1.up': ('convT2x2_f16x3', 1),
                                  'dec1.c0': ('conv3x3_f16x3', 1), 'dec1.c1': ('conv3x3_f16x3', 1), 'dec0.c0': ('conv3x3_up0', 1),
                                  'dec0.c1': ('conv3x3_res32', 1), 'head': ('head', 1)}),
    ('res_pad', 'full'): (None, {'stem': ('conv3x3_first', 1), 'enc0.b0.c1': ('conv3x3_f16x3_one<32>', 1),
                                 'enc0.b0.c2': ('conv3x3_f16x3_one<32>', 1), 'enc0.b0': ('res_join', 1),
                                 'enc1.b0.c1': ('conv3x3s2_v2<64>', 1), 'enc1.b0.c2': ('conv3x3_f16x3_one<64>', 1),
                                 'enc1.b0.proj': ('pool_proj1x1', 1), 'enc1.b0': ('res_join', 1),
                                 'enc1.b1.c1': ('conv3x3_f16x3_one<64>', 1), 'enc1.b1.c2': ('conv3x3_f16x3_one<64>', 1),
                                 'enc1.b1': ('res_join', 1), 'enc2.b0.c1': ('conv3x3s2_f16x3_one', 1),
                                 'enc2.b0.c2': ('conv3x3_f16x3_one<32>', 1), 'enc2.b0.proj': ('pool_proj1x1', 1),
                                 'enc2.b0': ('res_join', 1), 'dec1.c0': ('conv3x3_upc<64>', 1), 'dec1.c1': ('conv3x3_f16x3_one<64>', 1),
                                 'dec0.c0': ('conv3x3_upc<32>', 1), 'dec0.c1': ('conv3x3_f16x3_one<32>', 1), 'head': ('head', 1)}),
    ('res_deep', 'full'): (None, {'stem': ('conv3x3_first_split', 1), 'enc0.b0.c1': ('conv3x3_res32', 1),
                                  'enc0.b0.c2': ('conv3x3_res32', 1), 'enc0.b0': ('res_join', 1), 'enc1.b0.c1': ('conv3x3s2_v2<64>', 1),
                                  'enc1.b0.c2': ('conv3x3_f16x3_qp', 1), 'enc1.b0.proj': ('pool_proj1x1', 1), 'enc1.b0': ('res_join', 1),
                                  'enc1.b1.c1': ('conv3x3_f16x3_qp', 1), 'enc1.b1.c2': ('conv3x3_f16x3_qp', 1), 'enc1.b1': ('res_join', 1),
                                  'enc2.b0.c1': ('conv3x3s2_v2<128>', 1), 'enc2.b0.c2': ('conv3x3_f16x3_qp', 1),
                                  'enc2.b0.proj': ('pool_proj1x1', 1), 'enc2.b0': ('res_join', 1), 'enc2.b1.c1': ('conv3x3_f16x3_qp', 1),
                                  'enc2.b1.c2': ('conv3x3_f16x3_qp', 1), 'enc2.b1': ('res_join', 1),
                                  'enc3.b0.c1': ('conv3x3s2_v2<128>', 1), 'enc3.b0.c2': ('conv3x3_f16x3_one<64>', 1),
                                  'enc3.b0.proj': ('pool_proj1x1', 1), 'enc3.b0': ('res_join', 1),
                                  'enc3.b1.c1': ('conv3x3_f16x3_one<64>', 1), 'enc3.b1.c2': ('conv3x3_f16x3_one<64>', 1),
                                  'enc3.b1': ('res_join', 1), 'enc4.b0.c1': ('conv3x3s2_f16x3', 8), 'enc4.b0.c2': ('conv3x3_f16x3', 8),
                                  'enc4.b0.proj': ('pool_proj1x1', 1), 'enc4.b0': ('res_join', 1), 'enc4.b1.c1': ('conv3x3_f16x3', 8),
                                  'enc4.b1.c2': ('conv3x3_f16x3', 8), 'enc4.b1': ('res_join', 1), 'dec3.c0': ('conv3x3_upc<64>', 1),
                                  'dec2.c0': ('conv3x3_upq', 1), 'dec1.c0': ('conv3x3_upc<64>', 1), 'dec0.c0': ('conv3x3_up0', 1),
                                  'head': ('head', 1)}),
    ('res_span', 'full'): (None, {'stem': ('conv3x3_first', 1), 'enc0.b0.c1': ('conv3x3_f16x3_one<32>', 1),
                                  'enc0.b0.c2': ('conv3x3_f16x3_one<32>', 1), 'enc0.b0': ('res_join', 1),
                                  'enc1.b0.c1': ('conv3x3s2_v2<64>', 1), 'enc1.b0.c2': ('conv3x3_f16x3_one<64>', 1),
                                  'enc1.b0.proj': ('pool_proj1x1', 1), 'enc1.b0': ('res_join', 1), 'enc2.b0.c1': ('conv3x3s2_f16x3', 2),
                                  'enc2.b0.c2': ('conv3x3_f16x3', 1), 'enc2.b0.proj': ('pool_proj1x1', 1), 'enc2.b0': ('res_join', 1),
                                  'dec1.c0': ('conv3x3_upc<64>', 1), 'dec1.c1': ('conv3x3_f16x3_one<64>', 1),
                                  'dec0.c0': ('conv3x3_upc<32>', 1), 'dec0.c1': ('conv3x3_f16x3_one<32>', 1), 'head': ('head', 1)}),
    ('res_win12', 'full'): (None, {'stem': ('conv3x3_first_split', 1), 'enc0.b0.c1': ('conv3x3_res32', 1),
                                   'enc0.b0.c2': ('conv3x3_res32', 1), 'enc0.b0': ('res_join', 1), 'enc1.b0.c1': ('conv_mfma_f32', 1),
                                   'enc1.b0.c2': ('conv3x3_res32', 1), 'enc1.b0': ('res_join', 1), 'enc2.b0.c1': ('conv_mfma_f32', 1),
                                   'enc2.b0.c2': ('conv3x3_f16x3_qp', 1), 'enc2.b0.proj': ('pool_proj1x1', 1), 'enc2.b0': ('res_join', 1),
                                   'enc3.b0.c1': ('conv3x3s2_f16x3', 1), 'enc3.b0.c2': ('conv3x3_f16x3', 1), 'enc3.b0': ('res_join', 1),
                                   'dec2.c0': ('conv3x3_upc<64>', 1), 'dec2.c1': ('conv3x3_f16x3_qp', 1), 'dec1.up': ('convT_mfma_f32', 1),
                                   'dec1.c0': ('conv3x3_f16x3_one<32>', 1), 'dec1.c1': ('conv3x3_res32', 1),
                                   'dec0.up': ('convT_mfma_f32', 1), 'dec0.c0': ('conv3x3_f16x3_one<32>', 1),
                                   'dec0.c1': ('conv3x3_res32', 1), 'head': ('head', 1)}),
    ('res_win21', 'full'): (None, {'stem': ('conv3x3_first_split', 1), 'enc0.b0.c1': ('conv3x3_res32', 1),
                                   'enc0.b0.c2': ('conv3x3_res32', 1), 'enc0.b0': ('res_join', 1), 'enc1.b0.c1': ('conv_mfma_f32', 1),
                                   'enc1.b0.c2': ('conv3x3_res32', 1), 'enc1.b0': ('res_join', 1), 'enc1.b1.c1': ('conv3x3_res32', 1),
                                   'enc1.b1.c2': ('conv3x3_res32', 1), 'enc1.b1': ('res_join', 1), 'enc2.b0.c1': ('conv_mfma_f32', 1),
                                   'enc2.b0.c2': ('conv3x3_f16x3_qp', 1), 'enc2.b0.proj': ('pool_proj1x1', 1), 'enc2.b0': ('res_join', 1),
                                   'enc3.b0.c1': ('conv3x3s2_f16x3', 1), 'enc3.b0.c2': ('conv3x3_f16x3', 1), 'enc3.b0': ('res_join', 1),
                                   'dec2.c0': ('conv3x3_upc<64>', 1), 'dec2.c1': ('conv3x3_f16x3_qp', 1), 'dec1.up': ('convT_mfma_f32', 1),
                                   'dec1.c0': ('conv3x3_f16x3_one<32>', 1), 'dec1.c1': ('conv3x3_res32', 1),
                                   'dec0.up': ('convT_mfma_f32', 1), 'dec0.c0': ('conv3x3_f16x3_one<32>', 1),
                                   'dec0.c1': ('conv3x3_res32', 1), 'head': ('head', 1)}),
    ('res_aniso B=3', 'full'): (('res_aniso', 'full'), {}),
    ('res_aniso21 B=3', 'full'): (('res_aniso21', 'full'), {}),
    ('res_min', 'default'): (('res_min', 'full'), {}),
    ('res_pool', 'default'): (('res_pool', 'full'), {'dec1.up': ('convT2x2_f16x3', 1), 'dec1.c0': ('conv3x3_f16x3_one<64>', 2)}),
    ('res_aniso', 'default'): (('res_aniso', 'full'), {'dec1.up': ('convT2x2_f16x3', 1), 'dec1.c0': ('conv3x3_f16x3_one<64>', 2)}),
    ('res_aniso21', 'default'): (('res_aniso21', 'full'), {'dec1.up': ('convT2x2_f16x3', 1), 'dec1.c0': ('conv3x3_f16x3_one<64>', 2)}),
    ('res_tiny', 'default'): (('res_tiny', 'full'), {}),
    ('res_pad', 'default'): (('res_pad', 'full'), {'enc2.b0.c1': ('conv3x3s2_f16x3_one', 2), 'dec1.up': ('convT2x2_f16x3', 1),
                                                   'dec1.c0': ('conv3x3_f16x3_one<64>', 2)}),
    ('res_deep', 'default'): (('res_deep', 'full'), {'enc2.b0.c1': ('conv3x3s2_f16x3_one', 2), 'enc2.b0.c2': ('conv3x3_f16x3_one<64>', 2),
                                                     'enc2.b1.c1': ('conv3x3_f16x3_one<64>', 2),
                                                     'enc2.b1.c2': ('conv3x3_f16x3_one<64>', 2), 'enc3.b0.c1': ('conv3x3s2_f16x3_one', 4),
                                                     'enc3.b0.c2': ('conv3x3_f16x3_one<64>', 4),
                                                     'enc3.b1.c1': ('conv3x3_f16x3_one<64>', 4),
                                                     'enc3.b1.c2': ('conv3x3_f16x3_one<64>', 4), 'dec3.up': ('convT2x2_f16x3', 1),
                                                     'dec3.c0': ('conv3x3_f16x3_one<64>', 8), 'dec2.up': ('convT2x2_f16x3', 1),
                                                     'dec2.c0': ('conv3x3_f16x3_one<64>', 4), 'dec1.up': ('convT2x2_f16x3', 1),
                                                     'dec1.c0': ('conv3x3_f16x3_one<64>', 2)}),
    ('res_span', 'default'): (('res_span', 'full'), {'dec1.up': ('convT2x2_f16x3', 1), 'dec1.c0': ('conv3x3_f16x3_one<64>', 2)}),
    ('res_win12', 'default'): (('res_win12', 'full'), {'dec2.up': ('convT2x2_f16x3', 1), 'dec2.c0': ('conv3x3_f16x3_one<64>', 2)}),
    ('res_win21', 'default'): (('res_win21', 'full'), {'dec2.up': ('convT2x2_f16x3', 1), 'dec2.c0': ('conv3x3_f16x3_one<64>', 2)}),
    ('res_aniso B=3', 'default'): (('res_aniso', 'default'), {}),
    ('res_aniso21 B=3', 'default'): (('res_aniso21', 'default'), {}),
    ('res_deep B=1', 'default'): (('res_deep', 'default'), {}),
    ('res_deep upc=0', 'full'): (('res_deep', 'full'), {'dec3.up': ('convT2x2_f16x3', 1), 'dec3.c0': ('conv3x3_f16x3_one<64>', 1),
                                                        'dec2.up': ('convT2x2_f16x3', 1), 'dec2.c0': ('conv3x3_f16x3_one<64>', 1),
                                                        'dec1.up': ('convT2x2_f16x3', 1), 'dec1.c0': ('conv3x3_f16x3_one<64>', 1),
                                                        'dec0.up': ('convT2x2_f16x3', 1), 'dec0.c0': ('conv3x3_f16x3_one<32>', 1)}),
    ('res_deep up0=0', 'full'): (('res_deep', 'full'), {'dec0.c0': ('conv3x3_upc<32>', 1)}),
    ('res_deep q=0', 'full'): (('res_deep', 'full'), {'enc1.b0.c2': ('conv3x3_f16x3_one<64>', 1),
                                                      'enc1.b1.c1': ('conv3x3_f16x3_one<64>', 1),
                                                      'enc1.b1.c2': ('conv3x3_f16x3_one<64>', 1),
                                                      'enc2.b0.c2': ('conv3x3_f16x3_one<64>', 1),
                                                      'enc2.b1.c1': ('conv3x3_f16x3_one<64>', 1),
                                                      'enc2.b1.c2': ('conv3x3_f16x3_one<64>', 1)}),
    ('res_deep s2v2=0', 'full'): (('res_deep', 'full'), {'enc1.b0.c1': ('conv3x3s2_f16x3_one', 1),
                                                         'enc2.b0.c1': ('conv3x3s2_f16x3_one', 1),
                                                         'enc3.b0.c1': ('conv3x3s2_f16x3_one', 1)}),
    ('res_deep res=0', 'full'): (('res_deep', 'full'), {'enc0.b0.c1': ('conv3x3_f16x3_one<32>', 1),
                                                        'enc0.b0.c2': ('conv3x3_f16x3_one<32>', 1)}),
    ('res_deep one=0', 'full'): (('res_deep', 'full'), {'enc0.b0.c1': ('conv3x3_f16x3', 1), 'enc0.b0.c2': ('conv3x3_f16x3', 1),
                                                        'enc1.b0.c1': ('conv3x3s2_f16x3', 1), 'enc1.b0.c2': ('conv3x3_f16x3', 1),
                                                        'enc1.b1.c1': ('conv3x3_f16x3', 1), 'enc1.b1.c2': ('conv3x3_f16x3', 1),
                                                        'enc2.b0.c1': ('conv3x3s2_f16x3', 1), 'enc2.b0.c2': ('conv3x3_f16x3', 1),
                                                        'enc2.b1.c1': ('conv3x3_f16x3', 1), 'enc2.b1.c2': ('conv3x3_f16x3', 1),
                                                        'enc3.b0.c1': ('conv3x3s2_f16x3', 1), 'enc3.b0.c2': ('conv3x3_f16x3', 1),
                                                        'enc3.b1.c1': ('conv3x3_f16x3', 1), 'enc3.b1.c2': ('conv3x3_f16x3', 1),
                                                        'dec3.up': ('convT2x2_f16x3', 1), 'dec3.c0': ('conv3x3_f16x3', 1),
                                                        'dec2.up': ('convT2x2_f16x3', 1), 'dec2.c0': ('conv3x3_f16x3', 1),
                                                        'dec1.up': ('convT2x2_f16x3', 1), 'dec1.c0': ('conv3x3_f16x3', 1),
                                                        'dec0.up': ('convT2x2_f16x3', 1), 'dec0.c0': ('conv3x3_f16x3', 1)}),
}


def _exact_table(arch):
    """The exact mode: one kernel per op type, nothing composed, nothing split, whatever the dispatch."""
    name = {LC.OP_CONV3X3: 'conv_mfma_f32', LC.OP_CONVT2X2: 'convT_mfma_f32', LC.OP_HEAD1X1: 'head', LC.OP_PROJ1X1: 'pool_proj1x1',
            LC.OP_JOIN: 'res_join'}
    return {o['name']: ('conv3x3_first' if o['name'] == 'stem' else name[o['op']], 1) for o in arch.program()}


def _table(key, mode='split', arch=None):
    if mode == 'exact':
        return _exact_table(arch)
    base, diff = TABLES[key]
    t = dict(_table(base)) if base else {}
    for n, v in diff.items():
        if v is None:
            t.pop(n, None)
        else:
            t[n] = tuple(v)
    return t


# ------------------------------------------------------------------------------------------------------------------ helpers
CASES = [(name, None) for name in R.RES_CASES] + [('res_aniso', 3), ('res_aniso21', 3)]
IDS = [n if B is None else f'{n}-B{B}' for n, B in CASES]


def _tag(name, B):
    return name if B is None else f'{name} B={B}'


def _setup(name, B=None):
    arch, _, _, _, seed = R.RES_CASES[name]
    sd, blob = blob_for(arch, seed)
    return arch, sd, blob, R.case_input(name, B)


def _engine(arch, blob, dispatch, **opt):
    e = Engine(arch, blob, options=dict({'sbk': 0} if dispatch == 'full' else {}, **opt))
    e.set_profiling(True)
    e.keep_activations(True)
    return e


def _kind(arch, n):
    o = LC._program(arch)[n]
    if o['op'] != LC.OP_CONV3X3:
        return {LC.OP_CONVT2X2: 'up', LC.OP_HEAD1X1: 'head', LC.OP_PROJ1X1: 'proj', LC.OP_JOIN: 'join'}[o['op']]
    return 'dec' if o['key'].startswith('decoder.') else ('c2' if o['linear'] else 'stem / c1')


def _reads_join(arch, n):
    prog = LC._program(arch)
    return any(s == 'stem' or (s in prog and prog[s]['op'] == LC.OP_JOIN) for s in LC.op_sources(arch, n))


def _check(case, dispatch, e, arch, sd, x, mode):
    """One forward in `mode`; the op -> (kernel, S) table against TABLES[(case, dispatch)]; every op that ran under the per-layer oracle."""
    e.set_precision(mode)
    lg, _ = e.forward(x, logits=True)
    ran = _ran(e)
    names = [o['name'] for o in arch.program() if o['name'] in ran]
    assert set(names) == set(ran), (case, mode, sorted(set(ran) - set(names)))
    tag = f'[resenc-layers] {case} {dispatch} {mode} B={x.shape[0]} {x.shape[2]}x{x.shape[3]}'
    print(f'{tag} table: {json.dumps(ran)}')
    err, e_ops = None, {}
    try:
        worst = LC.check_layers(e, arch, sd, mode, names, rows=tuple(dict.fromkeys((0, x.shape[0] - 1))), x=x, logits=lg, memo=MEMO, e_ops=e_ops)
    except AssertionError as ex:                         # (print the table of the case before failing: the per-op values are in the message)
        err, worst = ex, {}
    print(f'{tag}: ' + ', '.join(f'{n} {ran[n][0]} S={ran[n][1]} {worst[n]:.2e}' + (f' (E_op {e_ops[n]:.1e})' if n in e_ops else '') for n in worst))
    want = _table((case, dispatch), mode, arch)            # (KeyError: a case without a pinned table)
    assert ran == want, (case, dispatch, mode, {n: (ran.get(n), want.get(n)) for n in set(ran) | set(want) if ran.get(n) != want.get(n)})
    if err is not None:
        raise err
    assert set(worst) == set(ran)                          # every op that ran was judged, through decoder and head
    for n, w in worst.items():
        SEEN.setdefault(ran[n][0], []).append((f'{case} {dispatch} {mode}', n, w, _reads_join(arch, n)))
        KINDS.setdefault((_kind(arch, n), mode), []).append((w, e_ops.get(n), f'{case} {dispatch}', n))
    return ran, worst, lg


def _note_reductions(case, arch, ran, x):
    for n, (_, S) in ran.items():
        if S > 1:
            h, w = arch.extent(LC._program(arch)[n]['level'], x.shape[2], x.shape[3])
            REDUCTIONS.setdefault(_reduction(h * w), []).append((case, n, S))


# ------------------------------------------------------------------------------------------------------------------ a. the full-batch dispatch
@pytest.mark.parametrize('name,B', CASES, ids=IDS)
def test_full_batch_dispatch_every_op(name, B):
    arch, sd, blob, x = _setup(name, B)
    with _engine(arch, blob, 'full') as e:
        for mode in MODES:
            ran, _, _ = _check(_tag(name, B), 'full', e, arch, sd, x, mode)
            assert all(ran[o['name']][0] == {LC.OP_PROJ1X1: 'pool_proj1x1', LC.OP_JOIN: 'res_join'}[o['op']]
                       for o in arch.program() if o['op'] in (LC.OP_PROJ1X1, LC.OP_JOIN)), ran


# ------------------------------------------------------------------------------------------------------------------ b. the default dispatch
@pytest.mark.parametrize('name,B', CASES + [('res_deep', 1)], ids=IDS + ['res_deep-B1'])
def test_default_dispatch_every_op(name, B):
    arch, sd, blob, x = _setup(name, B)
    prog = LC._program(arch)
    with _engine(arch, blob, 'default') as e:
        for mode in MODES:
            ran, _, _ = _check(_tag(name, B), 'default', e, arch, sd, x, mode)
            if mode != 'split':
                continue
            _note_reductions(_tag(name, B), arch, ran, x)
            if name == 'res_deep':                       # what this dispatch adds on a residual net, by the program's fields
                split = [n for n, v in ran.items() if v[1] > 1]
                assert any(prog[n]['op'] == LC.OP_CONV3X3 and prog[n]['linear'] for n in split), ran                   # a conv2: nothing activates its output
                assert any(prog[n]['op'] == LC.OP_CONV3X3 and tuple(prog[n]['stride']) == (2, 2) and _reads_join(arch, n) for n in split), ran
                ups = [n for n in ran if prog[n]['op'] == LC.OP_CONVT2X2]
                assert ups and any(_reads_join(arch, n) for n in ups), ran                                             # the un-composed entry


# ------------------------------------------------------------------------------------------------------------------ c. option twins
TWINS = ('upc', 'up0', 'q', 's2v2', 'res', 'one')


def test_option_twins_on_res_deep_every_op():
    arch, sd, blob, x = _setup('res_deep')
    with _engine(arch, blob, 'full') as e:
        _check('res_deep', 'full', e, arch, sd, x, 'split')
        for opt in TWINS:
            e.set_option(opt, 0)
            ran, _, _ = _check(f'res_deep {opt}=0', 'full', e, arch, sd, x, 'split')
            assert ran != _table(('res_deep', 'full')), opt                       # the switch switched something
            e.set_option(opt, 1)


# ------------------------------------------------------------------------------------------------------------------ e. batch invariance per layer
@pytest.mark.parametrize('mode', MODES)
def test_every_kept_tensor_of_a_row_equals_that_row_alone(mode):
    """The determinism rule of the full-batch dispatch, per layer: so far asserted for a residual net on aggregated logits only
    (tests/test_gpu_resenc.py).  res_win12: per-axis windows, whose image stride enters every join and projection."""
    arch, sd, blob, x = _setup('res_win12')
    one = np.ascontiguousarray(x[1:2])
    with _engine(arch, blob, 'full') as e:
        e.set_precision(mode)
        lg, _ = e.forward(x, logits=True)
        names = list(_ran(e))
        batch = {n: e.debug_tensor(n)[1] for n in names if n != 'head'}
        l1, _ = e.forward(one, logits=True)
        assert list(_ran(e)) == names
        alone = {n: e.debug_tensor(n)[0] for n in names if n != 'head'}
    assert {o['name'] for o in arch.program() if o['op'] != LC.OP_CONVT2X2} <= set(names)            # (a composed-away transposed conv holds no tensor)
    diff = [n for n in batch if not np.array_equal(batch[n].view(np.uint32), alone[n].view(np.uint32))]
    assert not diff, (mode, diff)
    assert np.array_equal(lg[1].view(np.uint32), l1[0].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ d. coverage of the names
# conv kernel name of FLOAT_NAMES -> why no op of a residual program that reads a join or the stem is served by it
UNREACHED = {
    'conv3x3_first': 'serves the stem only, which reads the network input (seen there, in every case)',
    'conv3x3_first_split': 'serves the stem only, which reads the network input (seen there, in every split-mode case)',
    'conv3x3_first_stats': 'fuse0_applies() is false on a residual encoder: the first join adds the stem\'s output, so the stem is materialised',
    'conv3x3_res32f': 'the second half of the fused first block: see conv3x3_first_stats',
    'head': 'reads dec0.c{last}: a net has at least two stages, so a decoder block always lies between the last join and the head',
}


def test_every_reduction_form_was_reached_by_an_op_that_passed():
    """Runs after b.  HW = 256 (splitk_reduce_stats<32>), HW % 256 == 0 with HW > 256 (splitk_reduce_part + finalize) and the generic one."""
    if not REDUCTIONS:
        pytest.skip('the default-dispatch cases of this module did not run in this session')
    for k, v in sorted(REDUCTIONS.items()):
        print(f'[resenc-layers] reduction {k}: {v}')
    assert set(REDUCTIONS) == {'stats32', 'part', 'generic'}, sorted(REDUCTIONS)


def test_every_kernel_name_was_seen_reading_a_join():
    """Runs last.  A name is seen when an op it served read a join or the stem and passed the per-layer oracle in some case above."""
    if not SEEN:
        pytest.skip('the cases of this module did not run in this session')
    for k, v in sorted(SEEN.items()):
        w = max(v, key=lambda t: t[2])
        print(f'[resenc-layers] seen {k:24s} {len(v):3d} ops ({sum(t[3] for t in v):3d} reading a join / the stem), worst {w[2]:.2e} ({w[0]}, {w[1]})')
    for (k, mode), v in sorted(KINDS.items()):
        w = max(v, key=lambda t: t[0])
        es = [t[1] for t in v if t[1] is not None]
        print(f'[resenc-layers] kind {k:10s} {mode:5s} {len(v):4d} ops, worst {w[0]:.2e} ({w[2]}, {w[3]})' + (f', worst E_op {max(es):.2e}' if es else ''))
    known = set(FLOAT_NAMES) | {'pool_proj1x1', 'res_join'}
    assert set(SEEN) <= known, sorted(set(SEEN) - known)                               # a name this list does not know: restate it
    joined = {k for k, v in SEEN.items() if any(t[3] for t in v)}
    missing = sorted(set(FLOAT_NAMES) - joined - set(UNREACHED))
    assert not missing, missing
    assert not (set(UNREACHED) & joined), sorted(set(UNREACHED) & joined)              # reached after all: take it off the list
    assert {'pool_proj1x1', 'res_join'} <= joined
