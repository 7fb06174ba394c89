"""The FULL-BATCH dispatch (option "sbk" off: what a 64-row batch and ``ts2d_engine_predict_tiled_batch`` run) under per-layer oracles.

tests/test_gpu_parity.py judges these kernels end to end at 1e-4; here EVERY op that ran in a forward is compared with ONE block of the
oracle on the engine's OWN inputs of that block (tests/layer_check.py: float64 in the split / exact mode, the 16-bit oracle block in the
16-bit mode), rows (0, B - 1), the head and - through ``enc0.c1`` from the network input - the fused first block included.  Every case first
pins, through ``op_kernels()`` / ``op_ksplit()``, the op -> kernel table it means to test (``TABLES`` below, written down from an MI355X
with 256 CUs), so that a change of the dispatch fails loudly instead of testing something else.  tests/test_layer_check_cpu.py shows,
without a GPU, which seeded defects these bounds catch.

  a. canonical net, 512 x 512, B = 3 and B = 5: level 6 (8 x 8) and 7 hold four images per 256-pixel tile and split K by geometry - B = 3
     leaves an empty image slot in the only tile, B = 5 a second tile with one image; the persistent kernels walk 2 B-tile segments.
  b. canonical widths on 640 x 384, B = 2: the FLEX instances of conv3x3_upc / conv3x3s2_v2 on extent-following tiles; "flex" = 0,
     "flex2" = 0 / 1 / 2 (2 is the default).
  c. the option twins on the canonical net at B = 2, one engine, one option at a time.
  d. small nets that reach the names the canonical net never reports (32-column instances, the exact kernels on a (2, 1) stage, widths
     that are no multiples of 32), transposed-conv bias x 40 on the composed-block net.
  e. 16-bit mode, B = 64: rows 0, 37, 63 bit-identical to those rows alone.
  f. (last) every name ``kernel_name()`` of csrc/dispatch.cpp can return was seen above, per storage.  The name ``head`` covers TWO kernels:
     ``head_mfma32`` (K <= 32 at width 32: nearly every case here) and ``head_1x1`` (csrc/kernels.h: the exact mode, the ``one`` = 0 twin - and
     every model with more than 32 heads or a level-0 width of 64), so "seen" says little about the second one.  It is judged, pinned by the
     construction of its cases, in tests/test_gpu_many_heads.py (K up to 256, C = 32 and 64).

Measured worst per-layer values (MI355X, 256 CUs; printed by every case and, per kernel name, by the last test: read them with ``pytest -s``).
Every op of every case stayed under the FIXED bounds of tests/layer_check.py (8e-6 block, 2e-6 / 2e-3 transposed conv, ``_f16_layer_ok``):
no kernel needed a bound of its own.  Split / exact mode, absolute on the normalised output against the float64 block (kernel, worst, case, op):
  conv3x3_up0            4.4e-6  twins fuse0=0 dec0.c0        conv3x3_res32          4.0e-6  twins fuse0=0 first_split=0 enc0.c1
  conv_mfma_f32 (exact)  3.9e-6  canonical B=3 dec0.c1        conv3x3_res32f + conv3x3_first_stats  3.8e-6  canonical B=3 enc0.c1 (from the input)
  conv3x3_f16x3_one<64>  3.1e-6  twins upc=0 dec5.c1          conv3x3_upq            2.5e-6  twins res=0 dec4.c0
  conv3x3_f16x3 (S = 8)  2.5e-6  twins one=0 dec4.c0          conv3x3s2_v2<128>      2.4e-6  canonical B=5 enc3.c0
  conv3x3s2_f16x3_one    2.4e-6  640x384 flex2=0 enc3.c0      conv3x3s2_v2<64>       2.3e-6  twins res=0 enc1.c0
  conv3x3_f16x3_one<32>  2.3e-6  twins res=0 enc0.c1          conv3x3_upc<64>        2.3e-6  640x384 dec4.c0 (FLEX tile)
  conv3x3_f16x3_qp       2.2e-6  canonical B=3 dec4.c1        conv3x3s2_f16x3        1.9e-6  twins one=0 enc5.c0
  conv3x3_upc<32>        1.6e-6  twins up0=0 dec0.c0          conv3x3_first (exact)  1.6e-6  640x384 enc0.c0
  conv3x3_first          1.4e-6  / conv3x3_first_split 1.2e-6 (twins, enc0.c0)       conv_mfma_f32 (split, (2, 1) stage) 1.6e-6  widths enc3.c0
  convT2x2_f16x3         6.9e-7 of the largest value (twins upc=0 dec4.up); convT_mfma_f32 2.9e-7 (640x384 dec6.up)
  head                   3.0e-7 split, 2.9e-7 exact of the largest logit -> HEAD_RTOL 1e-6
The level-0 blocks (288- and 576-term sums over 512 x 512 pixels) are the worst at 3.8e-6 ... 4.4e-6, twice the 2.0e-6 measured on the split-K
kernels; the torch-fp32 block against the same float64 block reaches 3.2e-6 on a 288-term block on the CPU (tests/test_layer_check_cpu.py), so
that is the summation length, not a kernel.  B = 3 and B = 5 (rows 0 and B - 1, the empty image slot and the one-image tile) give the same values
as B = 2 to the second digit.
16-bit mode, max / bound 1e-2 (single fp16 flips of stored values; the rms bounds 1e-4 / 7e-4 held everywhere):
  conv3x3_h32<32> / conv3x3_res32 / conv3x3_upc_h2 5.5e-3, conv3x3_up0 5.3e-3, conv3x3_h2 5.2e-3, conv3x3_upc_h<32> 5.2e-3, conv3x3_upc_h<64> 5.1e-3,
  conv3x3s2_f16x3_one 4.9e-3, conv3x3_h32<64> 4.8e-3, conv3x3s2_v2<128> 4.5e-3, conv3x3s2_v2<128,k32> 4.1e-3, conv3x3_f16x3 3.4e-3,
  conv3x3s2_v2<64> / <64,k32> / conv3x3s2_f16x3 / conv3x3_first_split 3.2e-3, conv_mfma_f32 2.8e-3, conv3x3_first 9.5e-7 (fp32 weights and input);
  convT_mfma_f32 5.6e-4, convT2x2_f16x3 5.1e-4 of the largest value; head 4.5e-4 of the largest logit -> HEAD_RTOL 1.5e-3.
  Exempt (measured, not asserted): the blocks of levels with fewer than 64 pixels per image - level 7 at 512 x 512 (4 x 4), levels 6 and 7 on
  640 x 384 (10 x 6, 5 x 3).
Not done here: the 7-stage net on 448 x 576 (tests/test_gpu_parity.py has it end to end).  The whole module takes 3.5 minutes, of which
the float64 references of the option twins take 1.8."""
import numpy as np
import pytest

from tests import cases
from tests import layer_check as LC
from tests.conftest import blob_for
from tests.test_gpu_default_dispatch import _ran, EDGE
from totalsegmentator2d_amd import weights
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.engine import Engine

pytestmark = pytest.mark.gpu

MODES = ('split', 'exact', 'f16')
SEEN = {}            # (kernel, storage) -> [(case, op, worst)]: filled by the cases, read by test_every_kernel_name_was_seen (runs last)
MEMO = {}            # reference blocks by the bytes of their inputs: the twins of a case share every block in front of the op they change

# ------------------------------------------------------------------------------------------------------------------ the pinned tables
# (case, mode) -> (base (case, mode) or None, {op: (kernel, S) that differs from the base; None: the op did not run}); split and 16-bit mode
TABLES = {('canonical B=3', 'split'): (None,
                              {'enc0.c0': ('conv3x3_first_stats', 1),
                               'enc0.c1': ('conv3x3_res32f', 1),
                               'enc1.c0': ('conv3x3s2_v2<64>', 1),
                               'enc1.c1': ('conv3x3_f16x3_qp', 1),
                               'enc2.c0': ('conv3x3s2_v2<128>', 1),
                               'enc2.c1': ('conv3x3_f16x3_qp', 1),
                               'enc3.c0': ('conv3x3s2_v2<128>', 1),
                               'enc3.c1': ('conv3x3_f16x3_qp', 1),
                               'enc4.c0': ('conv3x3s2_v2<128>', 1),
                               'enc4.c1': ('conv3x3_f16x3_qp', 1),
                               'enc5.c0': ('conv3x3s2_v2<128>', 1),
                               'enc5.c1': ('conv3x3_f16x3_one<64>', 1),
                               'enc6.c0': ('conv3x3s2_f16x3', 8),
                               'enc6.c1': ('conv3x3_f16x3', 8),
                               'enc7.c0': ('conv3x3s2_f16x3', 8),
                               'enc7.c1': ('conv3x3_f16x3', 8),
                               'dec6.up': ('convT2x2_f16x3', 1),
                               'dec6.c0': ('conv3x3_f16x3', 8),
                               'dec6.c1': ('conv3x3_f16x3', 8),
                               'dec5.c0': ('conv3x3_upc<64>', 1),
                               'dec5.c1': ('conv3x3_f16x3_one<64>', 1),
                               'dec4.c0': ('conv3x3_upq', 1),
                               'dec4.c1': ('conv3x3_f16x3_qp', 1),
                               'dec3.c0': ('conv3x3_upq', 1),
                               'dec3.c1': ('conv3x3_f16x3_qp', 1),
                               'dec2.c0': ('conv3x3_upq', 1),
                               'dec2.c1': ('conv3x3_f16x3_qp', 1),
                               'dec1.c0': ('conv3x3_upc<64>', 1),
                               'dec1.c1': ('conv3x3_f16x3_qp', 1),
                               'dec0.c0': ('conv3x3_up0', 1),
                               'dec0.c1': ('conv3x3_res32', 1),
                               'head': ('head', 1)}),
 ('canonical B=3', 'f16'): (None,
                            {'enc0.c0': ('conv3x3_first_split', 1),
                             'enc0.c1': ('conv3x3_res32', 1),
                             'enc1.c0': ('conv3x3s2_v2<64,k32>', 1),
                             'enc1.c1': ('conv3x3_h2', 1),
                             'enc2.c0': ('conv3x3s2_v2<128,k32>', 1),
                             'enc2.c1': ('conv3x3_h2', 1),
                             'enc3.c0': ('conv3x3s2_v2<128,k32>', 1),
                             'enc3.c1': ('conv3x3_h2', 1),
                             'enc4.c0': ('conv3x3s2_v2<128,k32>', 1),
                             'enc4.c1': ('conv3x3_h2', 1),
                             'enc5.c0': ('conv3x3s2_v2<128,k32>', 1),
                             'enc5.c1': ('conv3x3_h32<64>', 1),
                             'enc6.c0': ('conv3x3s2_f16x3', 8),
                             'enc6.c1': ('conv3x3_f16x3', 8),
                             'enc7.c0': ('conv3x3s2_f16x3', 8),
                             'enc7.c1': ('conv3x3_f16x3', 8),
                             'dec6.up': ('convT2x2_f16x3', 1),
                             'dec6.c0': ('conv3x3_f16x3', 8),
                             'dec6.c1': ('conv3x3_f16x3', 8),
                             'dec5.c0': ('conv3x3_upc_h<64>', 1),
                             'dec5.c1': ('conv3x3_h32<64>', 1),
                             'dec4.c0': ('conv3x3_upc_h2', 1),
                             'dec4.c1': ('conv3x3_h2', 1),
                             'dec3.c0': ('conv3x3_upc_h2', 1),
                             'dec3.c1': ('conv3x3_h2', 1),
                             'dec2.c0': ('conv3x3_upc_h2', 1),
                             'dec2.c1': ('conv3x3_h2', 1),
                             'dec1.c0': ('conv3x3_upc_h2', 1),
                             'dec1.c1': ('conv3x3_h2', 1),
                             'dec0.c0': ('conv3x3_up0', 1),
                             'dec0.c1': ('conv3x3_res32', 1),
                             'head': ('head', 1)}),
 ('canonical B=5', 'split'): (('canonical B=3', 'split'), {}),
 ('canonical B=5', 'f16'): (('canonical B=3', 'f16'), {}),
 ('640x384', 'split'): (None,
                        {'enc0.c0': ('conv3x3_first_stats', 1),
                         'enc0.c1': ('conv3x3_res32f', 1),
                         'enc1.c0': ('conv3x3s2_v2<64>', 1),
                         'enc1.c1': ('conv3x3_f16x3_qp', 1),
                         'enc2.c0': ('conv3x3s2_v2<128>', 1),
                         'enc2.c1': ('conv3x3_f16x3_qp', 1),
                         'enc3.c0': ('conv3x3s2_v2<128>', 1),
                         'enc3.c1': ('conv3x3_f16x3_one<64>', 1),
                         'enc4.c0': ('conv3x3s2_v2<128>', 1),
                         'enc4.c1': ('conv3x3_f16x3_one<64>', 1),
                         'enc5.c0': ('conv3x3s2_v2<128>', 1),
                         'enc5.c1': ('conv3x3_f16x3_one<64>', 1),
                         'enc6.c0': ('conv3x3s2_f16x3', 8),
                         'enc6.c1': ('conv3x3_f16x3', 8),
                         'enc7.c0': ('conv3x3s2_f16x3', 8),
                         'enc7.c1': ('conv3x3_f16x3', 8),
                         'dec6.up': ('convT2x2_f16x3', 1),
                         'dec6.c0': ('conv3x3_f16x3', 8),
                         'dec6.c1': ('conv3x3_f16x3', 8),
                         'dec5.c0': ('conv3x3_upc<64>', 1),
                         'dec5.c1': ('conv3x3_f16x3_one<64>', 1),
                         'dec4.c0': ('conv3x3_upc<64>', 1),
                         'dec4.c1': ('conv3x3_f16x3_one<64>', 1),
                         'dec3.c0': ('conv3x3_upc<64>', 1),
                         'dec3.c1': ('conv3x3_f16x3_one<64>', 1),
                         'dec2.c0': ('conv3x3_upq', 1),
                         'dec2.c1': ('conv3x3_f16x3_qp', 1),
                         'dec1.c0': ('conv3x3_upc<64>', 1),
                         'dec1.c1': ('conv3x3_f16x3_qp', 1),
                         'dec0.c0': ('conv3x3_up0', 1),
                         'dec0.c1': ('conv3x3_res32', 1),
                         'head': ('head', 1)}),
 ('640x384', 'f16'): (None,
                      {'enc0.c0': ('conv3x3_first_split', 1),
                       'enc0.c1': ('conv3x3_res32', 1),
                       'enc1.c0': ('conv3x3s2_v2<64,k32>', 1),
                       'enc1.c1': ('conv3x3_h2', 1),
                       'enc2.c0': ('conv3x3s2_v2<128,k32>', 1),
                       'enc2.c1': ('conv3x3_h2', 1),
                       'enc3.c0': ('conv3x3s2_v2<128,k32>', 1),
                       'enc3.c1': ('conv3x3_h32<64>', 1),
                       'enc4.c0': ('conv3x3s2_v2<128,k32>', 1),
                       'enc4.c1': ('conv3x3_h32<64>', 1),
                       'enc5.c0': ('conv3x3s2_v2<128,k32>', 1),
                       'enc5.c1': ('conv3x3_h32<64>', 1),
                       'enc6.c0': ('conv3x3s2_f16x3', 8),
                       'enc6.c1': ('conv3x3_f16x3', 8),
                       'enc7.c0': ('conv3x3s2_f16x3', 8),
                       'enc7.c1': ('conv3x3_f16x3', 8),
                       'dec6.up': ('convT2x2_f16x3', 1),
                       'dec6.c0': ('conv3x3_f16x3', 8),
                       'dec6.c1': ('conv3x3_f16x3', 8),
                       'dec5.c0': ('conv3x3_upc_h<64>', 1),
                       'dec5.c1': ('conv3x3_h32<64>', 1),
                       'dec4.c0': ('conv3x3_upc_h<64>', 1),
                       'dec4.c1': ('conv3x3_h32<64>', 1),
                       'dec3.c0': ('conv3x3_upc_h<64>', 1),
                       'dec3.c1': ('conv3x3_h32<64>', 1),
                       'dec2.c0': ('conv3x3_upc_h2', 1),
                       'dec2.c1': ('conv3x3_h2', 1),
                       'dec1.c0': ('conv3x3_upc_h2', 1),
                       'dec1.c1': ('conv3x3_h2', 1),
                       'dec0.c0': ('conv3x3_up0', 1),
                       'dec0.c1': ('conv3x3_res32', 1),
                       'head': ('head', 1)}),
 ('640x384 flex=0', 'split'): (('640x384', 'split'),
                               {'dec5.up': ('convT2x2_f16x3', 1),
                                'dec5.c0': ('conv3x3_f16x3_one<64>', 1),
                                'dec4.up': ('convT2x2_f16x3', 1),
                                'dec4.c0': ('conv3x3_f16x3_one<64>', 1),
                                'dec3.up': ('convT2x2_f16x3', 1),
                                'dec3.c0': ('conv3x3_f16x3_one<64>', 1)}),
 ('640x384 flex=0', 'f16'): (('640x384', 'f16'),
                             {'dec5.up': ('convT2x2_f16x3', 1),
                              'dec5.c0': ('conv3x3_h32<64>', 1),
                              'dec4.up': ('convT2x2_f16x3', 1),
                              'dec4.c0': ('conv3x3_h32<64>', 1),
                              'dec3.up': ('convT2x2_f16x3', 1),
                              'dec3.c0': ('conv3x3_h32<64>', 1)}),
 ('640x384 flex2=0', 'split'): (('640x384', 'split'),
                                {'enc3.c0': ('conv3x3s2_f16x3_one', 1),
                                 'enc4.c0': ('conv3x3s2_f16x3_one', 1),
                                 'enc5.c0': ('conv3x3s2_f16x3_one', 1)}),
 ('640x384 flex2=0', 'f16'): (('640x384', 'f16'),
                              {'enc3.c0': ('conv3x3s2_f16x3_one', 1), 'enc4.c0': ('conv3x3s2_f16x3_one', 1), 'enc5.c0': ('conv3x3s2_f16x3_one', 1)}),
 ('640x384 flex2=1', 'split'): (('640x384', 'split'),
                                {'enc3.c0': ('conv3x3s2_f16x3_one', 1),
                                 'enc4.c0': ('conv3x3s2_f16x3_one', 1),
                                 'enc5.c0': ('conv3x3s2_f16x3_one', 1)}),
 ('twins base', 'split'): (('canonical B=3', 'split'), {}),
 ('twins base', 'f16'): (('canonical B=3', 'f16'), {}),
 ('twins fuse0=0', 'split'): (('twins base', 'split'), {'enc0.c0': ('conv3x3_first_split', 1), 'enc0.c1': ('conv3x3_res32', 1)}),
 ('twins fuse0=0 first_split=0', 'split'): (('twins base', 'split'), {'enc0.c0': ('conv3x3_first', 1), 'enc0.c1': ('conv3x3_res32', 1)}),
 ('twins fuse0=0 first_split=0', 'f16'): (('twins base', 'f16'), {'enc0.c0': ('conv3x3_first', 1)}),
 ('twins up0=0', 'split'): (('twins base', 'split'), {'dec0.c0': ('conv3x3_upc<32>', 1)}),
 ('twins up0=0', 'f16'): (('twins base', 'f16'), {'dec0.c0': ('conv3x3_upc_h<32>', 1)}),
 ('twins upc=0', 'split'): (('twins base', 'split'),
                            {'dec5.up': ('convT2x2_f16x3', 1),
                             'dec5.c0': ('conv3x3_f16x3_one<64>', 1),
                             'dec4.up': ('convT2x2_f16x3', 1),
                             'dec4.c0': ('conv3x3_f16x3_one<64>', 1),
                             'dec3.up': ('convT2x2_f16x3', 1),
                             'dec3.c0': ('conv3x3_f16x3_one<64>', 1),
                             'dec2.up': ('convT2x2_f16x3', 1),
                             'dec2.c0': ('conv3x3_f16x3_one<64>', 1),
                             'dec1.up': ('convT2x2_f16x3', 1),
                             'dec1.c0': ('conv3x3_f16x3_one<64>', 1),
                             'dec0.up': ('convT2x2_f16x3', 1),
                             'dec0.c0': ('conv3x3_f16x3_one<32>', 1)}),
 ('twins upc=0', 'f16'): (('twins base', 'f16'),
                          {'dec5.up': ('convT2x2_f16x3', 1),
                           'dec5.c0': ('conv3x3_h32<64>', 1),
                           'dec4.up': ('convT2x2_f16x3', 1),
                           'dec4.c0': ('conv3x3_h32<64>', 1),
                           'dec3.up': ('convT2x2_f16x3', 1),
                           'dec3.c0': ('conv3x3_h32<64>', 1),
                           'dec2.up': ('convT2x2_f16x3', 1),
                           'dec2.c0': ('conv3x3_h32<64>', 1),
                           'dec1.up': ('convT2x2_f16x3', 1),
                           'dec1.c0': ('conv3x3_h32<64>', 1),
                           'dec0.up': ('convT2x2_f16x3', 1),
                           'dec0.c0': ('conv3x3_h32<32>', 1)}),
 ('twins q=0', 'split'): (('twins base', 'split'),
                          {'enc1.c1': ('conv3x3_f16x3_one<64>', 1),
                           'enc2.c1': ('conv3x3_f16x3_one<64>', 1),
                           'enc3.c1': ('conv3x3_f16x3_one<64>', 1),
                           'enc4.c1': ('conv3x3_f16x3_one<64>', 1),
                           'dec4.c1': ('conv3x3_f16x3_one<64>', 1),
                           'dec3.c1': ('conv3x3_f16x3_one<64>', 1),
                           'dec2.c1': ('conv3x3_f16x3_one<64>', 1),
                           'dec1.c1': ('conv3x3_f16x3_one<64>', 1)}),
 ('twins s2v2=0', 'split'): (('twins base', 'split'),
                             {'enc1.c0': ('conv3x3s2_f16x3_one', 1),
                              'enc2.c0': ('conv3x3s2_f16x3_one', 1),
                              'enc3.c0': ('conv3x3s2_f16x3_one', 1),
                              'enc4.c0': ('conv3x3s2_f16x3_one', 1),
                              'enc5.c0': ('conv3x3s2_f16x3_one', 1)}),
 ('twins s2v2=0', 'f16'): (('twins base', 'f16'),
                           {'enc1.c0': ('conv3x3s2_f16x3_one', 1),
                            'enc2.c0': ('conv3x3s2_f16x3_one', 1),
                            'enc3.c0': ('conv3x3s2_f16x3_one', 1),
                            'enc4.c0': ('conv3x3s2_f16x3_one', 1),
                            'enc5.c0': ('conv3x3s2_f16x3_one', 1)}),
 ('twins res=0', 'split'): (('twins base', 'split'),
                            {'enc0.c0': ('conv3x3_first_split', 1),
                             'enc0.c1': ('conv3x3_f16x3_one<32>', 1),
                             'dec0.c1': ('conv3x3_f16x3_one<32>', 1)}),
 ('twins res=0', 'f16'): (('twins base', 'f16'), {'enc0.c1': ('conv3x3_h32<32>', 1), 'dec0.c1': ('conv3x3_h32<32>', 1)}),
 ('twins one=0', 'split'): (('twins base', 'split'),
                            {'enc0.c0': ('conv3x3_first_split', 1),
                             'enc0.c1': ('conv3x3_f16x3', 1),
                             'enc1.c0': ('conv3x3s2_f16x3', 1),
                             'enc1.c1': ('conv3x3_f16x3', 1),
                             'enc2.c0': ('conv3x3s2_f16x3', 1),
                             'enc2.c1': ('conv3x3_f16x3', 1),
                             'enc3.c0': ('conv3x3s2_f16x3', 1),
                             'enc3.c1': ('conv3x3_f16x3', 1),
                             'enc4.c0': ('conv3x3s2_f16x3', 1),
                             'enc4.c1': ('conv3x3_f16x3', 1),
                             'enc5.c0': ('conv3x3s2_f16x3', 1),
                             'enc5.c1': ('conv3x3_f16x3', 1),
                             'dec5.up': ('convT2x2_f16x3', 1),
                             'dec5.c0': ('conv3x3_f16x3', 1),
                             'dec5.c1': ('conv3x3_f16x3', 1),
                             'dec4.up': ('convT2x2_f16x3', 1),
                             'dec4.c0': ('conv3x3_f16x3', 1),
                             'dec4.c1': ('conv3x3_f16x3', 1),
                             'dec3.up': ('convT2x2_f16x3', 1),
                             'dec3.c0': ('conv3x3_f16x3', 1),
                             'dec3.c1': ('conv3x3_f16x3', 1),
                             'dec2.up': ('convT2x2_f16x3', 1),
                             'dec2.c0': ('conv3x3_f16x3', 1),
                             'dec2.c1': ('conv3x3_f16x3', 1),
                             'dec1.up': ('convT2x2_f16x3', 1),
                             'dec1.c0': ('conv3x3_f16x3', 1),
                             'dec1.c1': ('conv3x3_f16x3', 1),
                             'dec0.up': ('convT2x2_f16x3', 1),
                             'dec0.c0': ('conv3x3_f16x3', 1),
                             'dec0.c1': ('conv3x3_f16x3', 1)}),
 ('twins one=0', 'f16'): (('twins base', 'f16'),
                          {'enc0.c1': ('conv3x3_h32<32>', 1),
                           'enc1.c0': ('conv3x3s2_f16x3', 1),
                           'enc2.c0': ('conv3x3s2_f16x3', 1),
                           'enc3.c0': ('conv3x3s2_f16x3', 1),
                           'enc4.c0': ('conv3x3s2_f16x3', 1),
                           'enc5.c0': ('conv3x3s2_f16x3', 1),
                           'dec5.up': ('convT2x2_f16x3', 1),
                           'dec5.c0': ('conv3x3_h32<64>', 1),
                           'dec4.up': ('convT2x2_f16x3', 1),
                           'dec4.c0': ('conv3x3_h32<64>', 1),
                           'dec3.up': ('convT2x2_f16x3', 1),
                           'dec3.c0': ('conv3x3_h32<64>', 1),
                           'dec2.up': ('convT2x2_f16x3', 1),
                           'dec2.c0': ('conv3x3_h32<64>', 1),
                           'dec1.up': ('convT2x2_f16x3', 1),
                           'dec1.c0': ('conv3x3_h32<64>', 1),
                           'dec0.up': ('convT2x2_f16x3', 1),
                           'dec0.c0': ('conv3x3_h32<32>', 1),
                           'dec0.c1': ('conv3x3_h32<32>', 1)}),
 ('twins uh2=0', 'f16'): (('twins base', 'f16'),
                          {'dec4.c0': ('conv3x3_upc_h<64>', 1),
                           'dec3.c0': ('conv3x3_upc_h<64>', 1),
                           'dec2.c0': ('conv3x3_upc_h<64>', 1),
                           'dec1.c0': ('conv3x3_upc_h<64>', 1)}),
 ('twins h2=0', 'f16'): (('twins base', 'f16'),
                         {'enc1.c1': ('conv3x3_h32<64>', 1),
                          'enc2.c1': ('conv3x3_h32<64>', 1),
                          'enc3.c1': ('conv3x3_h32<64>', 1),
                          'enc4.c1': ('conv3x3_h32<64>', 1),
                          'dec4.c1': ('conv3x3_h32<64>', 1),
                          'dec3.c1': ('conv3x3_h32<64>', 1),
                          'dec2.c1': ('conv3x3_h32<64>', 1),
                          'dec1.c1': ('conv3x3_h32<64>', 1)}),
 ('twins s2k32=0', 'f16'): (('twins base', 'f16'),
                            {'enc1.c0': ('conv3x3s2_v2<64>', 1),
                             'enc2.c0': ('conv3x3s2_v2<128>', 1),
                             'enc3.c0': ('conv3x3s2_v2<128>', 1),
                             'enc4.c0': ('conv3x3s2_v2<128>', 1),
                             'enc5.c0': ('conv3x3s2_v2<128>', 1)}),
 ('composed', 'split'): (None,
                         {'enc0.c0': ('conv3x3_first_stats', 1),
                          'enc0.c1': ('conv3x3_res32f', 1),
                          'enc1.c0': ('conv3x3s2_v2<64>', 1),
                          'enc1.c1': ('conv3x3_f16x3_qp', 1),
                          'enc2.c0': ('conv3x3s2_v2<128>', 1),
                          'enc2.c1': ('conv3x3_f16x3_qp', 1),
                          'enc3.c0': ('conv3x3s2_f16x3', 1),
                          'enc3.c1': ('conv3x3_f16x3', 1),
                          'dec2.c0': ('conv3x3_upc<64>', 1),
                          'dec2.c1': ('conv3x3_f16x3_qp', 1),
                          'dec1.c0': ('conv3x3_upc<64>', 1),
                          'dec1.c1': ('conv3x3_f16x3_qp', 1),
                          'dec0.c0': ('conv3x3_up0', 1),
                          'dec0.c1': ('conv3x3_res32', 1),
                          'head': ('head', 1)}),
 ('composed', 'f16'): (None,
                       {'enc0.c0': ('conv3x3_first_split', 1),
                        'enc0.c1': ('conv3x3_res32', 1),
                        'enc1.c0': ('conv3x3s2_v2<64,k32>', 1),
                        'enc1.c1': ('conv3x3_h2', 1),
                        'enc2.c0': ('conv3x3s2_v2<128,k32>', 1),
                        'enc2.c1': ('conv3x3_h2', 1),
                        'enc3.c0': ('conv3x3s2_f16x3', 1),
                        'enc3.c1': ('conv3x3_f16x3', 1),
                        'dec2.c0': ('conv3x3_upc_h2', 1),
                        'dec2.c1': ('conv3x3_h2', 1),
                        'dec1.c0': ('conv3x3_upc_h2', 1),
                        'dec1.c1': ('conv3x3_h2', 1),
                        'dec0.c0': ('conv3x3_up0', 1),
                        'dec0.c1': ('conv3x3_res32', 1),
                        'head': ('head', 1)}),
 ('composed up0=0 q=0 res=0 s2v2=0', 'split'): (('composed', 'split'),
                                                {'enc0.c0': ('conv3x3_first_split', 1),
                                                 'enc0.c1': ('conv3x3_f16x3_one<32>', 1),
                                                 'enc1.c0': ('conv3x3s2_f16x3_one', 1),
                                                 'enc1.c1': ('conv3x3_f16x3_one<64>', 1),
                                                 'enc2.c0': ('conv3x3s2_f16x3_one', 1),
                                                 'enc2.c1': ('conv3x3_f16x3_one<64>', 1),
                                                 'dec2.c1': ('conv3x3_f16x3_one<64>', 1),
                                                 'dec1.c1': ('conv3x3_f16x3_one<64>', 1),
                                                 'dec0.c0': ('conv3x3_upc<32>', 1),
                                                 'dec0.c1': ('conv3x3_f16x3_one<32>', 1)}),
 ('composed up0=0 q=0 res=0 s2v2=0', 'f16'): (('composed', 'f16'),
                                              {'enc0.c1': ('conv3x3_h32<32>', 1),
                                               'enc1.c0': ('conv3x3s2_f16x3_one', 1),
                                               'enc2.c0': ('conv3x3s2_f16x3_one', 1),
                                               'dec0.c0': ('conv3x3_upc_h<32>', 1),
                                               'dec0.c1': ('conv3x3_h32<32>', 1)}),
 ('edge', 'split'): (None,
                     {'enc0.c0': ('conv3x3_first_stats', 1),
                      'enc0.c1': ('conv3x3_res32f', 1),
                      'enc1.c0': ('conv3x3s2_v2<64>', 1),
                      'enc1.c1': ('conv3x3_f16x3_qp', 1),
                      'enc2.c0': ('conv3x3s2_f16x3_one', 1),
                      'enc2.c1': ('conv3x3_f16x3_one<32>', 1),
                      'enc3.c0': ('conv3x3s2_f16x3_one', 1),
                      'enc3.c1': ('conv3x3_f16x3_one<32>', 1),
                      'dec2.c0': ('conv3x3_upc<32>', 1),
                      'dec2.c1': ('conv3x3_f16x3_one<32>', 1),
                      'dec1.c0': ('conv3x3_upq', 1),
                      'dec1.c1': ('conv3x3_f16x3_qp', 1),
                      'dec0.c0': ('conv3x3_up0', 1),
                      'dec0.c1': ('conv3x3_res32', 1),
                      'head': ('head', 1)}),
 ('edge', 'f16'): (None,
                   {'enc0.c0': ('conv3x3_first_split', 1),
                    'enc0.c1': ('conv3x3_res32', 1),
                    'enc1.c0': ('conv3x3s2_v2<64,k32>', 1),
                    'enc1.c1': ('conv3x3_h2', 1),
                    'enc2.c0': ('conv3x3s2_f16x3_one', 1),
                    'enc2.c1': ('conv3x3_h32<32>', 1),
                    'enc3.c0': ('conv3x3s2_f16x3_one', 1),
                    'enc3.c1': ('conv3x3_h32<32>', 1),
                    'dec2.c0': ('conv3x3_upc_h<32>', 1),
                    'dec2.c1': ('conv3x3_h32<32>', 1),
                    'dec1.c0': ('conv3x3_upc_h2', 1),
                    'dec1.c1': ('conv3x3_h2', 1),
                    'dec0.c0': ('conv3x3_up0', 1),
                    'dec0.c1': ('conv3x3_res32', 1),
                    'head': ('head', 1)}),
 ('edge up0=0 q=0 res=0 s2v2=0', 'split'): (('edge', 'split'),
                                            {'enc0.c0': ('conv3x3_first_split', 1),
                                             'enc0.c1': ('conv3x3_f16x3_one<32>', 1),
                                             'enc1.c0': ('conv3x3s2_f16x3_one', 1),
                                             'enc1.c1': ('conv3x3_f16x3_one<64>', 1),
                                             'dec1.c1': ('conv3x3_f16x3_one<64>', 1),
                                             'dec0.c0': ('conv3x3_upc<32>', 1),
                                             'dec0.c1': ('conv3x3_f16x3_one<32>', 1)}),
 ('edge up0=0 q=0 res=0 s2v2=0', 'f16'): (('edge', 'f16'),
                                          {'enc0.c1': ('conv3x3_h32<32>', 1),
                                           'enc1.c0': ('conv3x3s2_f16x3_one', 1),
                                           'dec0.c0': ('conv3x3_upc_h<32>', 1),
                                           'dec0.c1': ('conv3x3_h32<32>', 1)}),
 ('aniso_21', 'split'): (None,
                         {'enc0.c0': ('conv3x3_first_stats', 1),
                          'enc0.c1': ('conv3x3_res32f', 1),
                          'enc1.c0': ('conv3x3s2_v2<64>', 1),
                          'enc1.c1': ('conv3x3_f16x3_qp', 1),
                          'enc2.c0': ('conv3x3s2_v2<128>', 1),
                          'enc2.c1': ('conv3x3_f16x3_qp', 1),
                          'enc3.c0': ('conv_mfma_f32', 1),
                          'enc3.c1': ('conv3x3_f16x3_one<64>', 1),
                          'dec2.up': ('convT_mfma_f32', 1),
                          'dec2.c0': ('conv3x3_f16x3_one<64>', 1),
                          'dec2.c1': ('conv3x3_f16x3_qp', 1),
                          'dec1.c0': ('conv3x3_upc<64>', 1),
                          'dec1.c1': ('conv3x3_f16x3_qp', 1),
                          'dec0.c0': ('conv3x3_up0', 1),
                          'dec0.c1': ('conv3x3_res32', 1),
                          'head': ('head', 1)}),
 ('aniso_21', 'f16'): (None,
                       {'enc0.c0': ('conv3x3_first_split', 1),
                        'enc0.c1': ('conv3x3_res32', 1),
                        'enc1.c0': ('conv3x3s2_v2<64,k32>', 1),
                        'enc1.c1': ('conv3x3_h2', 1),
                        'enc2.c0': ('conv3x3s2_v2<128,k32>', 1),
                        'enc2.c1': ('conv3x3_h2', 1),
                        'enc3.c0': ('conv_mfma_f32', 1),
                        'enc3.c1': ('conv3x3_h32<64>', 1),
                        'dec2.up': ('convT_mfma_f32', 1),
                        'dec2.c0': ('conv3x3_h32<64>', 1),
                        'dec2.c1': ('conv3x3_h2', 1),
                        'dec1.c0': ('conv3x3_upc_h2', 1),
                        'dec1.c1': ('conv3x3_h2', 1),
                        'dec0.c0': ('conv3x3_up0', 1),
                        'dec0.c1': ('conv3x3_res32', 1),
                        'head': ('head', 1)}),
 ('widths', 'split'): (None,
                       {'enc0.c0': ('conv3x3_first_stats', 1),
                        'enc0.c1': ('conv3x3_res32f', 1),
                        'enc1.c0': ('conv3x3s2_v2<64>', 1),
                        'enc1.c1': ('conv3x3_f16x3_qp', 1),
                        'enc2.c0': ('conv3x3s2_f16x3_one', 1),
                        'enc2.c1': ('conv3x3_f16x3_one<32>', 1),
                        'enc3.c0': ('conv_mfma_f32', 1),
                        'enc3.c1': ('conv3x3_f16x3_one<64>', 1),
                        'dec2.up': ('convT_mfma_f32', 1),
                        'dec2.c0': ('conv3x3_f16x3_one<32>', 1),
                        'dec2.c1': ('conv3x3_f16x3_one<32>', 1),
                        'dec1.c0': ('conv3x3_upc<64>', 1),
                        'dec1.c1': ('conv3x3_f16x3_qp', 1),
                        'dec0.c0': ('conv3x3_up0', 1),
                        'dec0.c1': ('conv3x3_res32', 1),
                        'head': ('head', 1)})}


def _table(key, arch=None):
    if key[1] == 'exact':                                   # the exact mode: one kernel per op type, nothing composed, nothing split
        return {o['name']: ({'head': 'head', 'enc0.c0': 'conv3x3_first'}.get(o['name'], 'convT_mfma_f32' if o['name'].endswith('.up') else 'conv_mfma_f32'), 1)
                for o in arch.program()}
    base, diff = TABLES[key]
    t = dict(_table(base)) if base else {}
    for n, v in diff.items():
        if v is None:
            t.pop(n, None)
        else:
            t[n] = tuple(v)
    return t


# ------------------------------------------------------------------------------------------------------------------ helpers
def _engine(arch, blob, **opt):
    e = Engine(arch, blob, options=dict({'sbk': 0}, **opt))
    e.set_profiling(True)
    e.keep_activations(True)
    return e


def _f16_exempt(arch, x):
    """16-bit mode only: blocks of levels with fewer than 64 pixels per image (statistics over a handful of stored fp16 values - the
    exemption of tests/test_gpu_parity.py::test_f16_mode_small_cases), at most the two deepest levels of a case."""
    out = []
    for o in arch.program():
        h, w = arch.extent(o['level'], x.shape[2], x.shape[3])
        if h * w < 64 and o['name'] != 'head':
            assert o['level'] >= arch.n_stages - 2, (o['name'], h, w)
            out.append(o['name'])
    return tuple(out)


def _check(case, e, arch, sd, x, mode, rows=None):
    """One forward in `mode`; the op -> kernel table against TABLES[(case, mode)]; every op that ran under the per-layer oracle."""
    e.set_precision(mode)
    lg, _ = e.forward(x, logits=True)
    ran = {n: v for n, v in _ran(e).items()}
    names = [o['name'] for o in arch.program() if o['name'] in ran]
    assert set(names) == set(ran), (case, mode, sorted(set(ran) - set(names)))
    print(f'[full-batch] {case} {mode} B={x.shape[0]} {x.shape[2]}x{x.shape[3]} table: {ran!r}')
    rows = (0, x.shape[0] - 1) if rows is None else rows
    exempt = _f16_exempt(arch, x) if mode == 'f16' else ()
    err = None
    try:
        worst = LC.check_layers(e, arch, sd, mode, names, rows=tuple(dict.fromkeys(rows)), x=x, logits=lg, exempt=exempt, memo=MEMO)
    except AssertionError as ex:                         # (print the table of the case before failing: the per-op values are in the message)
        err = ex
        worst = {}
    print(f'[full-batch] {case} {mode}: ' + ', '.join(f'{n} {ran[n][0]} S={ran[n][1]} {worst[n]:.2e}' for n in worst))
    want = _table((case, mode), arch)                      # (KeyError: a case without a pinned table)
    assert ran == want, (case, mode, {n: (ran.get(n), want.get(n)) for n in set(ran) | set(want) if ran.get(n) != want.get(n)})
    if err is not None:
        raise err
    storage = 'half' if mode == 'f16' else 'float'
    for n, w in worst.items():
        if n not in exempt:
            SEEN.setdefault((ran[n][0], storage), []).append((case, n, w))
    if 'enc0.c0' in ran and 'enc0.c0' not in worst:      # the statistics pass of the fused first block: judged through enc0.c1
        SEEN.setdefault((ran['enc0.c0'][0], storage), []).append((case, 'enc0.c1', worst['enc0.c1']))
    return ran, worst, lg


def _x40(sd):
    """The transposed convs' biases blown up so that a wrong border variant of a composed decoder entry cannot hide."""
    return {k: ((v * 40.0).astype(np.float32) if ('transpconvs' in k and k.endswith('bias')) else v) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------------------ a. odd batches
@pytest.mark.parametrize('B', [3, 5])
def test_canonical_net_odd_batches_every_op(B):
    arch = UNetArch.canonical()
    sd, blob = blob_for(arch, 1)
    x = cases.make_input(arch, B, 512, 512, 7)
    with _engine(arch, blob) as e:
        for mode in MODES:
            ran, worst, _ = _check(f'canonical B={B}', e, arch, sd, x, mode)
            if mode != 'exact':                              # four images per tile, K split by geometry (choose_ksplit) at 8 x 8 and below
                assert ran['enc6.c1'][1] > 1 and ran['enc7.c1'][1] > 1, ran


# ------------------------------------------------------------------------------------------------------------------ b. ragged levels
def test_canonical_widths_on_640x384_every_op():
    arch = UNetArch.canonical()
    sd, blob = blob_for(arch, 1)
    x = cases.make_input(arch, 2, 640, 384, 3)
    with _engine(arch, blob) as e:
        for mode in MODES:
            ran, _, _ = _check('640x384', e, arch, sd, x, mode)
        # ("flex2" = 2, both modes, is the default and ran above; 1 keeps the level-dividing stride-2 tiles to the 16-bit mode, 0 switches them off)
        for opt, val, back, modes in (('flex', 0, 1, ('split', 'f16')), ('flex2', 0, 2, ('split', 'f16')), ('flex2', 1, 2, ('split',))):
            e.set_option(opt, val)
            for mode in modes:
                _check(f'640x384 {opt}={val}', e, arch, sd, x, mode)
            e.set_option(opt, back)


# ------------------------------------------------------------------------------------------------------------------ c. option twins
TWINS = (({'fuse0': 0}, ('split',)), ({'fuse0': 0, 'first_split': 0}, ('split', 'f16')), ({'up0': 0}, ('split', 'f16')),
         ({'upc': 0}, ('split', 'f16')), ({'q': 0}, ('split',)), ({'s2v2': 0}, ('split', 'f16')), ({'res': 0}, ('split', 'f16')),
         ({'one': 0}, ('split', 'f16')), ({'uh2': 0}, ('f16',)), ({'h2': 0}, ('f16',)), ({'s2k32': 0}, ('f16',)))


def test_option_twins_on_the_canonical_net_every_op():
    arch = UNetArch.canonical()
    sd, blob = blob_for(arch, 1)
    x = cases.make_input(arch, 2, 512, 512, 2)
    with _engine(arch, blob) as e:
        for mode in MODES:
            _check('twins base', e, arch, sd, x, mode)
        for opts, modes in TWINS:
            for k, v in opts.items():
                e.set_option(k, v)
            tag = 'twins ' + ' '.join(f'{k}={v}' for k, v in opts.items())
            for mode in modes:
                ran, _, _ = _check(tag, e, arch, sd, x, mode)
                assert ran != _table(('twins base', mode)), (tag, mode)           # the switch switched something
            for k in opts:
                e.set_option(k, 1)


# ------------------------------------------------------------------------------------------------------------------ d. small nets
def _small(which):
    if which == 'composed':          # tests/test_gpu_parity.py::test_composed_upsampling_block_...: levels 0-2 compose, level 2 has ONE tile per image
        arch = cases.unet(4, (32, 64, 128, 128), 6, cin=2)
        sd = _x40(weights.synthetic_state_dict(arch, 31))
        return arch, sd, weights.pack_blob(arch, sd), cases.make_input(arch, 3, 64, 128, 31), MODES
    if which == 'edge':              # (32, 64, 288, 544): 32-column instances (288 = 9 x 32, 544 = 17 x 32)
        arch = cases.unet(EDGE['n_stages'], EDGE['feats'], EDGE['K'])
        sd, blob = blob_for(arch, 81)
        return arch, sd, blob, cases.make_input(arch, 2, 128, 128, 81), MODES
    if which == 'aniso_21':          # a (2, 1) stage: conv_mfma_f32 / convT_mfma_f32 in every mode
        arch, _, H, W, seed = cases.SMALL_CASES['aniso_21']
        sd, blob = blob_for(arch, seed)
        return arch, sd, blob, cases.make_input(arch, 2, 2 * H, 2 * W, seed), MODES
    arch = cases.unet(4, (16, 48, 80, 100), 5, cin=2, nconv=2, strides=[(1, 1), (2, 2), (2, 2), (2, 1)])      # widths that are no multiples of 32
    sd, blob = blob_for(arch, 77)
    dy, dx = arch.divisors
    return arch, sd, blob, cases.make_input(arch, 2, 8 * dy, 32 * dx, 77), ('split', 'exact')


@pytest.mark.parametrize('which', ['composed', 'edge', 'aniso_21', 'widths'])
def test_small_nets_that_reach_the_other_kernel_names(which):
    arch, sd, blob, x, modes = _small(which)
    with _engine(arch, blob) as e:
        for mode in modes:
            _check(which, e, arch, sd, x, mode)
        if which in ('composed', 'edge'):                    # without the dedicated level-0 entry and the 512-thread kernels: the 32-column instances
            for k in ('up0', 'q', 'res', 's2v2'):
                e.set_option(k, 0)
            for mode in ('split', 'f16'):
                _check(f'{which} up0=0 q=0 res=0 s2v2=0', e, arch, sd, x, mode)


# ------------------------------------------------------------------------------------------------------------------ e. batch invariance, 16-bit
def test_f16_rows_of_a_batch_of_64_equal_those_rows_alone():
    """With a. this carries the per-layer result to the headline size: a row of a B = 64 forward in the 16-bit mode is bit-identical to
    that row alone under the full dispatch (split mode: tests/test_gpu_parity.py::test_full_batch_properties_config2)."""
    import torch
    arch = UNetArch.canonical()
    _, blob = blob_for(arch, 1)
    gen = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(64, 2, 512, 512, device='cuda', generator=gen)
    with Engine(arch, blob, options={'sbk': 0}) as e:
        e.set_precision('f16')
        lg, _ = e.forward(x, logits=True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(lg).all())
        for i in (0, 37, 63):
            li, _ = e.forward(x[i:i + 1].contiguous(), logits=True)
            torch.cuda.synchronize()
            assert torch.equal(li[0], lg[i]), f'row {i} depends on its batch'


# ------------------------------------------------------------------------------------------------------------------ f. coverage of the names
# every string kernel_name() of csrc/dispatch.cpp can return, per storage in which pick_kernel() can choose it
FLOAT_NAMES = ('conv3x3_first_split', 'conv3x3_first', 'conv3x3_first_stats', 'conv_mfma_f32', 'convT_mfma_f32', 'conv3x3_f16x3',
               'conv3x3_f16x3_one<64>', 'conv3x3_f16x3_one<32>', 'conv3x3_f16x3_qp', 'conv3x3_res32', 'conv3x3_res32f', 'conv3x3s2_v2<128>',
               'conv3x3s2_v2<64>', 'conv3x3s2_f16x3_one', 'conv3x3s2_f16x3', 'convT2x2_f16x3', 'conv3x3_up0', 'conv3x3_upq', 'conv3x3_upc<64>',
               'conv3x3_upc<32>', 'head')
HALF_NAMES = ('conv3x3_first_split', 'conv3x3_first', 'conv_mfma_f32', 'convT_mfma_f32', 'conv3x3_f16x3', 'conv3x3_h32<64>', 'conv3x3_h32<32>',
              'conv3x3_h2', 'conv3x3_res32', 'conv3x3s2_v2<128,k32>', 'conv3x3s2_v2<64,k32>', 'conv3x3s2_v2<128>', 'conv3x3s2_v2<64>',
              'conv3x3s2_f16x3_one', 'conv3x3s2_f16x3', 'convT2x2_f16x3', 'conv3x3_up0', 'conv3x3_upc_h<64>', 'conv3x3_upc_h<32>',
              'conv3x3_upc_h2', 'head')
# (name, storage) -> why no case of this module reaches it under the full dispatch
UNREACHED = {}


def test_every_kernel_name_was_seen():
    """Runs last.  A name is seen when an op it served passed the per-layer oracle in some case above (an exempt block does not count)."""
    if not SEEN:
        pytest.skip('the cases of this module did not run in this session')
    for (k, st), v in sorted(SEEN.items()):
        print(f'[full-batch] seen {st:5s} {k:24s} {len(v):3d} ops, worst {max(w for _, _, w in v):.2e} ({max(v, key=lambda t: t[2])[:2]})')
    want = {(n, 'float') for n in FLOAT_NAMES} | {(n, 'half') for n in HALF_NAMES}
    assert set(SEEN) <= want, sorted(set(SEEN) - want)                                # a name this list does not know: restate it
    missing = sorted(want - set(SEEN) - set(UNREACHED))
    assert not missing, missing
    assert not (set(UNREACHED) & set(SEEN)), sorted(set(UNREACHED) & set(SEEN))       # reached after all: take it off the list
