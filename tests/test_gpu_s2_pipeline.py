"""The pipelined split-mode instance of the 512-thread stride-2 kernel (csrc/kernels_s2v2p.h, option "s2p") against its twin, the
single-buffered ``conv3x3s2_v2<128, float, 3>`` ("s2p" = 0), and against the per-layer oracle.

The two instances run the same arithmetic in the same order (same taps, same 16-channel chunks, a fresh accumulator per chunk, the same
epilogue and shifted partials), so everything they produce must agree BIT FOR BIT; both report ``conv3x3s2_v2<128>``.

Net: ``UNetArch.canonical(input_channels=2, num_classes=2, n_stages=3, base=64, max_features=256)``, split mode, full-batch dispatch
("sbk" = 0 for the module: small batches would otherwise go to split-K and never reach the kernel).
  * 256 x 512, B = 5: enc1.c0 64 -> 128 on 128 x 256 outputs = 640 pixel tiles, one column tile, 4 chunks - every workgroup walks two or
    three tiles and crosses image boundaries; enc2.c0 128 -> 256 on 64 x 128 = 160 tiles x 2 column tiles on a 256-workgroup grid, 8
    chunks - ragged streams of one and two tiles.
  * 64 x 128, B = 1: enc1.c0 on 32 x 64 = 8 tiles (top-row, left-column, both-border and interior tiles); enc2.c0 on 16 x 32 = two tiles -
    the pipeline fills and drains on one-tile streams.  Under "sbk" = 0 both ops stay on the fixed-tile kernel at this extent (asserted).

What is compared: ``Engine.debug_tensor`` shows an op's output as its consumer reads it, lrelu(raw * scale + shift) with the scale / shift
derived from the kernel's partials - a function of the raw output and the partials alone, evaluated by the same host code in both runs.
The accessor has no raw form, so the twin test asks for bit equality of that tensor for both stride-2 ops (every element of every row),
of the block behind each (which reads raw, scale and shift on the device) and of the logits."""
import numpy as np
import pytest

from tests import cases
from tests import layer_check as LC
from tests.conftest import blob_for
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.engine import Engine

pytestmark = pytest.mark.gpu

S2_OPS = ('enc1.c0', 'enc2.c0')
KERNEL = 'conv3x3s2_v2<128>'
RUNS = {}            # (B, H, W, s2p) -> (op kernels, {name: tensor}, logits, input): one forward per key, shared by the tests


@pytest.fixture(scope='module', autouse=True)
def _full_batch_dispatch():
    saved = dict(Engine.default_options)
    Engine.default_options = {'sbk': 0}
    yield
    Engine.default_options = saved
    RUNS.clear()


def _net():
    arch = UNetArch.canonical(input_channels=2, num_classes=2, n_stages=3, base=64, max_features=256)
    sd, blob = blob_for(arch, 57)
    return arch, sd, blob


def _run(B, H, W, s2p, keep_engine=False):
    key = (B, H, W, s2p)
    if key in RUNS and not keep_engine:
        return RUNS[key]
    arch, sd, blob = _net()
    x = cases.make_input(arch, B, H, W, 58)
    e = Engine(arch, blob, options={'s2p': s2p})
    e.set_precision('split')
    e.set_profiling(True)
    e.keep_activations(True)
    logits = e.forward(x, logits=True, mask=False)
    logits = np.array(logits[0] if isinstance(logits, tuple) else logits)
    kern = e.op_kernels()
    if keep_engine:
        return e, x, logits, kern
    try:
        t = {n: e.debug_tensor(n) for n in S2_OPS + ('enc1.c1', 'enc2.c1')}
    finally:
        e.close()
    RUNS[key] = (kern, t, logits, x)
    return RUNS[key]


def _twin(B, H, W):
    k1, t1, l1, _ = _run(B, H, W, 1)
    k0, t0, l0, _ = _run(B, H, W, 0)
    for n in S2_OPS:
        assert k1[n] == KERNEL and k0[n] == KERNEL, (n, k1[n], k0[n])
    for n in t1:
        a, b = t1[n], t0[n]
        assert a.shape == b.shape and np.isfinite(a).all(), n
        same = a.view(np.uint32) == b.view(np.uint32)
        assert same.all(), (n, int((~same).sum()), float(np.abs(a - b).max()), [int(v[0]) for v in np.nonzero(~same)])
    assert np.array_equal(l1.view(np.uint32), l0.view(np.uint32))


def test_twin_bit_identity_ragged_streams():
    _twin(5, 256, 512)


def test_twin_bit_identity_borders_and_one_tile_streams():
    _twin(1, 64, 128)


def test_per_layer_oracle():
    """Both stride-2 ops of the pipelined instance, rows 0 and B - 1, under the fixed split-mode block bound of tests/layer_check.py."""
    arch, sd, _ = _net()
    e, x, logits, kern = _run(5, 256, 512, 1, keep_engine=True)
    try:
        for n in S2_OPS:
            assert kern[n] == KERNEL, (n, kern[n])
        worst = LC.check_layers(e, arch, sd, 'split', S2_OPS, rows=(0, 4), x=x, logits=logits)
    finally:
        e.close()
    print({n: f'{v:.2e}' for n, v in worst.items()})
