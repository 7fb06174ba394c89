"""The device export (resample-back + threshold behind the sliding window) as far as it goes without a GPU: the numpy statement of its
arithmetic pinned to scipy, the C-ABI of ts2d_engine_predict_tiled_export (header, exports, binding, structure layout), the
emitted instruction stream of sw_resample_threshold (no fused multiply-add, no scratch) and the routing of a resampled case through
``HIPModel._run`` with a host double of the predictor's engine method."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests.batch_util import HostBatchModel, HostBatchPredictor
from tests.conftest import ROOT
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, nrrd
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.export import SIGMOID_HALF_THRESHOLD

HIPCC = '/opt/rocm/bin/hipcc'


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _shape_pairs(n, seed):
    """Seeded (input shape, output shape) pairs: down, up, mixed, equal, axes of length 1."""
    rng = np.random.default_rng(seed)
    pairs = [((7, 9), (7, 9)), ((1, 13), (5, 40)), ((12, 1), (3, 1)), ((1, 1), (4, 6)), ((40, 30), (1, 1)), ((33, 47), (80, 20)),
             ((64, 52), (107, 65)), ((100, 60), (50, 30))]
    while len(pairs) < n:
        pairs.append((tuple(int(v) for v in rng.integers(1, 90, 2)), tuple(int(v) for v in rng.integers(1, 140, 2))))
    return pairs


def _same_bits(got, ref):
    """Every float32 value bit-equal; NaN in the same places (a NaN's payload is the producer's own)."""
    nan = np.isnan(ref)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(ref)[~nan])


def test_linear_restatement_equals_scipy_bit_for_bit():
    """float16-valued input (what the engine aggregates into: upstream's half buffers) at three magnitudes, subnormal halves included, and
    full float32 input: every value of every pair is bit-equal to ``resize_like_skimage(order=1)``.  It takes scipy's own order to get
    there - unclamped coordinate with clamped tap indices, each sample times its row weight, then times its column weight: with the
    weights multiplied first, or the coordinate clamped, about two values in 100 000 differ by one float32 ulp."""
    rng = np.random.default_rng(5)
    pairs = _shape_pairs(240, 6)
    kinds = {'down': 0, 'up': 0, 'equal': 0, 'one': 0}
    total = 0
    for i, (si, so) in enumerate(pairs):
        scale = (1.0, 40.0, 1e-5)[i % 3]
        img = (rng.standard_normal(si) * scale).astype(np.float32)
        if i % 4:
            img = img.astype(np.float16).astype(np.float32)
        ref = P.resize_like_skimage(img, so, 1)
        got = P.resize_linear_f64(img, so)
        assert got.dtype == np.float32 and got.shape == tuple(so)
        assert np.array_equal(_bits(got), _bits(ref)), (si, so)
        # the clip that follows in resize_like_skimage is a no-op for order 1
        assert got.min() >= img.min() and got.max() <= img.max()
        for a, b in zip(si, so):
            kinds['down' if b < a else 'up' if b > a else 'equal'] += 1
            kinds['one'] += a == 1
        total += got.size
    assert all(v >= 8 for v in kinds.values()) and total > 500_000, (kinds, total)


def test_infinite_samples_propagate_as_in_scipy():
    """+-inf half logits (upstream aborts on an inf in the aggregated array before it exports, and so does the predictor; restatement
    and kernel still agree with scipy): scipy multiplies every tap, so an inf with weight gives +-inf, a zero weight on an inf gives NaN
    and so does +inf beside -inf.  Because scipy extends the array instead of clamping the coordinate, an output left of the first sample
    weighs that sample twice and never sees its neighbour.  Same NaNs, same bits elsewhere, same threshold decision."""
    from scipy import ndimage as ndi
    rng = np.random.default_rng(9)
    n_nan = n_inf = 0
    for si, so in _shape_pairs(60, 10):
        if tuple(si) == tuple(so):
            continue
        img = rng.standard_normal(si).astype(np.float16)
        flat = img.reshape(-1)
        flat[rng.integers(0, flat.size, max(1, flat.size // 12))] = np.inf
        flat[rng.integers(0, flat.size, max(1, flat.size // 20))] = -np.inf
        img = img.astype(np.float32)
        with np.errstate(invalid='ignore'):
            ref = ndi.zoom(img, [o / i for o, i in zip(so, si)], order=1, mode='nearest', grid_mode=True)
        got = P.resize_linear_f64(img, so)
        assert _same_bits(got, ref), (si, so)
        assert np.array_equal(got > SIGMOID_HALF_THRESHOLD, ref > SIGMOID_HALF_THRESHOLD)
        n_nan += int(np.isnan(ref).sum())
        n_inf += int(np.isinf(ref).sum())
    assert n_nan > 100 and n_inf > 100
    a = np.array([[1.0, np.inf, 2.0, 3.0], [0.5, 0.25, 4.0, 8.0]], np.float32)
    up = P.resize_linear_f64(a, (4, 8))
    assert up[0, 0] == 1.0 and np.isposinf(up[0, 1])          # left of the first sample: the edge sample twice; an inf with weight
    b = np.array([[1.0, 7.0, np.inf, 3.0, 4.0, 5.0]], np.float32)
    assert np.isnan(P.resize_linear_f64(b, (1, 2))[0, 0])      # cc = 1 exactly: the inf neighbour has weight 0, and 0 x inf = NaN
    with np.errstate(invalid='ignore'):
        assert _same_bits(up, ndi.zoom(a, (2, 2), order=1, mode='nearest', grid_mode=True))


def test_export_entry_is_declared_exported_and_bound():
    src = open(_lib.HEADER_PATH).read()
    body = re.search(r'typedef struct \{([^}]*)\} ts2d_tiled_export;', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        size = 8 if '*' in decl else 4
        names = decl.replace('*', ' ').split(None, 1)[1]
        fields += [(n.strip(), size) for n in names.split(',')]
    assert [n for n, _ in fields] == ['src_y', 'src_x', 'src_h', 'src_w', 'out_h', 'out_w', 'seg_u8', 'logits_f32']
    off = 0
    for n, size in fields:
        off = (off + size - 1) // size * size
        assert getattr(_lib.TiledExport, n).offset == off and getattr(_lib.TiledExport, n).size == size, n
        off += size
    assert ctypes.sizeof(_lib.TiledExport) == off == 40
    assert [f[0] for f in _lib.TiledExport._fields_] == [n for n, _ in fields]
    assert re.search(r'int ts2d_engine_predict_tiled_export\(ts2d_engine\* e, ts2d_tiled_image\* images, const ts2d_tiled_export\* exports, '
                     r'int n_images,\s*int patch_h, int patch_w, int mirror_mask, const uint16_t\* gaussian_f16, int full_batch\);', src)
    lib = _lib.load()
    assert 'ts2d_engine_predict_tiled_export' in _lib.SYMBOLS and hasattr(lib, 'ts2d_engine_predict_tiled_export')
    assert lib.ts2d_abi_version() == _lib.ABI_VERSION == 9             # new symbols only: no existing signature changed
    assert ctypes.sizeof(_lib.TiledImage) == 64
    desc, exd = (_lib.TiledImage * 1)(), (_lib.TiledExport * 1)()
    assert lib.ts2d_engine_predict_tiled_export(None, desc, exd, 1, 64, 64, 0, None, 1) == -1
    assert 'ts2d_engine_predict_tiled_export: null engine' in _lib.last_error()


@pytest.fixture(scope='module')
def resample_asm(tmp_path_factory):
    """kernels_resample.h alone, compiled to gfx950 assembly with the device flags of the shipped build (csrc/Makefile DEVFLAGS)."""
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    d = tmp_path_factory.mktemp('resample_isa')
    csrc = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
    tu = d / 'resample.hip'
    tu.write_text(f'#include "{os.path.join(csrc, "kernels_resample.h")}"\n')
    devflags = subprocess.check_output(['make', '-s', '-C', csrc, 'flags'], text=True).split()
    subprocess.check_call([HIPCC, '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S', *devflags, '-o', str(d / 'resample.s'), str(tu)],
                          stderr=subprocess.DEVNULL)
    return open(d / 'resample.s').read()


def test_resample_kernel_has_no_fused_multiply_add_and_no_scratch(resample_asm):
    m = re.search(r'^(_ZN4ts2d21sw_resample_threshold\w*):', resample_asm, re.M)
    assert m, 'sw_resample_threshold not found in the assembly'
    body = resample_asm[m.end():resample_asm.index('.Lfunc_end', m.end())]
    ops = [ln.split()[0] for ln in body.split('\n') if ln.strip() and not ln.strip().startswith((';', '.'))]
    fused = [o for o in ops if 'f64' in o and ('fma' in o or 'mad' in o)]          # v_fma_f64, v_fmac_f64, ...
    assert not fused, f'a float64 product was fused into its sum ({fused[0]}): bit-identity with the host statement is gone'
    assert sum(o == 'v_mul_f64' for o in ops) >= 8 and sum(o == 'v_add_f64' for o in ops) >= 3
    assert not [o for o in ops if o.startswith('scratch_')], 'sw_resample_threshold spills registers'
    meta = resample_asm[resample_asm.index('amdhsa.kernels:'):]
    blk = next(b for b in re.split(r'\n  - \.', meta)[1:] if 'sw_resample_threshold' in b)
    assert re.search(r'private_segment_fixed_size:\s*0\b', blk) and re.search(r'vgpr_spill_count:\s*0\b', blk)
    assert re.search(r'group_segment_fixed_size:\s*0\b', blk)           # no LDS either: pure memory traffic


# ------------------------------------------------------------------------------------------------ routing through HIPModel._run
class _ExportDouble(HostBatchPredictor):
    """Host double of the one predictor method that touches the engine, WITH the device export: the restatement of the sliding window
    (tests/host_predictor.py) followed by the numpy statement of sw_resample_threshold."""
    def _create_engines(self):
        self.engines = [SimpleNamespace(close=lambda: None)]           # (the single-case fast path asks for exactly one engine)
        self.calls = []

    def _sliding_window_batch(self, list_of_data, fold=0, want_seg=False, one_call=True, out_shapes=None):
        self.calls.append((len(list_of_data), want_seg, one_call, None if out_shapes is None else list(out_shapes)))
        logits = super()._sliding_window_batch(list_of_data, fold, False)
        if not want_seg:
            return logits
        out = []
        for lg, hw in zip(logits, out_shapes or [None] * len(logits)):
            lg = lg.astype(np.float32)
            if hw is not None:
                lg = np.stack([P.resize_linear_f64(pl[0], hw) for pl in lg])[:, None]
            out.append((lg > SIGMOID_HALF_THRESHOLD).astype(np.uint8))
        return out


class _ExportModel(HostBatchModel):
    def _make_predictor(self, kw):
        return _ExportDouble(network=self._config['oracle_network'], **kw)


def _image(seed, hw, spacing):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(hw + (2,)) * 300).astype(np.float32)
    return nrrd.Image(a, spacing, (3.0, -7.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


def test_a_resampled_case_joins_the_fast_group_and_exports_the_host_routes_bytes():
    m0, _, _ = synthetic_model('ts2d-v2-ep4000b2_cardiac', 3, 41, mirror=True, network=True, feats=(32, 32))
    m = _ExportModel(m0._config)
    imgs = {'off': _image(1, (70, 90), (0.9, 1.2)),            # -> 56 x 54 at the plan's (1.5, 1.5): smaller than the 64 x 64 patch
            'on': _image(2, (80, 70), (1.5, 1.5)),             # the plan's spacing: no resampling
            'up': _image(3, (40, 45), (2.5, 2.0))}             # -> 53 x 75: the logits are resampled DOWN to 40 x 45
    m.start()
    try:
        p = m._predictor
        m.device_threshold = False
        p.calls.clear()
        want = m.apply_batch(dict(imgs))
        assert [c[1] for c in p.calls] == [False]                       # host route: logits, scipy, threshold
        m.device_threshold = True
        p.calls.clear()
        got = m.apply_batch(dict(imgs))
        assert p.calls == [(3, True, True, [(70, 90), None, (40, 45)])]  # ONE call: every case in the fast group, with its target extent
        p.calls.clear()
        one = m.apply(imgs['off'])
        assert p.calls == [(1, True, False, [(70, 90)])]
    finally:
        m.stop()
    for k, img in imgs.items():
        assert got[k].array.dtype == np.uint8 and got[k].array.shape == img.array.shape[:2] + (3,)
        assert np.array_equal(got[k].array, want[k].array), k
        assert got[k].spacing == img.spacing and got[k].origin == img.origin and got[k].direction == img.direction
        assert got[k].meta == want[k].meta
    assert np.array_equal(one.array, want['off'].array) and 0 < want['off'].array.mean() < 1


def test_a_predictor_without_the_export_keyword_keeps_the_host_route():
    """tests/batch_util.HostBatchPredictor overrides the engine method as (list, fold, want_seg): a resampled case must not reach it with
    ``out_shapes=`` - it takes the logits route, as before the device export existed, and the un-resampled case keeps the fast path."""
    m0, _, _ = synthetic_model('ts2d-v2-ep4000b2_cardiac', 3, 41, mirror=False, network=True, feats=(32, 32))
    m = HostBatchModel(m0._config)
    imgs = {'off': _image(1, (70, 90), (0.9, 1.2)), 'on': _image(2, (80, 70), (1.5, 1.5))}
    m.start()
    try:
        calls = []
        orig = m._predictor._sliding_window_batch
        m._predictor._sliding_window_batch = lambda datas, fold=0, want_seg=False: (calls.append((len(datas), want_seg)), orig(datas, fold, want_seg))[1]
        got = m.apply_batch(dict(imgs))
        assert sorted(calls) == [(1, False), (1, True)]
        m.device_threshold = False
        want = m.apply_batch(dict(imgs))
    finally:
        m.stop()
    assert all(np.array_equal(got[k].array, want[k].array) and got[k].array.shape == imgs[k].array.shape[:2] + (3,) for k in imgs)


def test_out_shape_forms_and_refusals():
    p = _ExportDouble(network=None)
    d = np.zeros((2, 1, 10, 12), np.float32)
    assert p._in_plane(None, d) is None and p._in_plane((10, 12), d) is None and p._in_plane((1, 10, 12), d) is None
    assert p._in_plane((1, 20, 6), d) == (20, 6) and p._in_plane((20, 6), d) == (20, 6)
    assert p._in_plane((2, 20, 6), d) is False and p._in_plane((0, 6), d) is False          # a stack / an empty extent: not the device export's
