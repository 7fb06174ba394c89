"""The device export of a LABEL-MAP model (resample-back + argmax over the heads behind the sliding window) as far as it goes without a
GPU: the numpy statement of its arithmetic against today's host route, the comparator of the kernel compiled for the host and exhausted
against np.argmax, the emitted instruction stream of sw_labelmap (no fused multiply-add, no scratch), the C-ABI of the new entries
(header, exports, binding, structure layout) and the routing of a non-multilabel model through ``HIPModel._run`` with host doubles."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests.batch_util import HostBatchModel, HostBatchPredictor
from tests.conftest import ROOT
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, export, nrrd
from totalsegmentator2d_amd import preprocess as P

HIPCC = '/opt/rocm/bin/hipcc'
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')


# ------------------------------------------------------------------------------------------------ the statement against the host route
def _props(hw):
    hw = tuple(int(v) for v in hw)
    return {'shape_after_cropping_and_before_resampling': (1,) + hw, 'shape_before_cropping': (1,) + hw,
            'bbox_used_for_cropping': [(0, 1), (0, hw[0]), (0, hw[1])]}


def _host_route(case_f16, out_hw):
    """Today's export of a label-map model: the case's half logits [K,h,w] -> resample_data_to_shape(order=1) -> argmax, uint8 [H0,W0]."""
    seg = export.convert_predicted_logits_to_segmentation_with_correct_shape(case_f16[:, None], _props(out_hw), multilabel=False)
    assert seg.dtype == np.uint8 and seg.shape == (1,) + tuple(out_hw)
    return seg[0]


def _halves(rng, shape, levels=None):
    """Random halves; with `levels`, drawn from that few distinct values, so that heads tie exactly."""
    if levels:
        return rng.choice((rng.standard_normal(levels) * 3).astype(np.float16), size=shape)
    return (rng.standard_normal(shape) * 4).astype(np.float16)


# (case extent, export extent): up, down, mixed, identity, odd widths, widths that are no multiples of 4, an axis kept while the other moves
EXTENTS = [((20, 28), (33, 47)), ((31, 22), (12, 9)), ((17, 30), (40, 13)), ((19, 23), (19, 23)), ((16, 16), (16, 16)), ((9, 14), (9, 31)),
           ((24, 7), (50, 7)), ((1, 5), (3, 10)), ((12, 12), (1, 1))]


@pytest.mark.parametrize('K', [2, 3, 18, 256])
def test_statement_equals_the_host_route_byte_for_byte(K):
    rng = np.random.default_rng(100 + K)
    seen = set()
    for i, (hw, out) in enumerate(EXTENTS):
        y, x = (0, 0) if i % 3 == 0 else (int(rng.integers(0, 6)), int(rng.integers(0, 6)))
        Hp, Wp = y + hw[0] + int(rng.integers(0, 5)), x + hw[1] + int(rng.integers(0, 5))
        padded = _halves(rng, (K, Hp, Wp), levels=None if i % 2 else 5)
        got = export.labelmap_statement(padded, (y, x) + hw, out)
        want = _host_route(padded[:, y:y + hw[0], x:x + hw[1]], out)
        assert got.dtype == np.uint8 and got.shape == tuple(out)
        assert np.array_equal(got, want), (K, hw, out)
        seen |= set(np.unique(got).tolist())
    assert len(seen) >= min(K, 10) and max(seen) < K


def test_statement_keeps_the_identity_case_unresampled_as_the_host_route_does():
    """An infinite logit at the case's own extent stays infinite on the host route (it does not resample) and wins; resampled, the same
    plane meets zero weights (0 x inf = NaN, as in scipy) and the first NaN wins instead.  The statement follows the host route in both."""
    rng = np.random.default_rng(7)
    lg = _halves(rng, (4, 12, 10))
    lg[2, 5, 4] = np.inf
    lg[1, 3, 3] = -np.inf
    lg[3, 8, 8] = np.nan
    lg[1, 8, 8] = np.nan
    same = export.labelmap_statement(lg, (0, 0, 12, 10), (12, 10))
    assert np.array_equal(same, _host_route(lg, (12, 10)))
    assert same[5, 4] == 2 and same[8, 8] == 1 and same[3, 3] != 1
    # resampled: infinite SOURCE samples only (a NaN source sample makes the host route's whole plane NaN through skimage's clip to the
    # plane's [min, max]; the engine refuses NaN logits long before the export, ts2d_engine_check)
    lg[3, 8, 8], lg[1, 8, 8] = 1.0, 2.0
    nans = 0
    with np.errstate(invalid='ignore'):
        for out in [(24, 20), (12, 20), (7, 10), (6, 5)]:     # (one axis kept: the host route resamples the whole plane all the same)
            assert np.array_equal(export.labelmap_statement(lg, (0, 0, 12, 10), out), _host_route(lg, out)), out
            nans += int(np.isnan(np.stack([P.resize_linear_f64(pl.astype(np.float32), out) for pl in lg])).sum())
        wide = export.labelmap_statement(lg, (0, 0, 12, 10), (12, 20))
    assert nans > 0                                           # a zero weight met an infinite sample: the first NaN decided those pixels
    assert (wide[5] == 2).sum() >= 2 and wide[5, 8] == 2      # the +inf of head 2 spreads over its neighbours


def test_a_uint8_prediction_of_a_label_map_model_is_exported_unchanged():
    plane = np.random.default_rng(3).integers(0, 200, (1, 1, 9, 11)).astype(np.uint8)
    props = {'shape_after_cropping_and_before_resampling': (1, 9, 11), 'shape_before_cropping': (1, 14, 15),
             'bbox_used_for_cropping': [(0, 1), (2, 11), (3, 14)]}
    seg = export.convert_predicted_logits_to_segmentation_with_correct_shape(plane, props, multilabel=False)
    assert seg.dtype == np.uint8 and seg.shape == (1, 14, 15) and np.array_equal(seg[0, 2:11, 3:14], plane[0, 0])
    assert seg.sum() == plane.sum()
    with pytest.raises(ValueError, match='one plane of labels'):
        export.convert_predicted_logits_to_segmentation_with_correct_shape(np.zeros((3, 1, 9, 11), np.uint8), props, multilabel=False)


# ------------------------------------------------------------------------------------------------ the comparator
@pytest.fixture(scope='module')
def host_argmax(tmp_path_factory):
    """csrc/labelmap_cmp.h compiled as plain C++ for the host: the walk over the heads the kernel makes, as a C function."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    d = tmp_path_factory.mktemp('labelmap_cmp')
    src = d / 'cmp.cpp'
    src.write_text(f'#include "{os.path.join(CSRC, "labelmap_cmp.h")}"\n'
                   'extern "C" int lm_argmax(const float* v, int n) {\n'
                   '    float best = 0.f; int idx = 0;\n'
                   '    for (int k = 0; k < n; ++k)\n'
                   '        if (k == 0 || ts2d::lm_replaces(v[k], best)) { best = v[k]; idx = k; }\n'
                   '    return idx;\n}\n')
    so = d / 'cmp.so'
    subprocess.check_call([cxx, '-x', 'c++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', str(so), str(src)])
    fn = ctypes.CDLL(str(so)).lm_argmax
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]
    return lambda v: fn(np.ascontiguousarray(v, np.float32).ctypes.data, len(v))


def _special_values():
    h = lambda bits: np.array(bits, np.uint16).view(np.float16).astype(np.float32)                  # noqa: E731
    f = lambda bits: np.array(bits, np.uint32).view(np.float32)                                     # noqa: E731
    vals = [np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), -np.float32(np.nan),
            f(0x7FC00001), f(0x7F800001),                                # NaNs of other payloads, a signalling one
            h(0x0001), h(0x8001), h(0x0002), h(0x03FF), h(0x0400),       # half subnormals and the first normal
            f(0x00000001), f(0x80000001), f(0x007FFFFF),                 # float32 subnormals
            h(0x3C00), h(0x3C01), h(0x3BFF), h(0xBC00), h(0xBC01),       # 1 and its half neighbours, both signs
            h(0x7BFF), h(0xFBFF), h(0x7BFE),                             # +-65504 and the half below
            f(0x3F800001), np.float32(1.5 * 2.0 ** -24)]
    return [np.float32(v) for v in vals]


def test_comparator_is_numpys_argmax_on_every_ordered_pair_and_triple(host_argmax):
    vals = _special_values()
    assert sum(np.isnan(v) for v in vals) == 4 and len(vals) >= 26
    n = 0
    for r in (2, 3):
        for combo in itertools.product(vals, repeat=r):
            a = np.array(combo, np.float32)
            assert host_argmax(a) == int(np.argmax(a)), [hex(int(b)) for b in a.view(np.uint32)]
            n += 1
    assert n == len(vals) ** 2 + len(vals) ** 3
    # the cases by name: first maximum, signed zeros equal, a NaN beats everything, the first NaN stays
    assert host_argmax([1.0, 2.0, 2.0]) == 1 and host_argmax([0.0, -0.0]) == 0 and host_argmax([-0.0, 0.0]) == 0
    assert host_argmax([np.inf, np.nan, np.inf]) == 1 and host_argmax([np.nan, np.inf]) == 0 and host_argmax([1.0, np.nan, -np.nan]) == 1
    rng = np.random.default_rng(2)
    for _ in range(300):                                                 # longer walks over few distinct values
        a = rng.choice(np.array(vals, np.float32), size=int(rng.integers(1, 40)))
        assert host_argmax(a) == int(np.argmax(a))


# ------------------------------------------------------------------------------------------------ the instruction stream
@pytest.fixture(scope='module')
def labelmap_asm(tmp_path_factory):
    """kernels_labelmap.h alone, compiled to gfx950 assembly with the device flags of the shipped build (csrc/Makefile DEVFLAGS)."""
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    d = tmp_path_factory.mktemp('labelmap_isa')
    tu = d / 'labelmap.hip'
    tu.write_text(f'#include "{os.path.join(CSRC, "kernels_labelmap.h")}"\n')
    devflags = subprocess.check_output(['make', '-s', '-C', CSRC, 'flags'], text=True).split()
    subprocess.check_call([HIPCC, '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S', *devflags, '-o', str(d / 'labelmap.s'), str(tu)],
                          stderr=subprocess.DEVNULL)
    return open(d / 'labelmap.s').read()


def test_labelmap_kernel_has_no_fused_multiply_add_and_no_scratch(labelmap_asm):
    m = re.search(r'^(_ZN4ts2d11sw_labelmap\w*):', labelmap_asm, re.M)
    assert m, 'sw_labelmap not found in the assembly'
    body = labelmap_asm[m.end():labelmap_asm.index('.Lfunc_end', m.end())]
    ops = [ln.split()[0] for ln in body.split('\n') if ln.strip() and not ln.strip().startswith((';', '.'))]
    fused = [o for o in ops if 'f64' in o and ('fma' in o or 'mad' in o)]          # v_fma_f64, v_fmac_f64, ...
    assert not fused, f'a float64 product was fused into its sum ({fused[0]}): bit-identity with the host statement is gone'
    assert sum(o == 'v_mul_f64' for o in ops) >= 8 and sum(o == 'v_add_f64' for o in ops) >= 3
    assert not [o for o in ops if o.startswith('scratch_')], 'sw_labelmap spills registers'
    meta = labelmap_asm[labelmap_asm.index('amdhsa.kernels:'):]
    blk = next(b for b in re.split(r'\n  - \.', meta)[1:] if 'sw_labelmap' in b)
    assert re.search(r'private_segment_fixed_size:\s*0\b', blk) and re.search(r'vgpr_spill_count:\s*0\b', blk)
    assert re.search(r'group_segment_fixed_size:\s*0\b', blk)           # no LDS either: pure memory traffic


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_labelmap_entries_are_declared_exported_and_bound():
    src = open(_lib.HEADER_PATH).read()
    body = re.search(r'typedef struct \{([^}]*)\} ts2d_tiled_labelmap;', src, re.S)
    assert body, 'ts2d_tiled_labelmap is not declared in include/ts2d_engine.h'
    body = re.sub(r'/\*.*?\*/', '', body.group(1), flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        size = 8 if '*' in decl else 4
        names = decl.replace('*', ' ').split(None, 1)[1]
        fields += [(n.strip(), size) for n in names.split(',')]
    assert [n for n, _ in fields] == ['src_y', 'src_x', 'src_h', 'src_w', 'out_h', 'out_w', 'label_u8']
    off = 0
    for n, size in fields:
        off = (off + size - 1) // size * size
        assert getattr(_lib.TiledLabelmap, n).offset == off and getattr(_lib.TiledLabelmap, n).size == size, n
        off += size
    assert ctypes.sizeof(_lib.TiledLabelmap) == off == 32
    assert re.search(r'int ts2d_ensemble_predict_tiled_labelmap\(ts2d_engine\* const\* engines, int n_engines, ts2d_tiled_image\* images, '
                     r'const ts2d_tiled_labelmap\* labelmaps,\s*int n_images, int patch_h, int patch_w, int mirror_mask, '
                     r'const uint16_t\* gaussian_f16, int full_batch\);', src)
    assert re.search(r'int ts2d_labelmap_from_logits\(int device, const uint16_t\* logits_f16, int K, int H, int W, const int32_t rect\[4\], '
                     r'int out_h, int out_w,\s*uint8_t\* label_u8\);', src)
    lib = _lib.load()
    for name in ('ts2d_ensemble_predict_tiled_labelmap', 'ts2d_labelmap_from_logits'):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.ts2d_abi_version() == _lib.ABI_VERSION == 9             # new symbols only: no existing signature or structure changed
    assert ctypes.sizeof(_lib.TiledImage) == 64 and ctypes.sizeof(_lib.TiledExport) == 40
    # refused before any device work, by name
    desc, lmd = (_lib.TiledImage * 1)(), (_lib.TiledLabelmap * 1)()
    assert lib.ts2d_ensemble_predict_tiled_labelmap(None, 1, desc, lmd, 1, 64, 64, 0, None, 1) == -1
    assert 'ts2d_ensemble_predict_tiled_labelmap: 1 engines at a null pointer' in _lib.last_error()
    handles = (ctypes.c_void_p * 1)(None)
    assert lib.ts2d_ensemble_predict_tiled_labelmap(handles, 1, desc, lmd, 1, 64, 64, 0, None, 1) == -1
    assert 'ts2d_ensemble_predict_tiled_labelmap: engine 0 is null' in _lib.last_error()
    assert lib.ts2d_ensemble_predict_tiled_labelmap(handles, 0, desc, lmd, 1, 64, 64, 0, None, 1) == -1 and 'outside 1..32' in _lib.last_error()
    lg, out, rect = np.zeros((2, 8, 8), np.float16), np.zeros((5, 5), np.uint8), (ctypes.c_int32 * 4)(0, 0, 8, 8)
    p, o, r = lg.ctypes.data, out.ctypes.data, ctypes.byref(rect)
    for args, word in [((0, None, 2, 8, 8, r, 5, 5, o), 'null argument'), ((0, p, 2, 8, 8, None, 5, 5, o), 'null argument'),
                       ((0, p, 2, 8, 8, r, 5, 5, None), 'null argument'), ((0, p, 0, 8, 8, r, 5, 5, o), '0 heads outside 1 ... 256'),
                       ((0, p, 257, 8, 8, r, 5, 5, o), '257 heads'), ((0, p, 2, 0, 8, r, 5, 5, o), 'bad extent'),
                       ((0, p, 2, 8, 7, r, 5, 5, o), 'source rectangle 8x8 at (0,0) is empty or leaves the 8x7 image'),
                       ((0, p, 2, 8, 8, r, 0, 5, o), 'bad output extent 0x5'), ((0, p, 2, 8, 8, r, 1 << 16, 1 << 16, o), 'exceeds 2^31')]:
        assert lib.ts2d_labelmap_from_logits(*args) == -1, word
        assert 'ts2d_labelmap_from_logits' in _lib.last_error() and word in _lib.last_error(), (_lib.last_error(), word)
    assert not out.any()


# ------------------------------------------------------------------------------------------------ routing through HIPModel._run
def _labelmap_config(K=4, seed=43, mirror=True):
    """A synthetic LABEL-MAP sub-model: K heads = background + K - 1 labels, not multilabel."""
    m0, _, _ = synthetic_model('ts2d-v2-ep4000b2_cardiac', K, seed, mirror=mirror, network=True, feats=(32, 32))
    cfg = dict(m0._config)
    syn = dict(cfg['synthetic'])
    syn['dataset_json'] = {'channel_names': {'0': 'mean', '1': 'max'}, 'labels': {'background': 0, **{f'cardiac_{i}': i for i in range(1, K)}},
                           'file_ending': '.nrrd'}
    cfg['synthetic'] = syn
    cfg['param'] = dict(cfg['param'], **{'nnu.result.colors': None})
    return cfg


def _image(seed, hw, spacing):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(hw + (2,)) * 300).astype(np.float32)
    return nrrd.Image(a, spacing, (3.0, -7.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


def _cases():
    return {'off': _image(1, (70, 90), (0.9, 1.2)),            # -> 56 x 54 at the plan's (1.5, 1.5): smaller than the 64 x 64 patch
            'on': _image(2, (80, 70), (1.5, 1.5)),             # the plan's spacing: no resampling
            'up': _image(3, (40, 45), (2.5, 2.0))}             # -> 53 x 75: the logits are resampled DOWN to 40 x 45


class _Recorder:
    """Every call of the predictor methods the model may use, in order: (name, number of inputs, keywords)."""
    NAMES = ['predict_logits_from_preprocessed_data', 'predict_logits_from_preprocessed_data_batch',
             'predict_segmentation_from_preprocessed_data', 'predict_segmentation_from_preprocessed_data_batch',
             'predict_labelmap_from_preprocessed_data', 'predict_labelmap_from_preprocessed_data_batch']

    def __init__(self, predictor, returned=None):
        self.calls = []
        for name in self.NAMES:
            orig = getattr(predictor, name, None)
            if orig is None:
                continue

            def wrapped(data, *a, _o=orig, _n=name, **kw):
                out = _o(data, *a, **kw)
                self.calls.append((_n, len(data) if _n.endswith('_batch') else 1, dict(kw)))
                if returned is not None and 'labelmap' in _n:
                    returned.extend(out if _n.endswith('_batch') else [out])
                return out
            setattr(predictor, name, wrapped)


def test_a_predictor_without_the_labelmap_route_takes_exactly_the_old_path():
    """tests/batch_util.HostBatchPredictor restates the engine method as (list, fold, want_seg): no `labelmap` keyword, so a label-map model
    over it keeps the reference seam - logits from the predictor, resample and argmax in the export - whatever ``device_labelmap`` says."""
    m = HostBatchModel(_labelmap_config())
    imgs = _cases()
    assert not m.multilabel
    m.start()
    try:
        rec = _Recorder(m._predictor)
        runs = {}
        for switch in (True, False):
            m.device_labelmap = switch
            del rec.calls[:]
            many = m.apply_batch(dict(imgs))
            one = {k: m.apply(v) for k, v in imgs.items()}
            runs[switch] = (many, one, list(rec.calls))
    finally:
        m.stop()
    want_calls = [('predict_logits_from_preprocessed_data_batch', 3, {})] + [('predict_logits_from_preprocessed_data', 1, {})] * 3
    assert runs[True][2] == runs[False][2] == want_calls
    for k, img in imgs.items():
        a = runs[True][0][k]
        assert a.array.dtype == np.uint8 and a.array.shape == img.array.shape[:2] and 0 < a.array.max() < 4
        for other in (runs[True][1][k], runs[False][0][k], runs[False][1][k]):
            assert np.array_equal(a.array, other.array) and a.meta == other.meta


class _LabelmapDouble(HostBatchPredictor):
    """Host double of the one predictor method that touches the engine, WITH the label-map route: the restatement of the sliding window
    (tests/host_predictor.py) followed by the numpy statement of sw_labelmap."""
    def _create_engines(self):
        self.engines = [SimpleNamespace(close=lambda: None)]           # (the fast path asks for exactly one engine)
        self.engine_calls = []

    def _sliding_window_batch(self, list_of_data, fold=0, want_seg=False, one_call=True, out_shapes=None, labelmap=False):
        self.engine_calls.append((len(list_of_data), labelmap, one_call, None if out_shapes is None else list(out_shapes)))
        logits = super()._sliding_window_batch(list_of_data, fold, False)
        if not labelmap:
            return logits
        return [export.labelmap_statement(lg[:, 0], (0, 0) + lg.shape[2:], hw if hw is not None else lg.shape[2:])[None, None]
                for lg, hw in zip(logits, out_shapes)]


class _LabelmapModel(HostBatchModel):
    def _make_predictor(self, kw):
        return _LabelmapDouble(network=self._config['oracle_network'], **kw)


def test_a_predictor_with_the_labelmap_route_is_asked_once_per_case_and_its_plane_is_exported_unchanged():
    m = _LabelmapModel(_labelmap_config())
    imgs = _cases()
    m.start()
    try:
        p = m._predictor
        returned = []
        rec = _Recorder(p, returned)
        m.device_labelmap = False
        want = m.apply_batch(dict(imgs))
        want_one = {k: m.apply(v) for k, v in imgs.items()}
        assert [c[0] for c in rec.calls] == ['predict_logits_from_preprocessed_data_batch'] + ['predict_logits_from_preprocessed_data'] * 3
        assert all(not c[1] for c in p.engine_calls)
        m.device_labelmap = True
        del rec.calls[:], p.engine_calls[:]
        got = m.apply_batch(dict(imgs))
        assert rec.calls == [('predict_labelmap_from_preprocessed_data_batch', 3, {'out_shapes': [(1, 70, 90), None, (1, 40, 45)]})]
        assert p.engine_calls == [(3, True, True, [(70, 90), None, (40, 45)])]      # ONE call: every case, with its target extent
        planes_many = list(returned)
        del rec.calls[:], p.engine_calls[:], returned[:]
        got_one = {k: m.apply(v) for k, v in imgs.items()}
        assert rec.calls == [('predict_labelmap_from_preprocessed_data', 1, {'out_shape': (1, 70, 90)}), ('predict_labelmap_from_preprocessed_data', 1, {}),
                             ('predict_labelmap_from_preprocessed_data', 1, {'out_shape': (1, 40, 45)})]
        assert p.engine_calls == [(1, True, False, [(70, 90)]), (1, True, False, [None]), (1, True, False, [(40, 45)])]
        planes_one = list(returned)
    finally:
        m.stop()
    for i, (k, img) in enumerate(imgs.items()):
        for plane, seg, ref in ((planes_many[i], got[k], want[k]), (planes_one[i], got_one[k], want_one[k])):
            assert plane.dtype == np.uint8 and plane.shape == (1, 1) + img.array.shape[:2]
            assert seg.array.dtype == np.uint8 and np.array_equal(seg.array, plane[0, 0])      # the device's plane, unchanged
            assert np.array_equal(seg.array, ref.array), k                                     # ... and the host route's bytes
            assert seg.spacing == img.spacing and seg.origin == img.origin and seg.direction == img.direction and seg.meta == ref.meta
        assert len(np.unique(want[k].array)) >= 2


def test_the_labelmap_methods_refuse_what_is_not_theirs():
    p = _LabelmapDouble(network=None)
    p.list_of_parameters = [np.zeros(1, np.float32)]
    p._create_engines()
    stack = np.zeros((2, 3, 10, 12), np.float32)
    one = np.zeros((2, 1, 10, 12), np.float32)
    assert p.predict_labelmap_from_preprocessed_data(stack) is None and p.predict_labelmap_from_preprocessed_data_batch([one, stack]) is None
    assert p.predict_labelmap_from_preprocessed_data(one, out_shape=(2, 20, 6)) is None          # a stack's extent
    assert p.predict_labelmap_from_preprocessed_data_batch([one], out_shapes=[(0, 6)]) is None
    assert p.predict_labelmap_from_preprocessed_data_batch([one, one], out_shapes=[None]) is None
    assert p.predict_labelmap_from_preprocessed_data_batch([]) == []
    p.list_of_parameters = [np.zeros(1, np.float32)] * 2                                          # a fold ensemble without real engines
    assert p.predict_labelmap_from_preprocessed_data(one) is None and p.predict_labelmap_from_preprocessed_data_batch([one]) is None
    assert not p.engine_calls
