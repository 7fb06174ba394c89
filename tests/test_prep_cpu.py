"""Crop box and z-score of a native 2-D input on the device (csrc/kernels_prep.h) as far as it goes without a GPU: the numpy statement of the
arithmetic (preprocess.zscore_f32_statement, crop_box_statement) pinned to numpy bit for bit, the C-ABI of the ts2d_planes_* entries
(header, exports, binding, validation before any device work), the emitted instruction stream of the sum kernel (no fused multiply-add,
no scratch, no spills) and the routing of ``DefaultPreprocessor.run_case_npy`` with a stand-in for the handle."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests.conftest import ROOT
from totalsegmentator2d_amd import _lib
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.model import HIPModel

HIPCC = '/opt/rocm/bin/hipcc'
ENTRIES = ('ts2d_planes_create', 'ts2d_planes_crop_zscore', 'ts2d_planes_resample_cubic', 'ts2d_planes_extent', 'ts2d_planes_download',
           'ts2d_planes_destroy')


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _planes(rng, h, w):
    """N(0,1), integer-valued, constant, all-zero, all negative zero, high-dynamic-range."""
    yield rng.standard_normal((h, w)).astype(np.float32)
    yield rng.integers(-1000, 3000, (h, w)).astype(np.float32)
    yield np.full((h, w), np.float32(rng.standard_normal() * 100), np.float32)
    yield np.zeros((h, w), np.float32)
    yield np.full((h, w), -0.0, np.float32)
    yield (rng.standard_normal((h, w)) * 10.0 ** rng.uniform(-6, 6, (h, w))).astype(np.float32)


# run lengths on both sides of every branch: < 8 sequential, <= 128 one leaf, the first split, one chunk of 8192, several chunks and a tail
SHAPES = [(1, n) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 127, 128, 129, 130, 255, 256, 257, 1021, 4099, 8191, 8192, 8193, 8199, 8200, 16383,
                           16384, 16391, 65537)] + [(3, 5), (7, 11), (13, 127), (129, 131), (90, 77), (600, 512), (769, 1031), (2000, 1500)]


def test_the_statement_is_numpy_bit_for_bit():
    rng = np.random.default_rng(12)
    total = 0
    for h, w in SHAPES:
        for a in _planes(rng, h, w):
            a = a[None]                                       # [1, h, w]: what normalize_channel hands to zscore
            with np.errstate(all='ignore'):
                ref = P.zscore(a)
                mean, std = a.mean(), a.std()
            got = P.zscore_f32_statement(a)
            m, s, div = P.zscore_stats_f32_statement(a)
            assert got.dtype == np.float32 and got.shape == ref.shape
            assert _bits(m) == _bits(mean) and _bits(s) == _bits(std), ((h, w), m, mean, s, std)
            assert _bits(div) == _bits(np.float32(max(std, 1e-8)))
            diff = _bits(got) != _bits(ref)
            assert not diff.any(), ((h, w), int(diff.sum()))
            assert _bits(P.sum_f32_statement(a)) == _bits(a.sum())
            total += a.size
    assert total > 20_000_000


def test_the_statement_on_a_view_of_a_larger_plane_and_above_2_to_the_24():
    rng = np.random.default_rng(13)
    big = (rng.standard_normal((300, 400)) * 50 + 20).astype(np.float32)
    view = big[17:203, 5:391][None]                           # a cropped channel is a strided view: numpy normalises a compact copy of it
    assert np.array_equal(_bits(P.zscore_f32_statement(view)), _bits(P.zscore(view)))
    a = (rng.standard_normal((4100, 4100)) * 3 + 1000).astype(np.float32)[None]          # n > 2^24: the count is no float32
    assert a.size > 1 << 24
    assert np.array_equal(_bits(P.zscore_f32_statement(a)), _bits(P.zscore(a)))


def test_chunk_and_leaf_are_numpys():
    assert np.getbufsize() == P.SUM_CHUNK == 8192 and P.SUM_LEAF == 128
    for n in (1, 7, 8, 128, 129, 8191):
        leaves = P.pairwise_leaves(n)
        assert leaves[0][0] == 0 and sum(l for _, l in leaves) == n and all(o2 == o1 + l1 for (o1, l1), (o2, _) in zip(leaves, leaves[1:]))
        assert max(l for _, l in leaves) <= 128 and len(leaves) < 160
    assert P.pairwise_leaves(8192) == [(i * 128, 128) for i in range(64)]


def test_crop_box_statement_is_crop_to_nonzero():
    rng = np.random.default_rng(14)
    cases = []
    for h, w in ((1, 1), (3, 5), (40, 61), (128, 64)):
        full = rng.standard_normal((2, 1, h, w)).astype(np.float32)
        cases.append(full)
        cases.append(np.zeros((2, 1, h, w), np.float32))                           # all zero: the whole extent
        cases.append(np.full((1, 1, h, w), -0.0, np.float32))
        for r0, r1, c0, c1 in ((0, h, 0, w), (0, 1, 0, w), (h - 1, h, 0, w), (0, h, 0, 1), (0, h, w - 1, w), (h // 2, h // 2 + 1, w // 3, w),
                               (h // 3, h, w // 2, w // 2 + 1)):
            a = np.zeros((3, 1, h, w), np.float32)
            a[rng.integers(0, 3), 0, r0:r1, c0:c1] = 1.0                           # boxes that touch each edge, single rows and columns
            cases.append(a)
        a = np.zeros((2, 1, h, w), np.float32)
        a[0, 0, 0, 0] = np.nan; a[1, 0, h - 1, w - 1] = -1e-30                      # a NaN is not zero; different planes span the box
        cases.append(a)
    for a in cases:
        cropped, bbox = P.crop_to_nonzero(a)
        assert P.crop_box_statement(a) == bbox and all(type(v) is int for b in P.crop_box_statement(a) for v in b), a.shape
    with pytest.raises(ValueError, match='one slice'):
        P.crop_box_statement(np.zeros((1, 2, 4, 4), np.float32))


# ------------------------------------------------------------------------------------------------ C-ABI
def _header():
    return re.sub(r'/\*.*?\*/', '', open(_lib.HEADER_PATH).read(), flags=re.S)


def test_entries_are_declared_exported_and_bound_and_the_abi_is_still_9():
    hdr = _header()
    want = {'ts2d_planes_create': ['int device', 'const float* src', 'int n_planes', 'int h', 'int w', 'ts2d_planes** out'],
            'ts2d_planes_crop_zscore': ['ts2d_planes* p', 'int32_t box[4]', 'float* stats', 'int* nonfinite'],
            'ts2d_planes_resample_cubic': ['ts2d_planes* p', 'int out_h', 'int out_w'],
            'ts2d_planes_extent': ['const ts2d_planes* p', 'int* h', 'int* w'],
            'ts2d_planes_download': ['const ts2d_planes* p', 'float* dst'],
            'ts2d_planes_destroy': ['ts2d_planes* p']}
    assert sorted(want) == sorted(ENTRIES)
    for name, params in want.items():
        m = re.search(rf'int\s+{name}\s*\(([^)]*)\)\s*;', hdr)
        assert m, f'{name} is not declared in include/ts2d_engine.h'
        assert [' '.join(p.split()) for p in m.group(1).split(',')] == params
        assert name in _lib.SYMBOLS
    assert 'typedef struct ts2d_planes ts2d_planes;' in hdr and _lib.ABI_VERSION == 9
    lib = _lib.load()
    assert lib.ts2d_abi_version() == 9
    c = ctypes
    sig = {'ts2d_planes_create': [c.c_int, c.c_void_p, c.c_int, c.c_int, c.c_int, c.POINTER(c.c_void_p)],
           'ts2d_planes_crop_zscore': [c.c_void_p, c.POINTER(c.c_int32 * 4), c.c_void_p, c.POINTER(c.c_int)],
           'ts2d_planes_resample_cubic': [c.c_void_p, c.c_int, c.c_int], 'ts2d_planes_extent': [c.c_void_p, c.POINTER(c.c_int), c.POINTER(c.c_int)],
           'ts2d_planes_download': [c.c_void_p, c.c_void_p], 'ts2d_planes_destroy': [c.c_void_p]}
    for name, argtypes in sig.items():
        assert getattr(lib, name).restype is c.c_int and getattr(lib, name).argtypes == argtypes, name
    assert P.planes_device_entries() is lib


def test_every_entry_cites_the_reference_line_it_replaces():
    raw = open(_lib.HEADER_PATH).read()
    for name in ENTRIES:
        doc = raw[:raw.index(f'int {name}(')]
        doc = doc[doc.rindex('/*'):]
        assert 'prediction_worker.py:194-199' in doc, name


def test_bad_arguments_are_refused_by_name_before_any_device_work():
    """No GPU is needed: every check below runs before the first HIP call."""
    lib = _lib.load()
    src = np.ones((2, 4, 4), np.float32)
    h = ctypes.c_void_p()

    def refused(rc, *words):
        msg = _lib.last_error()
        return rc == -1 and all(w in msg for w in words)
    assert refused(lib.ts2d_planes_create(0, None, 2, 4, 4, ctypes.byref(h)), 'ts2d_planes_create', 'null')
    assert refused(lib.ts2d_planes_create(0, src.ctypes.data, 2, 4, 4, None), 'ts2d_planes_create', 'null')
    assert refused(lib.ts2d_planes_create(0, src.ctypes.data, 0, 4, 4, ctypes.byref(h)), 'ts2d_planes_create', '0 planes')
    assert refused(lib.ts2d_planes_create(0, src.ctypes.data, 70000, 4, 4, ctypes.byref(h)), 'ts2d_planes_create', '70000 planes')
    assert refused(lib.ts2d_planes_create(0, src.ctypes.data, 2, 0, 4, ctypes.byref(h)), 'ts2d_planes_create', 'extents 0 x 4')
    assert refused(lib.ts2d_planes_create(0, src.ctypes.data, 2, 4, 8193, ctypes.byref(h)), 'ts2d_planes_create', 'extents 4 x 8193', '8192')
    assert refused(lib.ts2d_planes_create(0, src.ctypes.data, 5, 8192, 8192, ctypes.byref(h)), 'ts2d_planes_create', '2^28')
    assert h.value is None
    box, bad, stats = (ctypes.c_int32 * 4)(), ctypes.c_int(), np.zeros((2, 2), np.float32)
    assert refused(lib.ts2d_planes_crop_zscore(None, ctypes.byref(box), stats.ctypes.data, ctypes.byref(bad)), 'ts2d_planes_crop_zscore', 'null')
    assert refused(lib.ts2d_planes_resample_cubic(None, 8, 8), 'ts2d_planes_resample_cubic', 'null')
    hh, ww = ctypes.c_int(), ctypes.c_int()
    assert refused(lib.ts2d_planes_extent(None, ctypes.byref(hh), ctypes.byref(ww)), 'ts2d_planes_extent', 'null')
    assert refused(lib.ts2d_planes_download(None, src.ctypes.data), 'ts2d_planes_download', 'null')
    assert lib.ts2d_planes_destroy(None) == 0


# ------------------------------------------------------------------------------------------------ instruction stream
@pytest.fixture(scope='module')
def prep_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc is not installed')
    d = tmp_path_factory.mktemp('prep')
    csrc = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
    tu = d / 'prep.hip'
    tu.write_text(f'#include "{os.path.join(csrc, "kernels_prep.h")}"\n'
                  'template __global__ void ts2d::prep_chunk_sums<0>(const float*, long long, const ts2d::PrepNorm*, const ts2d::PrepLeaf*, int, float*);\n'
                  'template __global__ void ts2d::prep_chunk_sums<1>(const float*, long long, const ts2d::PrepNorm*, const ts2d::PrepLeaf*, int, float*);\n')
    devflags = subprocess.check_output(['make', '-s', '-C', csrc, 'flags'], text=True).split()
    subprocess.check_call([HIPCC, '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S', *devflags, '-o', str(d / 'prep.s'), str(tu)],
                          stderr=subprocess.DEVNULL)
    return open(d / 'prep.s').read()


def _kernel(asm, pattern):
    m = re.search(rf'^(_ZN4ts2d\d*{pattern}\w*):', asm, re.M)
    assert m, f'{pattern} not found in the assembly'
    body = asm[m.end():asm.index('.Lfunc_end', m.end())]
    ops = [ln.split()[0] for ln in body.split('\n') if ln.strip() and not ln.strip().startswith((';', '.'))]
    meta = asm[asm.index('amdhsa.kernels:'):]
    blk = next(b for b in re.split(r'\n  - \.', meta)[1:] if m.group(1) in b)
    return ops, blk


@pytest.mark.parametrize('kernel', ['15prep_chunk_sumsILi0E', '15prep_chunk_sumsILi1E', '16prep_nonzero_box', '14prep_normalise'])
def test_kernels_have_no_scratch_and_no_spills_and_the_sums_no_fused_multiply_add(prep_asm, kernel):
    ops, blk = _kernel(prep_asm, kernel)
    assert not [o for o in ops if o.startswith('scratch_')], f'{kernel} spills registers'
    assert re.search(r'private_segment_fixed_size:\s*0\b', blk) and re.search(r'vgpr_spill_count:\s*0\b', blk) and re.search(r'sgpr_spill_count:\s*0\b', blk)
    if 'chunk_sums' in kernel:
        fused = [o for o in ops if 'f32' in o and ('fma' in o or 'mad' in o or 'mac' in o)]
        assert not fused, f'a float32 product was fused into its sum ({fused[0]}): bit-identity with numpy is gone'
        assert sum(o.startswith('v_add_f32') for o in ops) >= 24                 # 15 + 3 + 3 per full-chunk leaf, and the tail path
        if kernel.endswith('1E'):
            assert sum(o.startswith('v_mul_f32') for o in ops) >= 16 and sum(o.startswith(('v_sub_f32', 'v_subrev_f32')) for o in ops) >= 16
        assert not [o for o in ops if 'atomic' in o and 'f32' in o]


# ------------------------------------------------------------------------------------------------ routing
class _StandInLib:
    """The ts2d_planes_* entries computed by the numpy statement, counting their calls."""
    def __init__(self, nonfinite=False):
        self.calls, self.planes, self.next, self.nonfinite = [], {}, 1, nonfinite

    def ts2d_planes_create(self, device, src, n, h, w, out):
        self.calls.append(('create', device, n, h, w))
        a = np.ctypeslib.as_array(ctypes.cast(src, ctypes.POINTER(ctypes.c_float)), (n, h, w)).copy()
        out._obj.value = self.next
        self.planes[self.next] = {'a': a, 'lo_hi': None}
        self.next += 1
        return 0

    def ts2d_planes_crop_zscore(self, hnd, box, stats, bad):
        self.calls.append(('crop_zscore',))
        st = self.planes[hnd.value]
        (_, _), (r0, r1), (c0, c1) = P.crop_box_statement(st['a'][:, None])
        a = st['a'][:, r0:r1, c0:c1]
        if self.nonfinite or not np.isfinite(a).all():
            bad._obj.value = 1
            return 0
        st['a'] = np.stack([P.zscore_f32_statement(p) for p in a])
        st['lo_hi'] = [(p.min(), p.max()) for p in st['a']]
        for i, v in enumerate((r0, r1, c0, c1)):
            box._obj[i] = v
        bad._obj.value = 0
        return 0

    def ts2d_planes_resample_cubic(self, hnd, oh, ow):
        self.calls.append(('resample', oh, ow))
        st = self.planes[hnd.value]
        assert st['lo_hi'] is not None
        st['a'] = np.stack([P.resize_cubic_f64(p, (oh, ow)) for p in st['a']])
        st['lo_hi'] = None
        return 0

    def ts2d_planes_extent(self, hnd, h, w):
        h._obj.value, w._obj.value = self.planes[hnd.value]['a'].shape[1:]
        return 0

    def ts2d_planes_download(self, hnd, dst):
        self.calls.append(('download',))
        a = self.planes[hnd.value]['a']
        np.ctypeslib.as_array(ctypes.cast(dst, ctypes.POINTER(ctypes.c_float)), a.shape)[...] = a
        return 0

    def ts2d_planes_destroy(self, hnd):
        self.calls.append(('destroy',))
        del self.planes[hnd.value]
        return 0


def _run(data, spacing, props_extra, schemes=None, use_mask=None, tf=(0, 1, 2), plans=None):
    pm = SimpleNamespace(transpose_forward=list(tf), plans=plans or {})
    cm = SimpleNamespace(spacing=[1.5, 1.5] if len(tf) == 3 else [1.5], normalization_schemes=schemes or ['ZScoreNormalization'] * data.shape[0],
                         use_mask_for_norm=use_mask or [False] * data.shape[0])
    props = dict({'spacing': (999.0,) + tuple(spacing)}, **props_extra)
    with np.errstate(all='ignore'):
        out, _, props = P.DefaultPreprocessor(verbose=False).run_case_npy(data.copy(), None, props, pm, cm, {})
    return out, props


def _case(seed, c, h, w, border=(0, 0, 0, 0)):
    rng = np.random.default_rng(seed)
    data = np.zeros((c, 1, h, w), np.float32)
    t, b, l, r = border
    data[:, :, t:h - b, l:w - r] = (rng.standard_normal((c, 1, h - t - b, w - l - r)) * 30 + 7).astype(np.float32)
    return data


def _same(a, b):
    (x, px), (y, py) = a, b
    keys = ('shape_before_cropping', 'bbox_used_for_cropping', 'shape_after_cropping_and_before_resampling')
    return x.dtype == y.dtype == np.float32 and x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) and all(px[k] == py[k] for k in keys) \
        and all(type(px[k]) is type(py[k]) for k in keys) and sorted(px) == sorted(py)


def test_run_case_npy_takes_the_handle_when_asked_and_returns_the_same_bytes_and_properties(monkeypatch):
    stand = _StandInLib()
    monkeypatch.setattr(P, 'planes_device_entries', lambda: stand)
    monkeypatch.setattr(P, 'cubic_device_entry', lambda: None)
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    # on the plan spacing, with zero borders: box, z-score, download
    data = _case(1, 2, 60, 45, border=(3, 0, 5, 2))
    host = _run(data, (1.5, 1.5), {})
    assert stand.calls == []
    dev = _run(data, (1.5, 1.5), {'device_normalize': 3})
    assert stand.calls == [('create', 3, 2, 60, 45), ('crop_zscore',), ('download',), ('destroy',)]
    assert _same(dev, host) and 'device_normalize' not in dev[1] and dev[1]['bbox_used_for_cropping'] == [[0, 1], [3, 60], [5, 43]]
    # off the plan spacing, resample on the device: it happens on the handle, through resample_planes_cubic_device
    del stand.calls[:]
    seen = []
    orig = P.resample_planes_cubic_device
    monkeypatch.setattr(P, 'resample_planes_cubic_device', lambda d, hw, dev: (seen.append((type(d).__name__, d.shape, tuple(hw), dev)), orig(d, hw, dev))[1])
    host = _run(data, (1.0, 0.8), {})
    dev = _run(data, (1.0, 0.8), {'device_normalize': 0, 'device_resample': 0})
    assert stand.calls == [('create', 0, 2, 60, 45), ('crop_zscore',), ('resample', 38, 20), ('download',), ('destroy',)]
    assert seen == [('DevicePlanes', (2, 1, 57, 38), (38, 20), 0)] and _same(dev, host)
    # off the plan spacing, resample on the host: normalised planes come down and scipy resamples them
    del stand.calls[:], seen[:]
    dev = _run(data, (1.0, 0.8), {'device_normalize': 0})
    assert stand.calls == [('create', 0, 2, 60, 45), ('crop_zscore',), ('download',), ('destroy',)] and seen == [] and _same(dev, host)
    # an all-zero image keeps its extent; a one-channel image; a single row
    for d in (np.zeros((2, 1, 20, 30), np.float32), _case(2, 1, 33, 47, border=(0, 4, 0, 0)), _case(3, 3, 9, 200, border=(4, 4, 0, 0))):
        assert _same(_run(d, (1.5, 1.5), {'device_normalize': 0}), _run(d, (1.5, 1.5), {}))
    assert not stand.planes                                                       # every handle was destroyed


def test_every_ineligible_case_keeps_the_host_route_with_no_handle_call(monkeypatch):
    stand = _StandInLib()
    monkeypatch.setattr(P, 'planes_device_entries', lambda: stand)
    monkeypatch.setattr(P, 'cubic_device_entry', lambda: None)
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    data = _case(4, 2, 40, 30, border=(2, 2, 2, 2))
    on = {'device_normalize': 0}
    fip = {'0': {'percentile_00_5': -50.0, 'percentile_99_5': 60.0, 'mean': 5.0, 'std': 20.0}}
    vol = _case(5, 2, 40, 30)[:, 0].reshape(2, 4, 10, 30)
    cases = [('masked scheme', data, (1.5, 1.5), dict(use_mask=[True, False])),
             ('CT scheme', data, (1.5, 1.5), dict(schemes=['CTNormalization', 'ZScoreNormalization'], plans={'foreground_intensity_properties_per_channel': fip})),
             ('no normalisation', data, (1.5, 1.5), dict(schemes=['NoNormalization'] * 2)),
             ('Z > 1', vol, (1.5, 1.5), {}),
             ('transpose', data, (1.5, 1.5), dict(tf=(0, 2, 1)))]
    for name, d, sp, kw in cases:
        assert _same(_run(d, sp, on, **kw), _run(d, sp, {}, **kw)), name
        assert stand.calls == [], name
    # a z-score from the projection is there: that route keeps the case, used or not
    nz = P.zscore(data[0])[0]
    dz = {'shape': (40, 30), 'order': (0, 1), 'box': (2, 37, 2, 27), 'norm': np.stack([nz, nz])}
    assert _same(_run(data, (1.5, 1.5), dict(on, device_zscore=dz)), _run(data, (1.5, 1.5), {'device_zscore': dz})) and stand.calls == []
    # an extent over the limit
    wide = np.ones((1, 1, 1, P.CUBIC_MAX_EXTENT + 1), np.float32); wide[0, 0, 0, ::2] = 3
    assert _same(_run(wide, (1.5, 1.5), on), _run(wide, (1.5, 1.5), {})) and stand.calls == []
    # below the size from which the device route pays
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', data.size + 1)
    assert _same(_run(data, (1.5, 1.5), on), _run(data, (1.5, 1.5), {})) and stand.calls == []
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', data.size)
    assert _same(_run(data, (1.5, 1.5), on), _run(data, (1.5, 1.5), {})) and len(stand.calls) == 4
    del stand.calls[:]
    # a library without the entries
    monkeypatch.setattr(P, 'planes_device_entries', lambda: None)
    assert _same(_run(data, (1.0, 0.8), on), _run(data, (1.0, 0.8), {})) and stand.calls == []


def test_a_nonfinite_answer_falls_back_to_the_host_route_and_destroys_the_handle(monkeypatch):
    stand = _StandInLib()
    monkeypatch.setattr(P, 'planes_device_entries', lambda: stand)
    monkeypatch.setattr(P, 'cubic_device_entry', lambda: None)
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    data = _case(6, 2, 40, 30, border=(0, 3, 0, 0))
    for bad in (np.nan, np.inf):
        d = data.copy(); d[1, 0, 7, 7] = bad
        dev, host = _run(d, (1.5, 1.5), {'device_normalize': 0}), _run(d, (1.5, 1.5), {})
        assert dev[0].shape == host[0].shape and np.array_equal(dev[0], host[0], equal_nan=True) and dev[1] == host[1]
        assert stand.calls == [('create', 0, 2, 40, 30), ('crop_zscore',), ('destroy',)] and not stand.planes
        del stand.calls[:]


def test_device_planes_refuses_what_it_does_not_hold_and_closes_twice(monkeypatch):
    stand = _StandInLib()
    monkeypatch.setattr(P, 'planes_device_entries', lambda: stand)
    with pytest.raises(ValueError, match=r'float32 \[C, 1, H, W\]'):
        P.DevicePlanes(np.zeros((2, 2, 4, 4), np.float32), 0)
    with pytest.raises(ValueError, match='float32'):
        P.DevicePlanes(np.zeros((2, 1, 4, 4), np.float64), 0)
    p = P.DevicePlanes(_case(7, 2, 12, 10, border=(1, 0, 0, 2)), 0)
    assert p.shape == (2, 1, 12, 10) and p.crop_zscore() == [[0, 1], [1, 12], [0, 8]] and p.shape == (2, 1, 11, 8) and p.stats.shape == (2, 2)
    assert p.resample((5, 6)) is p and p.download().shape == (2, 1, 5, 6)
    p.close(); p.close()
    assert stand.calls.count(('destroy',)) == 1 and not stand.planes
    monkeypatch.setattr(P, 'planes_device_entries', lambda: None)
    with pytest.raises(RuntimeError, match='no ts2d_planes'):
        P.DevicePlanes(np.zeros((1, 1, 4, 4), np.float32), 0)


# ------------------------------------------------------------------------------------------------ the switch
def test_the_switch_its_gate_and_the_preprocess_key():
    m = HIPModel.__new__(HIPModel)
    m._discover = lambda: None
    HIPModel.__init__(m, {'param': {}})
    assert m.device_input_normalize is True and m.device_input_resample is True
    assert m._normalize_device() is None                                           # no predictor: no device
    m._predictor = SimpleNamespace(engines=[SimpleNamespace(close=lambda: None)])  # engines of another library: the host route
    assert m._normalize_device() is None and m._resample_device() is None
    p = SimpleNamespace(configuration_manager=SimpleNamespace(spacing=[1.5, 1.5]), plans_manager=SimpleNamespace(), dataset_json={})
    assert HIPModel._preprocess_key(p, {}) != HIPModel._preprocess_key(p, {'device_normalize': 0})
    assert HIPModel._preprocess_key(p, {'device_normalize': 0}) != HIPModel._preprocess_key(p, {'device_resample': 0})
    assert HIPModel._preprocess_key(p, {'device_normalize': 0}) == HIPModel._preprocess_key(p, {'device_normalize': 0})
