"""nnU-Net's largest-component postprocessing as far as it goes without a GPU: the numpy/scipy statement
(``postprocess.keep_largest_components_statement``) against a spelled-out flood fill, the find / union / link routines of the device kernels
(csrc/cc_label.h) compiled for the host against scipy's partition, the plan and its JSON reader, and the routing of ``HIPModel`` through the host
doubles of tests/surface_util.py and tests/batch_util.py."""
import ctypes
import json
import os
import shutil
import subprocess
from collections import deque

import numpy as np
import pytest
from scipy import ndimage

from tests import prob_util
from tests.batch_util import HostBatchModel
from tests.conftest import ROOT
from tests.surface_util import HostModel, synthetic_model
from totalsegmentator2d_amd import _lib, export, nrrd, postprocess
from totalsegmentator2d_amd import model as model_module
from totalsegmentator2d_amd.postprocess import PostprocessingPlan, apply_postprocessing, keep_largest_components_statement, load_postprocessing

CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
FULL = np.ones((3, 3, 3), bool)


# ------------------------------------------------------------------------------------------------ volumes
def random_volumes():
    """A few hundred volumes of at most 4 x 9 x 11 with labels 0..3, densities 0.1 ... 0.8, a third of them with Z = 1."""
    rng = np.random.default_rng(25)
    out = []
    for k in range(300):
        z = 1 if k % 3 == 0 else int(rng.integers(2, 5))
        h, w = int(rng.integers(1, 10)), int(rng.integers(1, 12))
        density = (0.1, 0.2, 0.3, 0.5, 0.65, 0.8)[k % 6]
        seg = (rng.random((z, h, w)) < density) * rng.integers(1, 4, (z, h, w))
        out.append(seg.astype(np.uint8))
    return out


def serpentine(Z, H, W):
    """A one-voxel corridor that walks every second column of every second slice up and down; one voxel in the slices between joins them."""
    v = np.zeros((Z, H, W), np.uint8)
    for z in range(0, Z, 2):
        v[z, :, 0::2] = 1
        for x in range(1, W, 2):
            if x + 1 < W:
                v[z, H - 1 if (x // 2) % 2 == 0 else 0, x] = 1
        if z + 1 < Z:
            v[z + 1, 0, 0] = 1
    return v


def bfs_components(mask):
    """The components of a boolean [Z, H, W] under 26-connectivity by a breadth-first flood fill: a list of lists of voxel indices."""
    Z, H, W = mask.shape
    seen = np.zeros(mask.shape, bool)
    nbrs = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
    comps = []
    for start in zip(*np.nonzero(mask)):
        if seen[start]:
            continue
        seen[start] = True
        queue, comp = deque([start]), []
        while queue:
            z, y, x = queue.popleft()
            comp.append((z, y, x))
            for dz, dy, dx in nbrs:
                q = (z + dz, y + dy, x + dx)
                if 0 <= q[0] < Z and 0 <= q[1] < H and 0 <= q[2] < W and mask[q] and not seen[q]:
                    seen[q] = True
                    queue.append(q)
        comps.append(comp)
    return comps


def bfs_statement(seg, plan):
    out = np.array(seg, np.uint8).reshape(((1,) + seg.shape)[-3:]).copy()
    stats = []
    for labels, bg in PostprocessingPlan(plan).steps:
        mask = np.isin(out, labels)
        comps = bfs_components(mask)
        if not comps:
            stats.append((0, 0, 0, 0))
            continue
        largest = max(len(c) for c in comps)
        removed = 0
        for c in comps:
            if len(c) < largest:
                for q in c:
                    out[q] = bg
                removed += len(c)
        stats.append((int(mask.sum()), len(comps), largest, removed))
    return out.reshape(seg.shape), np.array(stats, np.int64)


# ------------------------------------------------------------------------------------------------ 1. the statement
def test_statement_equals_a_spelled_out_flood_fill_on_random_volumes():
    plans = ([([1, 2, 3], 0)], [([1, 2, 3], 0), ([1], 0), ([2], 0), ([3], 0)], [([(1, 2), 3], 7)], [([2], 1), ([1], 0)])
    vols = random_volumes()
    assert len(vols) >= 300 and sum(v.shape[0] == 1 for v in vols) >= 100
    removed = 0
    for k, seg in enumerate(vols):
        plan = plans[k % len(plans)]
        got, stats = keep_largest_components_statement(seg, plan)
        want, want_stats = bfs_statement(seg, plan)
        assert got.dtype == np.uint8 and np.array_equal(got, want), k
        assert stats.dtype == np.int64 and np.array_equal(stats, want_stats), k
        removed += int(stats[:, 3].sum())
    assert removed > 1000                                          # (the plans did something)


def test_fixed_cases_by_name():
    S = keep_largest_components_statement
    # contact by a diagonal only, in the plane (8 neighbours at Z = 1) ...
    a = np.zeros((1, 4, 4), np.uint8)
    a[0, 0, 0] = a[0, 1, 1] = a[0, 2, 2] = 1
    a[0, 0, 3] = 1
    out, st = S(a, [([1], 0)])
    assert out[0, 0, 3] == 0 and out.sum() == 3 and st.tolist() == [[4, 2, 3, 1]]
    # ... and across slices (the corner neighbour of the 26)
    b = np.zeros((3, 3, 3), np.uint8)
    b[0, 0, 0] = b[1, 1, 1] = b[2, 2, 2] = 1
    b[0, 2, 2] = 1                                                 # (it touches (1, 1, 1) by a corner too)
    out, st = S(b, [([1], 0)])
    assert np.array_equal(out, b) and st.tolist() == [[4, 1, 4, 0]]
    b[1, 1, 1] = 0
    out, st = S(b, [([1], 0)])
    assert np.array_equal(out, b) and st.tolist() == [[3, 3, 1, 0]]  # three components of one voxel: a tie, all stay
    # two largest components of equal size both stay, the smaller one goes
    c = np.zeros((1, 5, 9), np.uint8)
    c[0, 0, 0:3] = c[0, 4, 6:9] = 1
    c[0, 2, 4] = 1
    out, st = S(c, [([1], 0)])
    assert out.sum() == 6 and out[0, 2, 4] == 0 and st.tolist() == [[7, 3, 3, 1]]
    # empty mask: nothing changes; all-mask: one component, nothing changes
    out, st = S(c, [([5], 0)])
    assert np.array_equal(out, c) and st.tolist() == [[0, 0, 0, 0]]
    full = np.full((2, 3, 4), 2, np.uint8)
    out, st = S(full, [([2], 0)])
    assert np.array_equal(out, full) and st.tolist() == [[24, 1, 24, 0]]
    # a region: labels 1 and 2 touching are ONE component of the step, a lone 2 elsewhere goes
    d = np.zeros((1, 3, 8), np.uint8)
    d[0, 1, 0:2] = 1
    d[0, 1, 2:4] = 2
    d[0, 1, 6] = 2
    out, st = S(d, [([(1, 2)], 0)])
    assert out[0, 1].tolist() == [1, 1, 2, 2, 0, 0, 0, 0] and st.tolist() == [[5, 2, 4, 1]]
    # ... while label 2 alone has two components of which the pair is the largest; background_label != 0
    out, st = S(d, [([2], 9)])
    assert out[0, 1].tolist() == [1, 1, 2, 2, 0, 0, 9, 0] and st.tolist() == [[3, 2, 2, 1]]
    # two steps: the second sees the first's output (the island of 1 that step one removed is not there to be the largest of label 1)
    e = np.zeros((1, 1, 12), np.uint8)
    e[0, 0, 0:3] = 1
    e[0, 0, 3:5] = 2                                               # 1 1 1 2 2 . 1 1 1 1 . .   foreground: {5 voxels}, {4 voxels}
    e[0, 0, 6:10] = 1
    out, st = S(e, [([1, 2], 0), ([1], 0)])
    assert out[0, 0].tolist() == [1, 1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0] and st.tolist() == [[9, 2, 5, 4], [3, 1, 3, 0]]
    out1, _ = S(e, [([1], 0)])
    assert out1[0, 0].tolist() == [0, 0, 0, 2, 2, 0, 1, 1, 1, 1, 0, 0]
    # label 255, and a 2-D array keeps its shape
    f = np.zeros((4, 6), np.uint8)
    f[0, 0:2] = f[3, 5] = 255
    out, st = S(f, [([255], 0)])
    assert out.shape == (4, 6) and out[3, 5] == 0 and out[0, 0] == 255 and st.tolist() == [[3, 2, 2, 1]]
    assert f[3, 5] == 255                                          # (the input is left alone)
    with pytest.raises(ValueError, match='uint8'):
        S(f.astype(np.int32), [([1], 0)])


# ------------------------------------------------------------------------------------------------ 2. the kernel routines on the host
@pytest.fixture(scope='module')
def host_cc(tmp_path_factory):
    """csrc/cc_label.h compiled as plain C++: the phases of the device kernels, single-threaded, voxel by voxel in index order or in reverse."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    d = tmp_path_factory.mktemp('cc_label')
    src = d / 'cc.cpp'
    src.write_text(f'#include "{os.path.join(CSRC, "cc_label.h")}"\n' + r'''
using namespace ts2d;
// mask [Z][H][W] of 0 / 1 -> parent [Z H W] flattened (-1 outside the mask), bits [Z H][ww]; returns the give-up bit
extern "C" int cc_host(const unsigned char* mask, int Z, int H, int W, int find_cap, int union_cap, int reverse, int* parent, cc_word* bits) {
    const int ww = (W + 63) >> 6;
    const long long rows = (long long)Z * H;
    int gave_up = 0;
    for (long long r = 0; r < rows; ++r)
        for (int w = 0; w < ww; ++w) {
            cc_word m = 0;
            for (int k = 0; k < 64 && w * 64 + k < W; ++k) m |= (cc_word)(mask[r * W + w * 64 + k] != 0) << k;
            bits[r * ww + w] = m;
            for (int k = 0; k < 64 && w * 64 + k < W; ++k)
                parent[r * W + w * 64 + k] = (m >> k & 1) ? (int)(r * W + w * 64 + cc_run_start(m, k)) : -1;
        }
    const long long n = rows * W;
    for (long long t = 0; t < n; ++t) {
        const long long i = reverse ? n - 1 - t : t;
        if (parent[i] < 0) continue;
        const long long r = i / W;
        cc_link_voxel(parent, bits, H, W, ww, (int)(r / H), (int)(r % H), (int)(i % W), find_cap, union_cap, &gave_up);
    }
    for (long long t = 0; t < n; ++t) {
        const long long i = reverse ? n - 1 - t : t;
        if (parent[i] >= 0) parent[i] = cc_find(parent, (int)i, find_cap, &gave_up);
    }
    return gave_up;
}
extern "C" int cc_caps(int which) { return which ? kCcUnionCap : kCcFindCap; }
extern "C" int cc_run(unsigned long long m, int lane, int length) { return length ? cc_run_length(m, lane) : cc_run_start(m, lane); }
''')
    so = d / 'cc.so'
    subprocess.check_call([cxx, '-x', 'c++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.cc_host.restype = ctypes.c_int
    lib.cc_host.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_void_p]
    lib.cc_run.restype, lib.cc_run.argtypes = ctypes.c_int, [ctypes.c_ulonglong, ctypes.c_int, ctypes.c_int]

    def run(mask, reverse=False, find_cap=None, union_cap=None):
        m = np.ascontiguousarray(mask, np.uint8)
        Z, H, W = m.shape
        parent = np.full(m.size, -7, np.int32)
        bits = np.zeros(Z * H * ((W + 63) // 64), np.uint64)
        gave_up = lib.cc_host(m.ctypes.data, Z, H, W, find_cap or lib.cc_caps(0), union_cap or lib.cc_caps(1), int(reverse), parent.ctypes.data,
                              bits.ctypes.data)
        return parent.reshape(m.shape), gave_up
    run.lib = lib
    return run


def assert_partition_is_scipys(parent, mask):
    lab, n = ndimage.label(mask, structure=FULL)
    assert np.array_equal(parent >= 0, mask.astype(bool))
    roots = parent[mask.astype(bool)]
    pairs = np.unique(np.stack([lab[mask.astype(bool)], roots]), axis=1)
    assert pairs.shape[1] == n == len(np.unique(roots))             # one root per scipy label and one label per root
    flat = parent.ravel()
    assert np.array_equal(flat[roots], roots)                       # flattened: every parent is a root ...
    if n:
        assert np.array_equal(np.sort(np.unique(roots)), np.sort(ndimage.minimum(np.arange(mask.size).reshape(mask.shape), lab, np.arange(1, n + 1))))   # ... the minimum index


def test_run_helpers_on_words(host_cc):
    rng = np.random.default_rng(3)
    words = [0xFFFFFFFFFFFFFFFF, 1, 1 << 63, 0x8000000000000001, 0x00FF00FF00FF00FF] + [int(v) for v in rng.integers(0, 2 ** 63, 200, dtype=np.uint64)]
    for m in words:
        for lane in range(64):
            if not m >> lane & 1:
                continue
            start = lane
            while start > 0 and m >> (start - 1) & 1:
                start -= 1
            end = lane
            while end < 63 and m >> (end + 1) & 1:
                end += 1
            assert host_cc.lib.cc_run(m, lane, 0) == start and host_cc.lib.cc_run(m, lane, 1) == end - lane + 1, (hex(m), lane)


def test_host_build_of_the_kernel_routines_gives_scipys_partition(host_cc):
    vols = [v != 0 for v in random_volumes()]
    rng = np.random.default_rng(8)
    vols += [rng.random(s) < p for s in ((1, 7, 130), (2, 5, 65), (3, 4, 64), (2, 3, 129), (1, 1, 200)) for p in (0.3, 0.6, 0.9)]   # runs that cross word ends
    vols += [np.ones((2, 3, 70), bool), np.zeros((2, 3, 5), bool)]
    diag, corner, tie = np.zeros((1, 4, 4), bool), np.zeros((3, 3, 3), bool), np.zeros((1, 5, 9), bool)             # the fixed cases of the statement
    diag[0, 0, 0] = diag[0, 1, 1] = diag[0, 2, 2] = diag[0, 0, 3] = True
    corner[0, 0, 0] = corner[1, 1, 1] = corner[2, 2, 2] = corner[0, 2, 2] = corner[2, 0, 2] = True
    tie[0, 0, 0:3] = tie[0, 4, 6:9] = tie[0, 2, 4] = True
    vols += [diag, corner, tie, np.eye(70, dtype=bool)[None], np.eye(70, dtype=bool)[None, ::-1]]
    for k, mask in enumerate(vols):
        for reverse in (False, True):
            parent, gave_up = host_cc(mask, reverse)
            assert gave_up == 0, k
            assert_partition_is_scipys(parent, mask)


def test_host_build_on_the_serpentine_stays_far_below_the_cap_and_a_tiny_cap_is_reported(host_cc):
    s = serpentine(4, 32, 32).astype(bool)
    assert ndimage.label(s, structure=FULL)[1] == 1 and ndimage.label(s)[1] == 1 and s.sum() > 1000
    for reverse in (False, True):
        parent, gave_up = host_cc(s, reverse)
        assert gave_up == 0
        assert_partition_is_scipys(parent, s)
        # both sides of the cap: the same walk under a cap below what it needs sets the bit (and still ends)
        depth = next(c for c in range(1, 4096) if host_cc(s, reverse, find_cap=c)[1] == 0)
        assert depth * 8 < host_cc.lib.cc_caps(0), depth
        if depth > 1:
            assert host_cc(s, reverse, find_cap=depth - 1)[1] == 1
    assert host_cc(s, True, find_cap=1)[1] == 1                     # (one step cannot even confirm a root's child)


# ------------------------------------------------------------------------------------------------ 3. the plan
def test_plan_validation_and_tables():
    p = PostprocessingPlan([([1, (2, 3), [3, 5]], 0), {'labels_or_regions': [255], 'background_label': 4}, ([7], None), (6, 0)])
    assert p.steps == (((1, 2, 3, 5), 0), ((255,), 4), ((7,), 0), ((6,), 0)) and len(p) == 4
    tables, bgs = p.compiled
    assert tables.dtype == bgs.dtype == np.uint8 and tables.shape == (4, 256) and bgs.tolist() == [0, 4, 0, 0]
    assert np.nonzero(tables[0])[0].tolist() == [1, 2, 3, 5] and np.nonzero(tables[1])[0].tolist() == [255] and tables.max() == 1
    assert PostprocessingPlan(p) == p and load_postprocessing(p) is p and load_postprocessing([([1], 0)]).steps == (((1,), 0),)
    for bad, word in [([], 'non-empty'), (None, 'non-empty'), ([([], 0)], 'non-empty'), ([([256], 0)], '256'), ([([-1], 0)], '-1'), ([([1.5], 0)], 'int'),
                      ([([1], 300)], 'background_label'), ([([()], 0)], 'empty region'), ([([True], 0)], 'int'), ([(1, 2, 3)], 'a step is'),
                      ([(['a'], 0)], 'int')]:
        with pytest.raises(ValueError, match=word):
            PostprocessingPlan(bad)


def _write(path, fns, kwargs):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump({'postprocessing_fns': fns, 'postprocessing_kwargs': kwargs}, f)


def test_json_reader_discovery_and_refusals(tmp_path):
    fn = postprocess.FUNCTION_NAME
    kwargs = [{'labels_or_regions': [1, 2, 3], 'background_label': 0}, {'labels_or_regions': [[1, 2]]}, {'labels_or_regions': 3, 'background_label': 0}]
    want = (((1, 2, 3), 0), ((1, 2), 0), ((3,), 0))
    f = str(tmp_path / 'a' / 'postprocessing.json')
    _write(f, [fn, fn, 'nnunetv2.postprocessing.remove_connected_components.' + fn], kwargs)
    assert load_postprocessing(f).steps == want and load_postprocessing(str(tmp_path / 'a')).steps == want
    # a trained-model folder: directly, else in crossval_results_folds_*
    folder = tmp_path / 'model'
    _write(str(folder / 'crossval_results_folds_0_1_2_3_4' / 'postprocessing.json'), [fn], kwargs[:1])
    assert load_postprocessing(str(folder)).steps == want[:1]
    _write(str(folder / 'postprocessing.json'), [fn], kwargs[1:2])
    assert load_postprocessing(str(folder)).steps == want[1:2]
    with pytest.raises(FileNotFoundError, match='postprocessing.json'):
        load_postprocessing(str(tmp_path))
    # refusals: another function by name, lists of different length, missing keys, no steps; a pickle is never looked for
    _write(f, [fn, 'remove_small_objects'], kwargs[:2])
    with pytest.raises(ValueError, match='remove_small_objects'):
        load_postprocessing(f)
    _write(f, [fn], kwargs[:2])
    with pytest.raises(ValueError, match='one length'):
        load_postprocessing(f)
    _write(f, [], [])
    with pytest.raises(ValueError, match='no steps'):
        load_postprocessing(f)
    with open(f, 'w') as fh:
        json.dump({'fns': []}, fh)
    with pytest.raises(ValueError, match='postprocessing_fns'):
        load_postprocessing(f)
    only_pkl = tmp_path / 'pkl'
    os.makedirs(only_pkl)
    (only_pkl / 'postprocessing.pkl').write_bytes(b'not read')
    with pytest.raises(FileNotFoundError):
        load_postprocessing(str(only_pkl))


# ------------------------------------------------------------------------------------------------ 4. routing
def test_apply_postprocessing_routes(monkeypatch):
    from totalsegmentator2d_amd import engine
    seg = random_volumes()[7]
    plan = [([1, 2, 3], 0), ([2], 0)]
    want, want_stats = keep_largest_components_statement(seg, plan)
    out, stats, route = apply_postprocessing(seg, plan)                                 # no device: the statement
    assert route == 'host' and np.array_equal(out, want) and np.array_equal(stats, want_stats)
    # a library without the symbol keeps the host route: the entry is not called
    assert 'ts2d_keep_largest_components' in _lib.SYMBOLS and 'ts2d_keep_largest_components' in _lib.OPTIONAL
    monkeypatch.setattr(engine, 'has_keep_largest_components', lambda: False)
    monkeypatch.setattr(engine, 'keep_largest_components', lambda *a, **kw: pytest.fail('called an entry the library does not have'))
    out, stats, route = apply_postprocessing(seg, plan, device=0)
    assert route == 'host' and np.array_equal(out, want)
    # a library that has it is called with the compiled plan; what it returns is the result ...
    calls = []

    def entry(s, tables, bgs, device=0):
        calls.append((s.shape, tables.shape, bgs.tolist(), device))
        return want.copy(), want_stats.copy(), 0
    monkeypatch.setattr(postprocess, '_device_entry', lambda: entry)
    out, stats, route = apply_postprocessing(seg, plan, device=3)
    assert route == 'device' and np.array_equal(out, want) and calls == [(seg.shape, (2, 256), [0, 0], 3)]
    # ... unless it gives up: then the statement runs
    monkeypatch.setattr(postprocess, '_device_entry', lambda: (lambda s, t, b, device=0: (None, None, _lib.CC_GIVE_UP)))
    out, stats, route = apply_postprocessing(seg, plan, device=3)
    assert route == 'host' and np.array_equal(out, want) and np.array_equal(stats, want_stats)


def _config(kind, seed=47):
    m0, _, _ = synthetic_model('ts2d-v2-ep4000b2_' + kind, 3, seed, network=True, feats=(32, 32))
    cfg = dict(m0._config)
    cfg['synthetic'] = dict(cfg['synthetic'], dataset_json=dict(prob_util.DATASETS[kind]))
    cfg['param'] = dict(cfg['param'], **{'nnu.result.colors': None})
    return cfg


def _image(seed, hw, spacing, margin):
    a = (np.random.default_rng(seed).standard_normal(hw + (2,)) * 300).astype(np.float32)
    keep = np.zeros(hw, bool)
    keep[margin[0]:hw[0] - margin[0], margin[1]:hw[1] - margin[1]] = True
    a[~keep] = 0
    return nrrd.Image(a, spacing, (3.0, -7.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


SEEDS = {'labelmap': 47, 'regions': 48}        # (chosen on this oracle: the maps hold stray components for the plans to remove)
PLANS = {'labelmap': [([1, 2], 0), ([1], 0), ([2], 0)], 'regions': [([(1, 2, 3)], 0), ([(2, 3)], 1), ([3], 2)]}


@pytest.mark.parametrize('kind', ['labelmap', 'regions'])
def test_models_through_the_host_doubles(kind, monkeypatch):
    imgs = {'on': _image(1, (80, 70), (1.5, 1.5), (5, 7)), 'off': _image(2, (70, 90), (0.9, 1.2), (4, 6))}
    seen = []
    orig = model_module.export_prediction_from_logits
    monkeypatch.setattr(model_module, 'export_prediction_from_logits', lambda *a, **kw: (seen.append(sorted(kw)), orig(*a, **kw))[1])
    results = {}
    for base, batched in ((HostModel, False), (HostBatchModel, True)):
        m = base(_config(kind, SEEDS[kind]))
        assert m.device_postprocessing is True and m.postprocessing is None
        m.start()
        try:
            call = m.apply_batch if batched else m.apply
            del seen[:]
            plain = call(dict(imgs))
            assert seen and all('postprocess' not in kw for kw in seen)                     # no plan: the export is called as it always was
            assert not any(hasattr(im, 'postprocessing') for im in plain.values()) and 'postprocessed' not in m.timestamps
            m.set_postprocessing(PLANS[kind])
            del seen[:]
            post = call(dict(imgs))
            assert seen and all('postprocess' in kw for kw in seen)
            stamps = m.batch_timestamps['off'] if batched else m.timestamps
            assert stamps['predicted'] <= stamps['postprocessed'] <= stamps['exported']
            prob = call(dict(imgs), save_probabilities=True)
            m.set_postprocessing(None)
            prob_plain = call(dict(imgs), save_probabilities=True)
        finally:
            m.stop()
        removed = 0
        for k in imgs:
            want, stats = keep_largest_components_statement(plain[k].array, PLANS[kind])
            assert np.array_equal(post[k].array, want) and post[k].meta == plain[k].meta
            assert post[k].postprocessing['route'] == 'host' and np.array_equal(post[k].postprocessing['stats'], stats)
            removed += int(stats[:, 3].sum())
            # save_probabilities: the same map, and probabilities that do not know of the plan
            assert np.array_equal(prob[k].array, want) and np.array_equal(prob[k].probabilities, prob_plain[k].probabilities)
            assert np.array_equal(prob_plain[k].array, plain[k].array)
        assert removed > 0, 'the plan removed nothing: the case proves nothing'
        results[batched] = post
    assert all(np.array_equal(results[False][k].array, results[True][k].array) for k in imgs)


def test_plan_sources_and_the_multilabel_refusal(tmp_path):
    cfg = _config('labelmap')
    cfg['synthetic'] = dict(cfg['synthetic'], postprocessing=[([1, 2], 0)])
    assert HostModel(cfg).postprocessing.steps == (((1, 2), 0),)
    f = str(tmp_path / 'postprocessing.json')
    _write(f, [postprocess.FUNCTION_NAME], [{'labels_or_regions': [2], 'background_label': 0}])
    cfg = _config('labelmap')
    cfg['param'] = dict(cfg['param'], **{'nnu.postprocessing': f})
    assert HostModel(cfg).postprocessing.steps == (((2,), 0),)
    cfg['param']['nnu.postprocessing'] = True
    with pytest.raises(ValueError, match='synthetic'):
        HostModel(cfg)
    ml = _config('multilabel')
    m = HostModel(ml)
    with pytest.raises(ValueError, match='multilabel'):
        m.set_postprocessing([([1], 0)])
    assert m.postprocessing is None
    ml['synthetic'] = dict(ml['synthetic'], postprocessing=[([1], 0)])
    with pytest.raises(ValueError, match='multilabel'):
        HostModel(ml)
    with pytest.raises(ValueError, match='multilabel'):
        export.export_prediction_from_logits(np.zeros((3, 1, 4, 4), np.uint8), {'shape_before_cropping': (1, 4, 4), 'bbox_used_for_cropping': [(0, 1), (0, 4), (0, 4)]},
                                             None, None, prob_util.DATASETS['multilabel'], None,
                                             ref_image=nrrd.Image(np.zeros((4, 4), np.float32), (1.0, 1.0), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 1, {}, None),
                                             postprocess=lambda s: (s, None, 'host'))
