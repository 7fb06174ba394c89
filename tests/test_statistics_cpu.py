"""Per-label statistics on the host (totalsegmentator2d_amd/statistics.py): the statement against an independent plain formulation, its
summation tree against a spelled-out per-lane loop and against csrc/stats_tree.h compiled into a stand-alone program, get_annotation_labels with
fetch / counts, Result.statistics / save_statistics / ``ts2d --statistics`` on the host route, and the refusals."""
import json
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.batch_util import synthetic_batch_model          # (tests/surface_util.synthetic_model behind a predictor that also serves batches)
from totalsegmentator2d_amd import image, main, nrrd, statistics as S
from totalsegmentator2d_amd.main import ts2d_run
from totalsegmentator2d_amd.tool import TS2D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
A = os.path.join(GOLDEN, 'assets')
U = 2.0 ** -53


def bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. statement against a plain formulation
def _case(kind, spatial, C, seed):
    """(seg, values, intensities): random labels plus an empty label, a one-pixel label in each corner and a label that covers everything
    (planes), or a map with four one-pixel corner labels and an absent value (label map; one map in three is a single value everywhere)."""
    rng = np.random.default_rng(seed)
    corners = [tuple(0 if not (c >> a) & 1 else s - 1 for a, s in enumerate(spatial)) for c in range(2 ** len(spatial))]
    if kind == 'planes':
        K = 4 + len(corners)
        seg = np.zeros((K,) + spatial, np.uint8)
        seg[0] = rng.integers(0, 2, spatial) * rng.integers(1, 255, spatial)          # any value > 0 counts
        seg[1] = rng.random(spatial) < 0.05
        seg[2] = 1                                                                     # covers everything
        for i, c in enumerate(corners):                                                # seg[3] stays empty
            seg[4 + i][c] = 255
        values = None
    else:
        seg = rng.integers(0, 5, spatial).astype(np.uint8)
        if seed % 3 == 0:
            seg[...] = 3                                                               # one value covers everything
        for i, c in enumerate(corners):
            seg[c] = 10 + i                                                            # (a 1-wide axis: later corners overwrite earlier ones)
        values = [1, 2, 3, 4, 200] + [10 + i for i in range(len(corners))]              # 200 is absent: an empty label
    x = None
    if C:
        x = (rng.normal(size=(C,) + spatial) * rng.choice([1e-3, 1.0, 1e4], size=(C,) + (1,) * len(spatial))).astype(np.float32)
        x[0][tuple(rng.integers(0, s) for s in spatial)] = -0.0
    return seg, values, x


def _plain(mask, xs):
    n = int(np.count_nonzero(mask))
    at = np.argwhere(mask)
    out = {'count': n}
    if n:
        out['bbox_min'], out['bbox_max'], out['index_sum'] = at.min(axis=0), at.max(axis=0), at.sum(axis=0)
    out['terms'] = [[float(v) for v in x[mask]] for x in xs]
    return out


CASES = [(kind, spatial, C, seed) for kind in ('planes', 'labelmap') for spatial in ((7, 70), (1, 1), (3, 5, 67), (3, 66, 1))
         for C in (0, 1, 2) for seed in (0, 1)]


@pytest.mark.parametrize('kind,spatial,C,seed', CASES)
def test_statement_against_the_plain_formulation(kind, spatial, C, seed):
    seg, values, x = _case(kind, spatial, C, 100 * len(spatial) + 10 * C + seed)
    st = S.label_statistics_statement(seg, x, (1.0,) * len(spatial), values)
    K = seg.shape[0] if values is None else len(values)
    assert st['count'].dtype == np.int64 and st['index_sum'].dtype == np.int64 and st['count'].shape == (K,)
    seen_empty = seen_full = seen_one = False
    for k in range(K):
        mask = seg[k] > 0 if values is None else seg == values[k]
        ref = _plain(mask, [] if x is None else list(x))
        n = ref['count']
        assert st['count'][k] == n and bool(st['exists'][k]) == (n > 0) and st['mm'][k] == float(n)
        seen_empty |= n == 0; seen_full |= n == mask.size; seen_one |= n == 1
        if n == 0:
            assert (st['bbox_max'][k] == -1).all() and (st['bbox_min'][k] == spatial).all() and (st['index_sum'][k] == 0).all()
            continue
        assert (st['bbox_min'][k] == ref['bbox_min']).all() and (st['bbox_max'][k] == ref['bbox_max']).all()
        assert (st['index_sum'][k] == ref['index_sum']).all()
        for c in range(C):
            t = ref['terms'][c]
            keys = S.float_keys(np.asarray(t, np.float32))
            assert bits(st['min'][k, c]) == bits(np.asarray(t, np.float32)[np.argmin(keys)]) and bits(st['max'][k, c]) == bits(np.asarray(t, np.float32)[np.argmax(keys)])
            assert st['min'][k, c] == min(t) and st['max'][k, c] == max(t)
            # any summation order stays within (n - 1) u sum|terms| of the exact sum (Higham, Accuracy and Stability, 4.2, first order)
            s, ssq, mean = float(st['sum'][k, c]), float(st['ssq'][k, c]), float(st['mean'][k, c])
            assert abs(s - math.fsum(t)) <= (n - 1) * U * math.fsum(abs(v) for v in t)
            sq = [(v - mean) * (v - mean) for v in t]                       # float64 terms with the statement's own mean
            assert abs(ssq - math.fsum(sq)) <= (n - 1) * U * math.fsum(sq)
            # one more rounding each: the IEEE divide and the IEEE square root of the statement's own sums
            assert bits(mean) == bits(np.float64(s) / np.float64(n)) and bits(st['std'][k, c]) == bits(np.sqrt(np.float64(ssq) / np.float64(n)))
    assert seen_empty and seen_one and (seen_full or kind == 'labelmap')


def test_a_label_map_of_one_value_is_covered():
    seg = np.full((4, 9), 3, np.uint8)
    st = S.label_statistics_statement(seg, None, (2.0, 0.5), [3, 1])
    assert st['count'].tolist() == [36, 0] and st['mm'].tolist() == [36.0, 0.0] and st['bbox_max'][0].tolist() == [3, 8]
    assert st['index_sum'][0].tolist() == [9 * 6, 4 * 36]


# ------------------------------------------------------------------------------------------------ 2. the tree itself
def _halve(v):
    n = 32
    while n >= 1:
        for l in range(n):
            v[l] = v[l] + v[l + n]
        n //= 2
    return v[0]


def _spelled(terms):
    """The tree of the module docstring, lane by lane in Python floats (IEEE doubles)."""
    rows, W = len(terms), len(terms[0])
    partial = []
    for r in range(rows):
        v = [0.0] * 64
        for l in range(64):
            s = 0.0
            for i in range(l, W, 64):
                s = s + terms[r][i]
            v[l] = s
        partial.append(_halve(v))
    v = [0.0] * 64
    for l in range(64):
        s = 0.0
        for r in range(l, rows, 64):
            s = s + partial[r]
        v[l] = s
    return _halve(v)


def _tree_case(rows, W, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((rows, W)) < 0.6
    mask[rng.integers(0, rows), rng.integers(0, W)] = True
    x = (rng.normal(size=(rows, W)) * 10.0 ** rng.integers(-3, 6, (rows, W))).astype(np.float32)
    return mask, x


TREE = [(rows, W) for W in (1, 63, 64, 65, 130) for rows in (1, 64, 65)]


def _spelled_statistics(mask, x):
    x64 = x.astype(np.float64)
    n = int(mask.sum())
    s = _spelled([[float(x64[r, i]) if mask[r, i] else 0.0 for i in range(x.shape[1])] for r in range(x.shape[0])])
    mean = float(np.float64(s) / np.float64(n))
    ssq = _spelled([[(float(x64[r, i]) - mean) * (float(x64[r, i]) - mean) if mask[r, i] else 0.0 for i in range(x.shape[1])] for r in range(x.shape[0])])
    return s, mean, ssq


@pytest.mark.parametrize('rows,W', TREE)
def test_the_vectorised_tree_is_the_spelled_out_tree(rows, W):
    mask, x = _tree_case(rows, W, 1000 * rows + W)
    st = S.label_statistics_statement(mask[None].astype(np.uint8), x[None], (1.0, 1.0))
    s, mean, ssq = _spelled_statistics(mask, x)
    assert bits(st['sum'][0, 0]) == bits(s) and bits(st['mean'][0, 0]) == bits(mean) and bits(st['ssq'][0, 0]) == bits(ssq)
    assert bits(S.tree_sum(np.where(mask, x.astype(np.float64), 0.0))) == bits(s)
    # the row axis is every axis but the last, flattened: the same samples as 3-D give the same bits
    if rows == 64:
        st3 = S.label_statistics_statement(mask.reshape(1, 4, 16, W).astype(np.uint8), x.reshape(1, 4, 16, W), (1.0, 1.0, 1.0))
        assert bits(st3['sum'][0, 0]) == bits(s) and bits(st3['ssq'][0, 0]) == bits(ssq)


def test_a_lone_negative_zero_sums_to_positive_zero_and_is_the_minimum():
    x = np.ones((3, 70), np.float32)
    x[1, 65] = -0.0
    mask = np.zeros((3, 70), np.uint8)
    mask[1, 65] = 1
    st = S.label_statistics_statement(mask[None], x[None], (1.0, 1.0))
    assert bits(st['sum'][0, 0]) == bits(0.0) and bits(st['mean'][0, 0]) == bits(0.0) and bits(st['ssq'][0, 0]) == bits(0.0) and bits(st['std'][0, 0]) == bits(0.0)
    assert np.signbit(st['min'][0, 0]) and np.signbit(st['max'][0, 0]) and st['min'][0, 0] == 0.0
    x[1, 64] = 0.0
    mask[1, 64] = 1                                                     # both zeros under the label: -0.0 < +0.0 on the keys
    st = S.label_statistics_statement(mask[None], x[None], (1.0, 1.0))
    assert np.signbit(st['min'][0, 0]) and not np.signbit(st['max'][0, 0])
    k = S.float_keys(np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32))
    assert (np.diff(k.astype(np.int64)) > 0).all() and np.array_equal(S.float_unkeys(k).view(np.uint32), np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. csrc/stats_tree.h as a stand-alone program
PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
int main(int argc, char** argv) {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int head[4];
    while (std::fread(head, sizeof(int), 4, f) == 4) {                    // kind, value, rows, W
        const int kind = head[0], value = head[1], rows = head[2], W = head[3];
        const size_t n = (size_t)rows * W;
        std::vector<uint8_t> m(n);
        std::vector<float> x(n);
        if (std::fread(m.data(), 1, n, f) != n || std::fread(x.data(), 4, n, f) != n) return 3;
        std::vector<double> partial(rows);
        uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
        int bad = 0;
        long long count = 0;
        for (size_t i = 0; i < n; ++i) count += ts2d::st_masked(m[i], kind, (uint8_t)value) ? 1 : 0;
        const double sum = ts2d::st_tree_label(m.data(), kind, (uint8_t)value, x.data(), rows, W, 0, 0.0, partial.data(), &kmin, &kmax, &bad);
        const double mean = sum / (double)count;
        const double ssq = ts2d::st_tree_label(m.data(), kind, (uint8_t)value, x.data(), rows, W, 1, mean, partial.data(), &kmin, &kmax, &bad);
        unsigned long long bs, bq;
        std::memcpy(&bs, &sum, 8); std::memcpy(&bq, &ssq, 8);
        const float lo = ts2d::rs_unkey<float>(kmin), hi = ts2d::rs_unkey<float>(kmax);
        unsigned bl, bh;
        std::memcpy(&bl, &lo, 4); std::memcpy(&bh, &hi, 4);
        std::printf("%lld %llu %llu %u %u %d\n", count, bs, bq, bl, bh, bad);
    }
    std::fclose(f);
    return 0;
}
'''


@pytest.fixture(scope='module')
def tree_program(tmp_path_factory):
    """csrc/stats_tree.h - the lane sums the kernels call and the tree they form - as plain C++ behind a main of its own, under the address and
    undefined-behaviour sanitizers where the toolchain links them (nothing loaded into Python runs under a sanitizer)."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    d = tmp_path_factory.mktemp('stats_tree')
    src = d / 'tree.cpp'
    src.write_text(f'#include "{os.path.join(CSRC, "stats_tree.h")}"\n' + PROGRAM)
    exe = d / 'tree'
    base = [cxx, '-x', 'c++', '-O1', '-g', '-std=c++17', '-Wno-unknown-pragmas', '-o', str(exe), str(src)]
    if subprocess.call(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    return str(exe)


def test_the_shared_header_forms_the_statements_tree(tree_program, tmp_path):
    cases = []
    for rows, W in TREE:
        mask, x = _tree_case(rows, W, 1000 * rows + W)
        cases.append((0, 0, (mask * 7).astype(np.uint8), x))
        lab = np.where(mask, 9, np.random.default_rng(W).integers(0, 9, mask.shape)).astype(np.uint8)
        cases.append((1, 9, lab, x))
    x = np.ones((3, 70), np.float32); x[1, 65] = -0.0
    m = np.zeros((3, 70), np.uint8); m[1, 65] = 1
    cases.append((0, 0, m, x))
    xb = x.copy(); xb[1, 65] = np.inf
    cases.append((0, 0, m, xb))
    path = tmp_path / 'cases.bin'
    with open(path, 'wb') as f:
        for kind, value, m, x in cases:
            f.write(struct.pack('<4i', kind, value, m.shape[0], m.shape[1])); f.write(m.tobytes()); f.write(x.tobytes())
    lines = subprocess.run([tree_program, str(path)], check=True, capture_output=True, text=True).stdout.split('\n')[:-1]
    assert len(lines) == len(cases)
    for line, (kind, value, m, x) in zip(lines, cases[:-1]):
        got = [int(v) for v in line.split()]
        st = S.label_statistics_statement(m[None], x[None], (1.0, 1.0)) if kind == 0 else S.label_statistics_statement(m, x[None], (1.0, 1.0), [value])
        assert got == [int(st['count'][0]), int(bits(st['sum'][0, 0])), int(bits(st['ssq'][0, 0])), int(st['min'][0].view(np.uint32)[0]),
                       int(st['max'][0].view(np.uint32)[0]), 0]
    assert int(lines[-1].split()[-1]) == 1                              # the infinite sample under the label is reported


# ------------------------------------------------------------------------------------------------ 4. get_annotation_labels
def _annotated(multilabel: bool, dim3: bool):
    rng = np.random.default_rng(5)
    spatial = (4, 1, 5) if dim3 else (4, 5)
    sp = (0.8, 2.0, 1.5) if dim3 else (0.8, 1.5)
    eye = tuple(float(v) for v in np.eye(len(spatial)).reshape(-1))
    if multilabel:
        arr = (rng.random(spatial + (3,)) < 0.4).astype(np.uint8) * 200
        arr[..., 1] = 0
        seg = nrrd.Image(arr, sp, (0.0,) * len(spatial), eye, 3, {}, None)
        image.set_annotation_meta(seg, {1: 'a', 2: 'b', 3: 'c'}, {'a': (255, 0, 0)})
    else:
        arr = rng.integers(0, 3, spatial).astype(np.uint8) * 2          # values 0, 2, 4
        seg = nrrd.Image(arr, sp, (0.0,) * len(spatial), eye, 1, {}, None)
        image.set_annotation_meta(seg, {2: 'two', 4: 'four'}, {'four': '#00FF00'})
    return seg


def test_get_annotation_labels_defaults_are_unchanged_and_counts_follow_the_reference():
    seg = _annotated(True, False)
    assert image.get_annotation_labels(seg) == {'a': {'value': 1, 'color': [1.0, 0.0, 0.0]}, 'b': {'value': 2}, 'c': {'value': 3}}
    seg = _annotated(False, False)
    assert image.get_annotation_labels(seg) == {'two': {'value': 2}, 'four': {'value': 4, 'color': [0.0, 1.0, 0.0]}}
    for multilabel in (True, False):
        for dim3 in (False, True):
            seg = _annotated(multilabel, dim3)
            plain = image.get_annotation_labels(seg)
            mm = float(np.prod(seg.spacing))                             # get_voxel_mm: every axis, the unit axis included
            assert mm == pytest.approx(2.4 if dim3 else 1.2)
            if multilabel:                                              # get_labels_voxels: count_nonzero per component / np.unique counts
                counts = {i + 1: int(np.count_nonzero(seg.array[..., i])) for i in range(seg.components)}
            else:
                counts = {int(v): int(c) for v, c in zip(*np.unique(seg.array, return_counts=True))}
            got = image.get_annotation_labels(seg, fetch=True, counts=True)
            assert list(got) == list(plain)
            for name, info in got.items():
                n = counts.get(info['value'], 0)
                assert info == dict(plain[name], exists=n > 0, count=n, mm=n * mm) and type(info['count']) is int and type(info['mm']) is float
            assert {k for i in image.get_annotation_labels(seg, fetch=True).values() for k in i} <= {'value', 'color', 'exists'}
            assert {k for i in image.get_annotation_labels(seg, counts=True).values() for k in i} <= {'value', 'color', 'count', 'mm'}
    assert image.get_annotation_labels(_annotated(True, True), fetch=True)['b']['exists'] is False


def test_label_statistics_fields_and_geometry():
    seg = _annotated(False, True)
    seg.origin, seg.direction = (10.0, 20.0, 30.0), (0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0)
    x = np.arange(20, dtype=np.float32).reshape(4, 1, 5)
    st = S.label_statistics(seg, {'grey': nrrd.Image(x, seg.spacing, seg.origin, seg.direction, 1, {}, None)})
    assert list(st) == ['two', 'four']
    for name, e in st.items():
        mask = seg.array == e['value']
        at = np.argwhere(mask)
        assert e['count'] == len(at) and e['bbox'] == [at.min(0).tolist(), at.max(0).tolist()]
        ci = at.sum(0) / len(at)
        assert e['centroid_index'] == ci.tolist()
        want = np.asarray(seg.origin) + np.asarray(seg.direction).reshape(3, 3) @ (np.asarray(seg.spacing) * ci[::-1])
        assert e['centroid_physical'] == want.tolist()
        assert e['intensity']['grey']['min'] == x[mask].min() and e['intensity']['grey']['max'] == x[mask].max()
        assert e['intensity']['grey']['mean'] == pytest.approx(x[mask].mean(dtype=np.float64), rel=1e-14)
        assert e['intensity']['grey']['std'] == pytest.approx(x[mask].std(dtype=np.float64), rel=1e-13)
    # an interleaved multi-component image (a file read back) and the plane-major view of the same samples give the same dict
    multi = _annotated(True, True)
    planes = np.ascontiguousarray(np.moveaxis(multi.array, -1, 0))
    view = nrrd.Image(np.moveaxis(planes, 0, -1), multi.spacing, multi.origin, multi.direction, 3, dict(multi.meta), None)
    assert not view.array.flags['C_CONTIGUOUS'] and S.label_statistics(view, {'grey': x}) == S.label_statistics(multi, {'grey': x})
    empty = S.label_statistics(multi, {'grey': x})['b']
    assert empty == {'value': 2, 'exists': False, 'count': 0, 'mm': 0.0, 'bbox': None, 'centroid_index': None, 'centroid_physical': None,
                     'intensity': {'grey': {'min': None, 'max': None, 'mean': None, 'std': None}}}


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_shape_mismatch_raises_and_a_non_finite_intensity_does_not():
    seg = _annotated(True, False)
    with pytest.raises(ValueError, match='shape'):
        S.label_statistics(seg, {'grey': np.zeros((4, 6), np.float32)})
    with pytest.raises(ValueError, match='shape'):
        S.label_statistics_statement(np.zeros((2, 4, 5), np.uint8), np.zeros((1, 5, 4), np.float32), (1.0, 1.0))
    x = np.ones((4, 5), np.float32)
    at = tuple(np.argwhere(seg.array[..., 0] > 0)[0])
    x[at] = np.nan
    with np.errstate(all='ignore'):
        e = S.label_statistics(seg, {'grey': x})['a']['intensity']['grey']
    assert math.isnan(e['mean']) and math.isnan(e['std'])
    x[at] = np.inf
    with np.errstate(all='ignore'):
        e = S.label_statistics(seg, {'grey': x})['a']['intensity']['grey']
    assert e['mean'] == math.inf and e['max'] == math.inf and math.isnan(e['std'])
    x[at] = 1.0
    x[tuple(np.argwhere(seg.array[..., 0] == 0)[0])] = np.nan            # outside the label: of no consequence
    e = S.label_statistics(seg, {'grey': x})['a']['intensity']['grey']
    assert e == {'min': 1.0, 'max': 1.0, 'mean': 1.0, 'std': 0.0}


# ------------------------------------------------------------------------------------------------ 6. Result.statistics, save_statistics, the CLI
@pytest.fixture(scope='module')
def two_models():
    m1, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_cardiac', 3, 31, mirror=False, feats=(32, 32))
    m2, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_ribs', 4, 32, mirror=False, feats=(32, 32))
    return {'ts2d-v2-ep4000b2_cardiac': m1, 'ts2d-v2-ep4000b2_ribs': m2}


def test_result_statistics_and_save_statistics_on_the_host_route(tmp_path, two_models):
    with TS2D(models=dict(two_models)) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device is None
        seg = res.get_segmentation()
        before = seg.array.tobytes()
        st = res.statistics()
        assert list(st) == list(image.get_annotation_labels(seg)) and len(st) == 7
        pr = res.get_projection()
        assert all(sorted(e['intensity']) == ['max', 'mean'] for e in st.values())
        for i, (name, e) in enumerate(st.items()):
            mask = seg.array[..., i] > 0
            assert e['count'] == int(mask.sum()) and e['mm'] == e['count'] * float(np.prod(seg.spacing))
            if e['count']:
                assert e['intensity']['max']['max'] == float(pr['max'].array[mask].max())
                assert e['intensity']['mean']['mean'] == pytest.approx(float(pr['mean'].array[mask].mean(dtype=np.float64)), rel=1e-12)
        assert seg.array.tobytes() == before
        assert res.statistics(channels='max') == {n: dict(e, intensity={'max': e['intensity']['max']}) for n, e in st.items()}
        part = res.statistics('ts2d-v2-ep4000b2_ribs')
        assert list(part) == [f'ribs_{i}' for i in range(1, 5)] and all(part[n] == dict(st[n], value=part[n]['value']) for n in part)
        with pytest.raises(ValueError, match='no projection'):
            res.statistics(channels=['median'])
        files = res.save_statistics(str(tmp_path), 'case')
        assert [os.path.basename(f) for f in files] == ['case.statistics.json']
        files = res.save_statistics(str(tmp_path), 'case', models='all')
        assert [os.path.basename(f) for f in files] == ['case.statistics.json', 'case-cardiac.statistics.json', 'case-ribs.statistics.json']
        assert [os.path.basename(f) for f in res.save_statistics(str(tmp_path), 'case', models='all', naming='model')][1:] == \
            ['case-ts2d-v2-ep4000b2_cardiac.statistics.json', 'case-ts2d-v2-ep4000b2_ribs.statistics.json']
        with open(tmp_path / 'case.statistics.json') as f:
            text = f.read()
        assert json.loads(text) == st and json.loads(text)['cardiac_1']['count'] == st['cardiac_1']['count']
        with open(tmp_path / 'case-ribs.statistics.json') as f:
            assert json.load(f) == part
        # a collapsed (2-D) segmentation meets projections that kept their unit axis
        flat = ts.predict(os.path.join(A, 'sample_s0521.nrrd'), collapse=True)
        got = flat.statistics()
        assert {n: (e['count'], e['intensity']) for n, e in got.items()} == {n: (e['count'], e['intensity']) for n, e in st.items()}
        assert all(len(e['bbox'][0]) == 2 for e in got.values() if e['exists'])


def test_cli_statistics_files_and_batches(tmp_path, two_models, monkeypatch):
    src = tmp_path / 'in'
    os.makedirs(src)
    shutil.copy(os.path.join(A, 'sample_s0521.nrrd'), src / 'one.nrrd')
    shutil.copy(os.path.join(A, 'sample_s0521.nrrd'), src / 'two.nrrd')
    ts2d_run(str(src), str(tmp_path / 'a'), models=dict(two_models), visualize=False, save_all=True, silent=True, statistics=True)
    ts2d_run(str(src), str(tmp_path / 'b'), models=dict(two_models), visualize=False, save_all=True, silent=True, statistics=True, batch_cases=2)
    ts2d_run(str(src), str(tmp_path / 'c'), models=dict(two_models), visualize=False, silent=True, statistics=True)
    ts2d_run(str(src), str(tmp_path / 'd'), models=dict(two_models), visualize=False, silent=True)
    stats = [f'{c}{m}.statistics.json' for c in ('one', 'two') for m in ('', '-cardiac', '-ribs')]
    assert sorted(f for f in os.listdir(tmp_path / 'a') if 'statistics' in f) == sorted(stats)
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(os.listdir(tmp_path / 'b'))
    for f in stats:
        assert (tmp_path / 'a' / f).read_bytes() == (tmp_path / 'b' / f).read_bytes()
    assert sorted(f for f in os.listdir(tmp_path / 'c') if 'statistics' in f) == ['one.statistics.json', 'two.statistics.json']
    assert (tmp_path / 'c' / 'one.statistics.json').read_bytes() == (tmp_path / 'a' / 'one.statistics.json').read_bytes()
    assert sorted(os.listdir(tmp_path / 'd')) == sorted(f for f in os.listdir(tmp_path / 'c') if 'statistics' not in f)      # without the flag: as before
    seen = {}
    monkeypatch.setattr(main, 'ts2d_run', lambda **kw: seen.update(kw))
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--statistics'])
    assert seen['statistics'] is True
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e')])
    assert seen['statistics'] is False


def test_the_symbol_is_optional_and_the_abi_version_stays():
    from totalsegmentator2d_amd import _lib
    with open(os.path.join(ROOT, 'include', 'ts2d_engine.h')) as f:
        hdr = f.read()
    assert 'ts2d_label_statistics' in _lib.SIGNATURES and 'ts2d_label_statistics' in _lib.OPTIONAL and _lib.ABI_VERSION == 9
    for name, value in (('PLANES', _lib.STATS_PLANES), ('LABELMAP', _lib.STATS_LABELMAP), ('NONFINITE', _lib.STATS_NONFINITE), ('INTS', _lib.STATS_INTS),
                        ('F64S', _lib.STATS_F64S), ('MAX_CHANNELS', _lib.STATS_MAX_CHANNELS)):
        assert f'#define TS2D_STATS_{name} {value}\n' in hdr
    lib = _lib.load()
    assert hasattr(lib, 'ts2d_label_statistics') and lib.ts2d_abi_version() == 9
