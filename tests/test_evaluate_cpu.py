"""Scoring on the host (totalsegmentator2d_amd/evaluate.py): the label projection against a direct triple loop, the overlap counts against
per-label numpy, the boundary distances against the brute force over all border pairs (bit for bit) and against scipy, csrc/surface_dist.h
compiled into a stand-alone program, the empty cases, evaluate / dump_evaluation, and Result.evaluate / save_evaluation / ``ts2d --reference`` on
the host route."""
import json
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from tests.conftest import GOLDEN
from tests.batch_util import synthetic_batch_model
from totalsegmentator2d_amd import evaluate as E, image, main, nrrd
from totalsegmentator2d_amd.main import ts2d_run
from totalsegmentator2d_amd.tool import TS2D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
A = os.path.join(GOLDEN, 'assets')
EYE3 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


def volume(arr, components=1):
    nd = arr.ndim - (1 if components > 1 else 0)
    return nrrd.Image(arr, (0.8, 1.5, 2.0)[:nd], (1.0, 2.0, 3.0)[:nd], tuple(np.eye(nd).reshape(-1)), components, {}, None)


# ------------------------------------------------------------------------------------------------ 1. project_labels
def _loop_projection(a, num, npax):
    shape = list(a.shape)
    shape[npax] = 1
    out = np.zeros(shape + [num], np.uint8)
    for i in range(a.shape[0]):
        for j in range(a.shape[1]):
            for k in range(a.shape[2]):
                v = int(a[i, j, k])
                if v > 0:
                    at = [i, j, k]
                    at[npax] = 0
                    out[at[0], at[1], at[2], v - 1] = 1
    return out


@pytest.mark.parametrize('dtype', ['int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64', 'uint64'])
def test_project_labels_against_the_triple_loop_along_every_axis(dtype):
    rng = np.random.default_rng(11)
    a = (rng.integers(0, 4, (5, 7, 9)) * (rng.random((5, 7, 9)) < 0.3)).astype(dtype)
    img = volume(a)
    for axis, npax in (('sagittal', 2), ('coronal', 1), ('axial', 0), (0, 2), (-1, 0)):
        got = E.project_labels(img, 3, axis)
        assert got.components == 3 and got.array.dtype == np.uint8 and got.array.shape == _loop_projection(a, 3, npax).shape
        assert np.array_equal(got.array, _loop_projection(a, 3, npax))
        assert got.origin == img.origin and got.spacing == img.spacing and got.direction == img.direction
        assert got.size[2 - npax] == 1
    plane_major = np.moveaxis(E.project_labels(img, 3).array, -1, 0)          # the layout of a merged TS2D segmentation
    assert plane_major.flags['C_CONTIGUOUS']


def test_project_labels_edge_cases_and_refusals():
    rng = np.random.default_rng(12)
    a = rng.integers(0, 4, (5, 1, 9)).astype(np.int16)                       # a ray of length 1
    assert np.array_equal(E.project_labels(volume(a), 3).array, _loop_projection(a, 3, 1))
    zero = E.project_labels(volume(np.zeros((5, 7, 9), np.uint8)), 3)        # an all-zero volume
    assert zero.array.shape == (5, 1, 9, 3) and not zero.array.any()
    a = rng.integers(0, 256, (4, 6, 8)).astype(np.uint8)
    a[0, 0, 0], a[1, 2, 3] = 255, 1
    got = E.project_labels(volume(a), 255)
    assert got.components == 255 and np.array_equal(got.array, _loop_projection(a, 255, 1))
    one = E.project_labels(volume((a > 128).astype(np.uint8)), 1)            # num = 1: a scalar image
    assert one.components == 1 and np.array_equal(one.array, (a > 128).any(axis=1, keepdims=True))
    multi = rng.integers(0, 200, (4, 6, 8, 3)).astype(np.uint8)              # multi-component: the per-component maximum
    got = E.project_labels(volume(multi, 3), 17)
    assert got.components == 3 and np.array_equal(got.array, multi.max(axis=1, keepdims=True))
    a = np.zeros((3, 4, 5), np.int16)
    a[1, 2, 3] = 4
    with pytest.raises(ValueError, match='outside 0 ... 3'):
        E.project_labels(volume(a), 3)
    a[1, 2, 3] = -1
    with pytest.raises(ValueError, match='outside 0 ... 3'):
        E.project_labels(volume(a), 3)
    with pytest.raises(ValueError, match='integer'):
        E.project_labels(volume(np.zeros((3, 4, 5), np.float32)), 3)
    for num in (0, 256):
        with pytest.raises(ValueError, match='num'):
            E.project_labels(volume(np.zeros((3, 4, 5), np.uint8)), num)


def test_image_project_still_refuses_multiclass():
    img = volume(np.zeros((3, 4, 5), np.int16))
    with pytest.raises(RuntimeError, match='Unsupported filter mode'):
        image.project(img, 'multiclass:3', 'coronal')
    assert image.device_projection_mode('multiclass:3', 4) is None


# ------------------------------------------------------------------------------------------------ 2. overlap
def _two_sides(rng, K, spatial, empty=True):
    """planes and a label map for each side with the values 1 ... K; label K absent on both sides, K - 1 on side b (where K allows)."""
    la = rng.integers(0, K + 1, spatial).astype(np.uint8)
    lb = np.where(rng.random(spatial) < 0.7, la, rng.integers(0, K + 1, spatial)).astype(np.uint8)
    if empty and K > 1:
        la[la == K] = 0
        lb[lb == K] = 0
    if empty and K > 2:
        lb[lb == K - 1] = 0
    values = list(range(1, K + 1))
    pa = np.stack([(la == v) * rng.integers(1, 256, spatial) for v in values]).astype(np.uint8)      # any value > 0 counts
    pb = np.stack([(lb == v) for v in values]).astype(np.uint8)
    return {E.PLANES: (pa, pb), E.LABELMAP: (la, lb)}, values


@pytest.mark.parametrize('kind_a', [E.PLANES, E.LABELMAP])
@pytest.mark.parametrize('kind_b', [E.PLANES, E.LABELMAP])
def test_overlap_statement_against_per_label_numpy(kind_a, kind_b):
    rng = np.random.default_rng(21)
    for spatial in ((1, 1, 1), (7, 65), (3, 33, 13)):
        sides, values = _two_sides(rng, 5, spatial)
        a, b = sides[kind_a][0], sides[kind_b][1]
        got = E.overlap_statement(a, kind_a, b, kind_b, values)
        la, lb = sides[E.LABELMAP]
        for k, v in enumerate(values):
            assert (got['n_a'][k], got['n_b'][k], got['n_both'][k]) == ((la == v).sum(), (lb == v).sum(), ((la == v) & (lb == v)).sum())
        assert all(got[f].dtype == np.int64 for f in got)
    with pytest.raises(ValueError, match='shape'):
        E.overlap_statement(np.zeros((2, 3, 4), np.uint8), E.PLANES, np.zeros((2, 4, 3), np.uint8), E.PLANES)
    with pytest.raises(ValueError, match='values'):
        E.overlap_statement(np.zeros((3, 4), np.uint8), E.LABELMAP, np.zeros((2, 3, 4), np.uint8), E.PLANES)


# ------------------------------------------------------------------------------------------------ 3. border and distances
def _blobs(rng, H, W, n=3):
    """a mask of a few discs and boxes, some of which touch the image edge"""
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(2, min(H, W) // 2 + 1))
        m |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r) if rng.random() < 0.6 else ((abs(yy - cy) <= r) & (abs(xx - cx) <= r // 2 + 1))
    return m


def _brute_d2(border_a, border_b, sy, sx):
    """d2 of every border pixel of A over ALL border pixels of B, the formula as written"""
    ya, xa = np.nonzero(border_a)
    yb, xb = np.nonzero(border_b)
    if len(yb) == 0:
        return np.full(len(ya), np.inf)
    ry = np.abs(ya[:, None] - yb[None, :]).astype(np.float64) * np.float64(sy)
    rx = np.abs(xa[:, None] - xb[None, :]).astype(np.float64) * np.float64(sx)
    return (ry * ry + rx * rx).min(axis=1)


SURFACE_SHAPES = [(1, 1), (1, 70), (37, 1), (16, 16), (37, 70)]


@pytest.mark.parametrize('H,W', SURFACE_SHAPES)
@pytest.mark.parametrize('spacing', [(1.0, 1.0), (2.5, 0.8)])
def test_d2_against_the_brute_force_and_scipy(H, W, spacing):
    rng = np.random.default_rng(1000 * H + W)
    for trial in range(4):
        ma, mb = _blobs(rng, H, W), _blobs(rng, H, W)
        if trial == 3:
            mb = ma.copy()
        ba, bb = E.border_of(ma), E.border_of(mb)
        assert np.array_equal(ba, ma & ~ndimage.binary_erosion(ma)) and np.array_equal(bb, mb & ~ndimage.binary_erosion(mb))
        g = E.row_distance(bb)
        d2 = E.d2_from_rows(ba, g, spacing)
        assert np.array_equal(bits(d2), bits(_brute_d2(ba, bb, *spacing)))
        if bb.any() and ba.any():
            edt = ndimage.distance_transform_edt(~bb, sampling=spacing)[ba] ** 2
            # five roundings are about 6e-16; distinct candidate distances at these sizes differ by more than 1e-6 relative
            assert np.all(np.abs(d2 - edt) <= 1e-12 * np.maximum(edt, 1e-300))
        st = E.surface_statement(ma[None].astype(np.uint8), E.PLANES, mb.astype(np.uint8) * 7, E.LABELMAP, [7], spacing, [0.0, 1.0, 3.0])
        back = _brute_d2(bb, ba, *spacing)
        assert st['border'].tolist() == [[int(ba.sum()), int(bb.sum())]]
        for d, dd in enumerate((d2, back)):
            assert bits(st['d2_max'][0, d]) == bits(dd.max() if len(dd) else -np.inf)
            assert st['within'][0, d].tolist() == [int((dd <= t * t).sum()) for t in (0.0, 1.0, 3.0)]


def test_the_tie_tolerance_counts_as_within():
    a = np.zeros((5, 9), np.uint8); b = np.zeros((5, 9), np.uint8)
    a[2, 3], b[2, 4] = 1, 1                                                  # one pixel each, one column apart
    sx = 0.8
    st = E.surface_statement(a[None], E.PLANES, b[None], E.PLANES, None, (2.5, sx), [sx, np.nextafter(sx, 0.0)])
    assert bits(st['d2_max'][0, 0]) == bits(np.float64(sx) * np.float64(sx)) == bits((np.float64(1) * sx) * (np.float64(1) * sx))
    assert st['within'][0].tolist() == [[1, 0], [1, 0]]
    seg = nrrd.Image(a, (sx, 2.5), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 1, {}, None)
    image.set_annotation_meta(seg, {1: 'dot'})
    ref = nrrd.Image(b, (sx, 2.5), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 1, {}, None)
    e = E.evaluate(seg, ref, tolerances=[sx])['dot']
    assert e['surface_dice'] == {repr(sx): 1.0} and e['hausdorff'] == sx and e['dice'] == 0.0


def test_the_empty_cases():
    a = np.zeros((3, 6, 6), np.uint8)
    a[0, 1:4, 1:4] = 1
    a[1, 2, 2] = 1
    b = np.zeros((3, 6, 6), np.uint8)
    b[0, 2:5, 2:5] = 1
    st = E.surface_statement(a, E.PLANES, b, E.PLANES, None, (1.0, 1.0), [2.0])
    assert st['border'].tolist() == [[8, 8], [1, 0], [0, 0]]
    assert st['d2_max'][1].tolist() == [np.inf, -np.inf] and st['d2_max'][2].tolist() == [-np.inf, -np.inf]
    assert st['within'][1].tolist() == [[0], [0]]
    with pytest.raises(ValueError, match='2-D'):
        E.surface_statement(np.zeros((1, 2, 6, 6), np.uint8), E.PLANES, np.zeros((1, 2, 6, 6), np.uint8), E.PLANES, None, (1.0, 1.0), [2.0])
    seg = nrrd.Image(np.moveaxis(a, 0, -1), (1.0, 1.0), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 3, {}, None)
    image.set_annotation_meta(seg, {1: 'box', 2: 'dot', 3: 'none'})
    ref = nrrd.Image(np.moveaxis(b, 0, -1), (1.0, 1.0), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 3, {}, None)
    ev = E.evaluate(seg, ref)
    assert ev['none'] == {'value': 3, 'count_pred': 0, 'count_ref': 0, 'count_both': 0, 'dice': None, 'iou': None, 'precision': None, 'recall': None,
                          'mm_pred': 0.0, 'mm_ref': 0.0, 'surface_dice': {'2.0': None}, 'hausdorff': None}
    assert ev['dot']['hausdorff'] == math.inf and ev['dot']['surface_dice'] == {'2.0': 0.0} and ev['dot']['recall'] is None
    assert ev['dot']['dice'] == 0.0 and ev['dot']['precision'] == 0.0
    assert ev['box']['dice'] == 2 * 4 / 18 and ev['box']['iou'] == 4 / 14 and ev['box']['hausdorff'] == math.sqrt(2.0)


# ------------------------------------------------------------------------------------------------ 4. evaluate and its dump
def _annotated_pair(multilabel_pred: bool, multilabel_ref: bool, dim3: bool, seed=31):
    rng = np.random.default_rng(seed)
    spatial = (12, 1, 17) if dim3 else (12, 17)
    sp = (0.8, 2.0, 2.5) if dim3 else (0.8, 2.5)
    nd = len(spatial)
    sides, values = _two_sides(rng, 4, spatial)

    def make(which, multi):
        arr = np.moveaxis(sides[E.PLANES][which], 0, -1) if multi else sides[E.LABELMAP][which]
        return nrrd.Image(np.ascontiguousarray(arr), sp, (0.0,) * nd, tuple(np.eye(nd).reshape(-1)), 4 if multi else 1, {}, None)
    pred, ref = make(0, multilabel_pred), make(1, multilabel_ref)
    if multilabel_pred:
        image.set_annotation_meta(pred, {i + 1: f'l{i + 1}' for i in range(4)})
    else:                                                                    # (the keys of a label map name the values present: written by hand)
        pred.meta = {k: v for i in range(4) for k, v in ((f'Segment{i}_ID', str(i)), (f'Segment{i}_Name', f'l{i + 1}'),
                                                          (f'Segment{i}_LabelValue', str(i + 1)), (f'Segment{i}_Layer', '0'))}
    return pred, ref, sides


@pytest.mark.parametrize('multilabel_pred', [True, False])
@pytest.mark.parametrize('multilabel_ref', [True, False])
@pytest.mark.parametrize('dim3', [True, False])
def test_evaluate_and_the_json_round_trip(multilabel_pred, multilabel_ref, dim3, tmp_path):
    pred, ref, sides = _annotated_pair(multilabel_pred, multilabel_ref, dim3)
    ev = E.evaluate(pred, ref, tolerances=(1.0, 2.5))
    la, lb = (x.reshape(12, 17) for x in sides[E.LABELMAP])
    assert list(ev) == ['l1', 'l2', 'l3', 'l4']
    for v, (name, e) in enumerate(ev.items(), 1):
        ma, mb = la == v, lb == v
        na, nb, both = int(ma.sum()), int(mb.sum()), int((ma & mb).sum())
        assert (e['value'], e['count_pred'], e['count_ref'], e['count_both']) == (v, na, nb, both)
        assert e['dice'] == (None if na + nb == 0 else 2 * both / (na + nb)) and e['precision'] == (None if na == 0 else both / na)
        assert e['recall'] == (None if nb == 0 else both / nb) and e['iou'] == (None if na + nb - both == 0 else both / (na + nb - both))
        assert e['mm_pred'] == na * float(np.prod(np.float64(pred.spacing)))
        ba, bb = E.border_of(ma), E.border_of(mb)
        ab, ba_ = _brute_d2(ba, bb, 2.5, 0.8), _brute_d2(bb, ba, 2.5, 0.8)   # array rows are 2.5 mm apart, columns 0.8 mm
        n = int(ba.sum() + bb.sum())
        for t in (1.0, 2.5):
            assert e['surface_dice'][repr(t)] == (None if n == 0 else (int((ab <= t * t).sum()) + int((ba_ <= t * t).sum())) / n)
        assert e['hausdorff'] == (None if n == 0 else float(np.sqrt(max(ab.max(initial=-np.inf), ba_.max(initial=-np.inf)))))
    assert ev['l4']['dice'] is None and ev['l3']['hausdorff'] == math.inf
    path = E.dump_evaluation(ev, str(tmp_path / 'e.json'))
    with open(path) as f:
        assert json.load(f) == ev
    with pytest.raises(ValueError, match='extent'):
        E.evaluate(pred, nrrd.Image(ref.array[:-1], ref.spacing, ref.origin, ref.direction, ref.components, {}, None))


def test_a_volume_gets_overlap_scores_only():
    rng = np.random.default_rng(41)
    sides, values = _two_sides(rng, 3, (4, 5, 6))
    pred = nrrd.Image(sides[E.LABELMAP][0], (1.0, 1.0, 1.0), (0.0,) * 3, EYE3, 1, {}, None)
    pred.meta = {k: v for i in range(3) for k, v in ((f'Segment{i}_ID', str(i)), (f'Segment{i}_Name', f'l{i + 1}'), (f'Segment{i}_LabelValue', str(i + 1)))}
    ref = nrrd.Image(sides[E.LABELMAP][1], (1.0, 1.0, 1.0), (0.0,) * 3, EYE3, 1, {}, None)
    ev = E.evaluate(pred, ref)
    assert all('surface_dice' not in e and 'hausdorff' not in e for e in ev.values()) and ev['l1']['count_both'] > 0


# ------------------------------------------------------------------------------------------------ 5. csrc/surface_dist.h as a stand-alone program
PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
int main(int argc, char** argv) {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int head[6];
    while (std::fread(head, sizeof(int), 6, f) == 6) {                    // kind a, kind b, value, H, W, T
        const int kind_a = head[0], kind_b = head[1], value = head[2], H = head[3], W = head[4], T = head[5];
        const size_t n = (size_t)H * W;
        double sp[2];
        std::vector<double> tol(T);
        std::vector<uint8_t> a(n), b(n), b0(n), b1(n);
        std::vector<uint16_t> g(n);
        std::vector<long long> within(T);
        if (std::fread(sp, 8, 2, f) != 2 || std::fread(tol.data(), 8, T, f) != (size_t)T) return 3;
        if (std::fread(a.data(), 1, n, f) != n || std::fread(b.data(), 1, n, f) != n) return 3;
        for (int dir = 0; dir < 2; ++dir) {
            uint64_t key = 0;
            const long long cnt = dir == 0
                ? ts2d::sd_label(a.data(), kind_a, b.data(), kind_b, (uint8_t)value, H, W, sp[0], sp[1], tol.data(), T, b0.data(), b1.data(), g.data(), &key, within.data())
                : ts2d::sd_label(b.data(), kind_b, a.data(), kind_a, (uint8_t)value, H, W, sp[0], sp[1], tol.data(), T, b0.data(), b1.data(), g.data(), &key, within.data());
            std::printf("%lld %llu", cnt, (unsigned long long)key);
            for (int t = 0; t < T; ++t) std::printf(" %lld", within[t]);
            std::printf("\n");
        }
    }
    std::fclose(f);
    return 0;
}
'''


@pytest.fixture(scope='module')
def distance_program(tmp_path_factory):
    """csrc/surface_dist.h - the border, the candidate and the key the kernels call, and the two passes they form - as plain C++ behind a main of
    its own, under the address and undefined-behaviour sanitizers where the toolchain links them (nothing loaded into Python runs under one)."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    d = tmp_path_factory.mktemp('surface_dist')
    src = d / 'dist.cpp'
    src.write_text(f'#include "{os.path.join(CSRC, "surface_dist.h")}"\n' + PROGRAM)
    exe = d / 'dist'
    base = [cxx, '-x', 'c++', '-O1', '-g', '-std=c++17', '-Wno-unknown-pragmas', '-o', str(exe), str(src)]
    if subprocess.call(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    return str(exe)


def test_the_shared_header_forms_the_statement(distance_program, tmp_path):
    rng = np.random.default_rng(51)
    cases = []
    for H, W in SURFACE_SHAPES + [(9, 130)]:
        for spacing in ((1.0, 1.0), (2.5, 0.8)):
            ma, mb = _blobs(rng, H, W), _blobs(rng, H, W)
            kind_a, kind_b = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            a = np.where(ma, 9, rng.integers(0, 9, ma.shape)).astype(np.uint8) if kind_a else (ma * rng.integers(1, 256, ma.shape)).astype(np.uint8)
            b = np.where(mb, 9, rng.integers(0, 9, mb.shape)).astype(np.uint8) if kind_b else mb.astype(np.uint8)
            cases.append((kind_a, kind_b, a, b, spacing, [0.0, spacing[1], 2.0]))
    empty = np.zeros((4, 5), np.uint8)
    cases.append((0, 0, empty, empty, (1.0, 1.0), [2.0]))
    cases.append((0, 0, (np.arange(20).reshape(4, 5) == 7).astype(np.uint8), empty, (1.0, 1.0), [2.0]))
    path = tmp_path / 'cases.bin'
    with open(path, 'wb') as f:
        for kind_a, kind_b, a, b, spacing, tol in cases:
            f.write(struct.pack('<6i', kind_a, kind_b, 9, a.shape[0], a.shape[1], len(tol)))
            f.write(struct.pack(f'<{2 + len(tol)}d', *spacing, *[np.float64(t) * np.float64(t) for t in tol]))
            f.write(a.tobytes()); f.write(b.tobytes())
    lines = subprocess.run([distance_program, str(path)], check=True, capture_output=True, text=True).stdout.split('\n')[:-1]
    assert len(lines) == 2 * len(cases)
    for i, (kind_a, kind_b, a, b, spacing, tol) in enumerate(cases):
        st = E.surface_statement(a[None] if kind_a == 0 else a, kind_a, b[None] if kind_b == 0 else b, kind_b, [9], spacing, tol)
        for d in range(2):
            got = [int(v) for v in lines[2 * i + d].split()]
            n = int(st['border'][0, d])
            assert got == [n, int(bits(st['d2_max'][0, d])) if n else 0] + st['within'][0, d].tolist(), (i, d)


# ------------------------------------------------------------------------------------------------ 6. the symbols
def test_the_symbols_are_optional_and_the_abi_version_stays():
    from totalsegmentator2d_amd import _lib
    with open(os.path.join(ROOT, 'include', 'ts2d_engine.h')) as f:
        hdr = f.read()
    assert _lib.ABI_VERSION == 9
    for name in ('ts2d_project_labels_coronal', 'ts2d_label_overlap', 'ts2d_surface_distances'):
        assert name in _lib.SIGNATURES and name in _lib.OPTIONAL and f'int {name}(' in hdr
    for name, value in (('LABELS_RANGE', _lib.LABELS_RANGE), ('EVAL_MAX_TOLERANCES', _lib.EVAL_MAX_TOLERANCES), ('EVAL_MAX_EXTENT', _lib.EVAL_MAX_EXTENT)):
        assert f'#define TS2D_{name} {value}\n' in hdr
    assert (E.PLANES, E.LABELMAP, E.MAX_TOLERANCES) == (_lib.STATS_PLANES, _lib.STATS_LABELMAP, _lib.EVAL_MAX_TOLERANCES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ('ts2d_project_labels_coronal', 'ts2d_label_overlap', 'ts2d_surface_distances'))


# ------------------------------------------------------------------------------------------------ 7. Result.evaluate, save_evaluation, the CLI
@pytest.fixture(scope='module')
def two_models():
    m1, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_cardiac', 3, 31, mirror=False, feats=(32, 32))
    m2, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_ribs', 4, 32, mirror=False, feats=(32, 32))
    return {'ts2d-v2-ep4000b2_cardiac': m1, 'ts2d-v2-ep4000b2_ribs': m2}


def _reference_volume(seed=61):
    """a 3-D label volume on the grid of the sample case: labels 0 ... 7 in boxes"""
    case = nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))
    rng = np.random.default_rng(seed)
    lab = np.zeros(case.array.shape, np.int16)
    for v in range(1, 7):                                                   # label 7 stays absent
        lo = [int(rng.integers(0, s // 2)) for s in lab.shape]
        lab[tuple(slice(o, o + int(rng.integers(3, s // 2))) for o, s in zip(lo, lab.shape))] = v
    return nrrd.Image(lab, case.spacing, case.origin, case.direction, 1, {}, case.space)


def test_result_evaluate_and_save_evaluation_on_the_host_route(tmp_path, two_models):
    vol = _reference_volume()
    with TS2D(models=dict(two_models)) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device is None
        seg = res.get_segmentation()
        before = seg.array.tobytes()
        ev = res.evaluate(vol)
        ref2d = E.project_labels(image.reorient_image(vol), 7, 'coronal')
        assert ref2d.array.shape == seg.array.shape and ev == E.evaluate(seg, ref2d)
        assert list(ev) == list(image.get_annotation_labels(seg)) and len(ev) == 7
        for i, e in enumerate(ev.values()):
            assert e['count_ref'] == int(ref2d.array[..., i].sum()) and e['count_pred'] == int((seg.array[..., i] > 0).sum())
            assert e['count_both'] == int(((seg.array[..., i] > 0) & (ref2d.array[..., i] > 0)).sum()) and '2.0' in e['surface_dice']
        assert list(ev.values())[6]['count_ref'] == 0 and any(e['count_both'] > 0 for e in ev.values())
        assert res.evaluate(ref2d) == ev                                     # an already-2-D segmentation
        assert seg.array.tobytes() == before
        assert list(res.evaluate(vol, tolerances=(1.0, 3.0))['cardiac_1']['surface_dice']) == ['1.0', '3.0']
        with pytest.raises(ValueError, match=r'extent .* against extent'):
            res.evaluate(nrrd.Image(ref2d.array[:-1], ref2d.spacing, ref2d.origin, ref2d.direction, 7, {}, None))
        with pytest.raises(ValueError, match='spacing'):
            res.evaluate(nrrd.Image(ref2d.array, (9.0, 9.0, 9.0), ref2d.origin, ref2d.direction, 7, {}, None))
        files = res.save_evaluation(str(tmp_path), 'case', vol)
        assert [os.path.basename(f) for f in files] == ['case.evaluation.json']
        with open(files[0]) as f:
            assert json.load(f) == ev
        flat = ts.predict(os.path.join(A, 'sample_s0521.nrrd'), collapse=True)          # a collapsed result collapses the projected reference
        def but_mm(d):                                                       # (mm is count * prod(spacing): the collapsed image has one axis fewer)
            return {n: {k: v for k, v in e.items() if not k.startswith('mm_')} for n, e in d.items()}
        assert flat.get_segmentation().dimension == 2 and but_mm(flat.evaluate(vol)) == but_mm(ev)


def test_cli_reference_files_and_refusals(tmp_path, two_models, monkeypatch):
    src, refs = tmp_path / 'in', tmp_path / 'refs'
    os.makedirs(src); os.makedirs(refs)
    for name in ('one', 'two'):
        shutil.copy(os.path.join(A, 'sample_s0521.nrrd'), src / f'{name}.nrrd')
    nrrd.write(_reference_volume(61), str(refs / 'one.nrrd'), True)
    with pytest.raises(FileNotFoundError, match='two'):                      # a case without a reference is an error that names it
        ts2d_run(str(src), str(tmp_path / 'x'), models=dict(two_models), visualize=False, silent=True, reference=str(refs))
    assert not os.path.exists(tmp_path / 'x')
    nrrd.write(_reference_volume(62), str(refs / 'two.nrrd'), True)
    ts2d_run(str(src), str(tmp_path / 'a'), models=dict(two_models), visualize=False, silent=True, reference=str(refs))
    ts2d_run(str(src), str(tmp_path / 'b'), models=dict(two_models), visualize=False, silent=True, reference=str(refs), batch_cases=2)
    ts2d_run(str(src / 'one.nrrd'), str(tmp_path / 'c'), models=dict(two_models), visualize=False, silent=True, reference=str(refs / 'one.nrrd'))
    ts2d_run(str(src), str(tmp_path / 'd'), models=dict(two_models), visualize=False, silent=True)
    assert sorted(f for f in os.listdir(tmp_path / 'a') if 'evaluation' in f) == ['one.evaluation.json', 'two.evaluation.json']
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(os.listdir(tmp_path / 'b'))
    assert (tmp_path / 'a' / 'one.evaluation.json').read_bytes() == (tmp_path / 'c' / 'one.evaluation.json').read_bytes()
    assert (tmp_path / 'a' / 'one.evaluation.json').read_bytes() != (tmp_path / 'a' / 'two.evaluation.json').read_bytes()
    assert sorted(os.listdir(tmp_path / 'd')) == sorted(f for f in os.listdir(tmp_path / 'a') if 'evaluation' not in f)      # without the flag: as before
    with pytest.raises(ValueError, match='single input'):
        ts2d_run(str(src), str(tmp_path / 'y'), models=dict(two_models), visualize=False, silent=True, reference=str(refs / 'one.nrrd'))
    seen = {}
    monkeypatch.setattr(main, 'ts2d_run', lambda **kw: seen.update(kw))
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--reference', str(refs)])
    assert seen['reference'] == str(refs)
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e')])
    assert seen['reference'] is None
