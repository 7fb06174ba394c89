"""The boundary distances of volumes on the host (totalsegmentator2d_amd/evaluate.py): the three-pass statement against the brute force over all
border pairs (bit for bit) and against scipy, the hand cases, the profile, the keys of evaluate(volume_distances=True) and what the flag leaves
alone, csrc/surface_dist.h and the planner of csrc/evaluate_plan.cpp compiled into a stand-alone program, and the symbol."""
import json
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from totalsegmentator2d_amd import evaluate as E, image, nrrd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
U = 2.0 ** -53
QS = (0, 5, 50, 95, 97.5, 100)
ANISO = (2.5, 0.8, 1.3)
EXTENTS = [(2, 2, 2), (1, 6, 6), (5, 9, 11), (7, 3, 4)]
EYE3 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
DEFAULT_KEYS = {'value', 'count_pred', 'count_ref', 'count_both', 'dice', 'iou', 'precision', 'recall', 'mm_pred', 'mm_ref', 'surface_dice', 'hausdorff'}
NEW_KEYS = {'hausdorff_percentile', 'asd_pred_to_ref', 'asd_ref_to_pred', 'assd', 'masd'}


def bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


def _brute_d2(border_a, border_b, spacing):
    """d2 of every border voxel of A over ALL border voxels of B, the formula as written: (f(dz) + f(dy)) + f(dx)"""
    pa, pb = np.argwhere(border_a), np.argwhere(border_b)
    if len(pb) == 0:
        return np.full(len(pa), np.inf)
    r = [np.abs(pa[:, None, i] - pb[None, :, i]).astype(np.float64) * np.float64(spacing[i]) for i in range(3)]
    return ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]).min(axis=1)


def _three_passes(border_a, border_b, spacing):
    return E.d2_from_planes(border_a, E.plane_distance(E.line_distance(border_b), spacing[0], spacing[1]), spacing[2])


def _ranks(n, q):
    h = np.float64(n - 1) * (np.float64(q) / np.float64(100))
    i = min(int(math.floor(h)), n - 1)
    return i, min(i + 1, n - 1), h - i


# ------------------------------------------------------------------------------------------------ 1. the statement against the brute force
@pytest.mark.parametrize('extent', EXTENTS)
def test_d2_against_the_brute_force_and_scipy(extent):
    rng = np.random.default_rng(3400 + sum(extent))
    differing = 0
    for trial in range(10):                                                  # 4 extents x 10: the 40 random volumes
        spacing = ANISO if trial % 2 == 0 else tuple(float(v) for v in rng.uniform(0.3, 3.0, 3))
        ma, mb = rng.random(extent) < rng.uniform(0.2, 0.8), rng.random(extent) < rng.uniform(0.1, 0.8)
        ba, bb = E.border_of_volume(ma), E.border_of_volume(mb)
        for m, bd in ((ma, ba), (mb, bb)):
            assert np.array_equal(bd, m & ~ndimage.binary_erosion(m))
        for own, other in ((ba, bb), (bb, ba)):
            d2 = _three_passes(own, other, spacing)
            differing += int((bits(d2) != bits(_brute_d2(own, other, spacing))).sum())
            if other.any() and own.any():
                edt = ndimage.distance_transform_edt(~other, sampling=spacing)[own] ** 2
                assert np.all(np.abs(d2 - edt) <= 1e-12 * np.maximum(edt, 1e-300))
        st = E.volume_surface_statement(ma[None].astype(np.uint8), E.PLANES, mb.astype(np.uint8) * 9, E.LABELMAP, [9], spacing, [1.0])
        want = _brute_d2(ba, bb, spacing)
        assert st['border'].tolist() == [[int(ba.sum()), int(bb.sum())]]
        assert bits(st['d2_max'][0, 0]) == bits(want.max() if len(want) else -np.inf) and st['within'][0, 0, 0] == int((want <= 1.0).sum())
    assert differing == 0


def test_plane_distance_is_chunked_over_z():
    rng = np.random.default_rng(3410)
    g = E.line_distance(E.border_of_volume(rng.random((6, 7, 5)) < 0.4))
    whole = E.plane_distance(g, 2.5, 0.8)
    assert E.plane_distance(g, 2.5, 0.8, chunk_bytes=1).tobytes() == whole.tobytes() == E.plane_distance(g, 2.5, 0.8, chunk_bytes=3 * 8 * 7 * 7 * 5).tobytes()


# ------------------------------------------------------------------------------------------------ 2. hand cases
def test_hand_cases():
    sz, sy, sx = ANISO
    # two single voxels, both directions: d2 is the formula
    a, b = np.zeros((1, 4, 5, 6), np.uint8), np.zeros((1, 4, 5, 6), np.uint8)
    a[0, 0, 1, 1], b[0, 3, 3, 5] = 1, 1
    st = E.volume_surface_statement(a, E.PLANES, b, E.PLANES, None, ANISO, [9.0, 10.0])
    d2 = ((np.float64(3) * sz) * (np.float64(3) * sz) + (np.float64(2) * sy) * (np.float64(2) * sy)) + (np.float64(4) * sx) * (np.float64(4) * sx)
    assert st['border'].tolist() == [[1, 1]] and (bits(st['d2_max']) == bits(d2)).all() and st['within'].tolist() == [[[0, 1], [0, 1]]]
    # a solid 3 x 3 x 3 cube: all but the centre
    cube = np.zeros((5, 5, 5), bool)
    cube[1:4, 1:4, 1:4] = True
    assert int(E.border_of_volume(cube).sum()) == 26 and not E.border_of_volume(cube)[2, 2, 2]
    # Z == 1: every foreground voxel is a border voxel - not the 2-D border
    flat = np.zeros((1, 6, 6), bool)
    flat[0, 1:5, 1:5] = True
    assert np.array_equal(E.border_of_volume(flat), flat) and int(E.border_of(flat[0]).sum()) == 12
    st = E.volume_surface_statement(flat[None].astype(np.uint8), E.PLANES, flat[None].astype(np.uint8), E.PLANES, None, ANISO, [0.0])
    assert st['border'].tolist() == [[16, 16]] and st['within'].tolist() == [[[16], [16]]]
    # empty on one side: inf, within 0; empty on both: -inf
    e = np.zeros((3, 4, 5, 6), np.uint8)
    f = np.zeros((3, 4, 5, 6), np.uint8)
    e[0, 1:3, 1:4, 2:5] = 1; f[0, 1:3, 1:4, 2:5] = 1                          # identical
    e[1, 2, 2, 2] = 1                                                        # the other side is empty
    st = E.volume_distance_profile_statement(e, E.PLANES, f, E.PLANES, None, ANISO, [2.0], [50])
    assert st['d2_max'].tolist() == [[0.0, 0.0], [np.inf, -np.inf], [-np.inf, -np.inf]] and st['within'][1:].tolist() == [[[0], [0]], [[0], [0]]]
    assert st['dist_sum'].tolist() == [[0.0, 0.0], [np.inf, 0.0], [0.0, 0.0]] and (st['d2_rank'][1, 0] == np.inf).all() and (st['d2_rank'][2] == -np.inf).all()
    # identical masks: everything 0, NSD 1.0; and None where both are empty
    seg = nrrd.Image(np.ascontiguousarray(np.moveaxis(e, 0, -1)), (1.3, 0.8, 2.5), (0.0,) * 3, EYE3, 3, {}, None)
    image.set_annotation_meta(seg, {1: 'same', 2: 'dot', 3: 'none'})
    ref = nrrd.Image(np.ascontiguousarray(np.moveaxis(f, 0, -1)), (1.3, 0.8, 2.5), (0.0,) * 3, EYE3, 3, {}, None)
    ev = E.evaluate(seg, ref, percentiles=(95,), average_distance=True, volume_distances=True)
    assert ev['same']['surface_dice'] == {'2.0': 1.0} and ev['same']['hausdorff'] == 0.0 and ev['same']['assd'] == 0.0 and ev['same']['hausdorff_percentile'] == {'95.0': 0.0}
    assert ev['dot']['hausdorff'] == math.inf and ev['dot']['surface_dice'] == {'2.0': 0.0} and ev['dot']['asd_ref_to_pred'] is None
    assert ev['none']['hausdorff'] is None and ev['none']['surface_dice'] == {'2.0': None} and ev['none']['assd'] is None
    assert ev['none']['hausdorff_percentile'] == {'95.0': None}
    # the refusals: only [K, Z, H, W] / [Z, H, W]; the 2-D statements keep refusing volumes
    for bad in (np.zeros((1, 5, 6), np.uint8), np.zeros((1, 2, 3, 5, 6), np.uint8)):
        with pytest.raises(ValueError, match='volumes'):
            E.volume_surface_statement(bad, E.PLANES, bad, E.PLANES, None, ANISO, [2.0])
    with pytest.raises(ValueError, match='2-D'):
        E.surface_statement(e, E.PLANES, f, E.PLANES, None, (1.0, 1.0), [2.0])
    with pytest.raises(ValueError, match='percentiles'):
        E.volume_distance_profile_statement(e, E.PLANES, f, E.PLANES, None, ANISO, [2.0], [101])
    with pytest.raises(ValueError, match='label map needs'):
        E.volume_surface_statement(e[0], E.LABELMAP, f, E.PLANES, None, ANISO, [2.0])


# ------------------------------------------------------------------------------------------------ 3. the profile
@pytest.mark.parametrize('extent', EXTENTS + [(3, 5, 70)])
def test_the_profile_against_the_brute_force(extent):
    rng = np.random.default_rng(3420 + sum(extent))
    for spacing in (ANISO, (1.0, 1.0, 1.0)):
        ma, mb = rng.random(extent) < 0.5, rng.random(extent) < 0.3
        a, b = ma[None].astype(np.uint8), mb.astype(np.uint8) * 7
        tol = [0.0, 1.0, 3.0]
        st = E.volume_distance_profile_statement(a, E.PLANES, b, E.LABELMAP, [7], spacing, tol, QS)
        old = E.volume_surface_statement(a, E.PLANES, b, E.LABELMAP, [7], spacing, tol)
        for f in old:
            assert st[f].dtype == old[f].dtype and st[f].tobytes() == old[f].tobytes(), f
        ba, bb = E.border_of_volume(ma), E.border_of_volume(mb)
        for d, d2 in enumerate((_brute_d2(ba, bb, spacing), _brute_d2(bb, ba, spacing))):
            n = len(d2)
            assert n == st['border'][0, d] and n > 0
            ordered = np.sort(d2)
            dist = [float(v) for v in np.sqrt(d2)]
            # any summation order stays within (n - 1) u sum|terms| of the exact sum (Higham, Accuracy and Stability, 4.2, first order)
            assert abs(float(st['dist_sum'][0, d]) - math.fsum(dist)) <= (n - 1) * U * math.fsum(dist)
            for p, q in enumerate(QS):
                i, j, t = _ranks(n, q)
                assert bits(st['d2_rank'][0, d, p, 0]) == bits(ordered[i]) and bits(st['d2_rank'][0, d, p, 1]) == bits(ordered[j]), (d, q)
                assert bits(st['rank_weight'][0, d, p]) == bits(t)
                got = E.percentile_of_ranks(st['d2_rank'][0, d, p, 0], st['d2_rank'][0, d, p, 1], st['rank_weight'][0, d, p])
                want = np.percentile(np.sqrt(d2), q)
                assert abs(got - want) <= 1e-12 * max(abs(want), 1e-300), (d, q, got, want)


# ------------------------------------------------------------------------------------------------ 4. evaluate()
def _two_sides(rng, K, spatial):
    la = rng.integers(0, K + 1, spatial).astype(np.uint8)
    lb = np.where(rng.random(spatial) < 0.7, la, rng.integers(0, K + 1, spatial)).astype(np.uint8)
    la[la == K] = 0
    lb[lb == K] = 0
    lb[lb == K - 1] = 0
    values = list(range(1, K + 1))
    pa = np.stack([(la == v) * rng.integers(1, 256, spatial) for v in values]).astype(np.uint8)
    pb = np.stack([(lb == v) for v in values]).astype(np.uint8)
    return {E.PLANES: (pa, pb), E.LABELMAP: (la, lb)}, values


def _pair(multilabel_pred, multilabel_ref, spatial, spacing, seed=31):
    rng = np.random.default_rng(seed)
    nd = len(spatial)
    sides, values = _two_sides(rng, 4, spatial)

    def make(which, multi):
        arr = np.moveaxis(sides[E.PLANES][which], 0, -1) if multi else sides[E.LABELMAP][which]
        return nrrd.Image(np.ascontiguousarray(arr), spacing, (0.0,) * nd, tuple(np.eye(nd).reshape(-1)), 4 if multi else 1, {}, None)
    pred, ref = make(0, multilabel_pred), make(1, multilabel_ref)
    if multilabel_pred:
        image.set_annotation_meta(pred, {i + 1: f'l{i + 1}' for i in range(4)})
    else:
        pred.meta = {k: v for i in range(4) for k, v in ((f'Segment{i}_ID', str(i)), (f'Segment{i}_Name', f'l{i + 1}'),
                                                          (f'Segment{i}_LabelValue', str(i + 1)), (f'Segment{i}_Layer', '0'))}
    return pred, ref, sides


@pytest.mark.parametrize('multilabel_pred,multilabel_ref', [(True, True), (True, False), (False, True), (False, False)])
def test_evaluate_keys_values_and_the_json_round_trip(multilabel_pred, multilabel_ref, tmp_path):
    spatial, spacing = (4, 6, 7), (1.3, 0.8, 2.5)                            # the image's spacing is x, y, z: array axis k has spacing[2 - k]
    pred, ref, sides = _pair(multilabel_pred, multilabel_ref, spatial, spacing)
    today = E.evaluate(pred, ref, tolerances=(1.0, 2.5), percentiles=(95,), average_distance=True)
    assert today == E.evaluate(pred, ref, tolerances=(1.0, 2.5), percentiles=(95,), average_distance=True, volume_distances=False)
    assert all(not (set(e) & (NEW_KEYS | {'surface_dice', 'hausdorff'})) for e in today.values())
    plain = E.evaluate(pred, ref, tolerances=(1.0, 2.5), volume_distances=True)
    assert all(set(e) == DEFAULT_KEYS for e in plain.values())
    ev = E.evaluate(pred, ref, tolerances=(1.0, 2.5), percentiles=(95, 50.0), average_distance=True, volume_distances=True)
    assert all(set(e) == DEFAULT_KEYS | NEW_KEYS for e in ev.values())
    assert all({k: v for k, v in e.items() if k in DEFAULT_KEYS} == plain[n] for n, e in ev.items())
    assert all({k: v for k, v in e.items() if k in today[n]} == {k: v for k, v in today[n].items()} for n, e in plain.items())      # the overlap part: untouched
    assert all(set(e) == DEFAULT_KEYS | {'hausdorff_percentile'} for e in E.evaluate(pred, ref, percentiles=[95], volume_distances=True).values())
    assert all(set(e) == DEFAULT_KEYS | (NEW_KEYS - {'hausdorff_percentile'}) for e in E.evaluate(pred, ref, average_distance=True, volume_distances=True).values())
    # rebuilt from the statement, with the formulas of the 2-D case
    a, b = sides[E.PLANES if multilabel_pred else E.LABELMAP][0], sides[E.PLANES if multilabel_ref else E.LABELMAP][1]
    st = E.volume_distance_profile_statement(a, E.PLANES if multilabel_pred else E.LABELMAP, b, E.PLANES if multilabel_ref else E.LABELMAP, [1, 2, 3, 4],
                                             (2.5, 0.8, 1.3), [1.0, 2.5], [95, 50.0])
    la, lb = sides[E.LABELMAP]
    for k, (name, e) in enumerate(ev.items()):
        ba, bb = E.border_of_volume(la == k + 1), E.border_of_volume(lb == k + 1)
        assert (int(ba.sum()), int(bb.sum())) == tuple(st['border'][k])
        n = int(ba.sum()) + int(bb.sum())
        for i, t in enumerate((1.0, 2.5)):
            assert e['surface_dice'][repr(t)] == (None if n == 0 else float(np.float64(int(st['within'][k, :, i].sum())) / np.float64(n)))
        assert e['hausdorff'] == (None if n == 0 else float(np.sqrt(st['d2_max'][k].max())))
        ab, ba_ = np.sqrt(_brute_d2(ba, bb, (2.5, 0.8, 1.3))), np.sqrt(_brute_d2(bb, ba, (2.5, 0.8, 1.3)))
        assert list(e['hausdorff_percentile']) == ['95.0', '50.0']
        for p, q in enumerate((95, 50.0)):
            got = e['hausdorff_percentile'][repr(float(q))]
            if n == 0:
                assert got is None
            elif not (np.isfinite(ab).all() and np.isfinite(ba_).all()):
                assert got == math.inf
            else:
                want = max(np.percentile(d, q) for d in (ab, ba_) if len(d))
                assert abs(got - want) <= 1e-12 * max(want, 1e-300)
                assert got == float(max(E.percentile_of_ranks(st['d2_rank'][k, d, p, 0], st['d2_rank'][k, d, p, 1], st['rank_weight'][k, d, p]) for d in range(2)))
        for key, dist, cnt in (('asd_pred_to_ref', st['dist_sum'][k, 0], int(ba.sum())), ('asd_ref_to_pred', st['dist_sum'][k, 1], int(bb.sum())),
                               ('assd', st['dist_sum'][k, 0] + st['dist_sum'][k, 1], n)):
            assert e[key] == (None if cnt == 0 else float(np.float64(dist) / np.float64(cnt)))
        both = (e['asd_pred_to_ref'], e['asd_ref_to_pred'])
        assert e['masd'] == (None if None in both else float((np.float64(both[0]) + np.float64(both[1])) / np.float64(2)))
    assert ev['l4']['assd'] is None and ev['l3']['hausdorff'] == math.inf and ev['l1']['assd'] not in (None, math.inf)
    path = E.dump_evaluation(ev, str(tmp_path / 'e.json'))
    with open(path) as f:
        assert json.load(f) == ev


@pytest.mark.parametrize('spatial,spacing', [((12, 17), (0.8, 2.5)), ((12, 1, 17), (0.8, 2.0, 2.5)), ((1, 12, 17), (0.8, 2.0, 2.5)), ((12, 17, 1), (0.8, 2.0, 2.5))])
def test_the_flag_changes_nothing_on_2d_inputs(spatial, spacing):
    pred, ref, _ = _pair(False, True, spatial, spacing)
    for kw in ({}, {'percentiles': (95,), 'average_distance': True}):
        without = E.evaluate(pred, ref, **kw)
        assert E.evaluate(pred, ref, volume_distances=True, **kw) == without
        assert all('surface_dice' in e and 'hausdorff' in e for e in without.values())


# ------------------------------------------------------------------------------------------------ 5. the header and the planner as a stand-alone program
PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace ts2d;

static int walk(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    int head[8];
    while (std::fread(head, sizeof(int), 8, f) == 8) {                    // kind a, kind b, value, Z, H, W, T, P
        const int kind_a = head[0], kind_b = head[1], value = head[2], Z = head[3], H = head[4], W = head[5], T = head[6], P = head[7];
        const size_t n = (size_t)Z * H * W;
        double sp[3];
        std::vector<double> tol(T), q(P), partial((size_t)Z * H), weights(P), h(n);
        std::vector<uint8_t> a(n), b(n), b0(n), b1(n);
        std::vector<uint16_t> g(n);
        std::vector<uint64_t> keys(n), ranks(2 * P);
        std::vector<long long> within(T), within_plain(T);
        if (std::fread(sp, 8, 3, f) != 3 || std::fread(tol.data(), 8, T, f) != (size_t)T || std::fread(q.data(), 8, P, f) != (size_t)P) return 3;
        if (std::fread(a.data(), 1, n, f) != n || std::fread(b.data(), 1, n, f) != n) return 3;
        for (int dir = 0; dir < 2; ++dir) {
            uint64_t key = 0, key_plain = 0;
            double sum = -1.0;
            std::fill(ranks.begin(), ranks.end(), 0);
            std::fill(weights.begin(), weights.end(), 0.0);
            const uint8_t* own = dir == 0 ? a.data() : b.data();
            const uint8_t* other = dir == 0 ? b.data() : a.data();
            const int ko = dir == 0 ? kind_a : kind_b, kt = dir == 0 ? kind_b : kind_a;
            const long long cnt = sd_volume_label_profile(own, ko, other, kt, (uint8_t)value, Z, H, W, sp[0], sp[1], sp[2], tol.data(), T, q.data(), P,
                                                          b0.data(), b1.data(), g.data(), h.data(), keys.data(), partial.data(), &key, within.data(), &sum,
                                                          ranks.data(), weights.data());
            const long long plain = sd_volume_label(own, ko, other, kt, (uint8_t)value, Z, H, W, sp[0], sp[1], sp[2], tol.data(), T, b0.data(), b1.data(),
                                                    g.data(), h.data(), &key_plain, within_plain.data());
            if (plain != cnt || key_plain != key || within_plain != within) return 4;      // the call without the profile: the same
            std::printf("%lld %llu", cnt, (unsigned long long)key);
            for (int t = 0; t < T; ++t) std::printf(" %lld", within[t]);
            std::printf(" %llu", (unsigned long long)sd_key(sum));
            for (int r = 0; r < 2 * P; ++r) std::printf(" %llu", (unsigned long long)ranks[r]);
            for (int p = 0; p < P; ++p) std::printf(" %llu", (unsigned long long)sd_key(weights[p]));
            std::printf("\n");
        }
    }
    std::fclose(f);
    return 0;
}

// plan <P> <want_sum> <budget> <K> then K x 6 box integers: "ok" and per chunk "k0 k1 vox rows", per label its descriptor; or "over k need"
static int plan(int argc, char** argv) {
    const int P = std::atoi(argv[2]), want_sum = std::atoi(argv[3]), K = std::atoi(argv[5]);
    const size_t budget = (size_t)std::strtoull(argv[4], nullptr, 10);
    if (argc != 6 + 6 * K) return 2;
    std::vector<int32_t> box((size_t)K * 6);
    for (size_t i = 0; i < box.size(); ++i) box[i] = std::atoi(argv[6 + i]);
    std::vector<SdvLabel> labels;
    std::vector<SdvChunk> chunks;
    size_t need = 0;
    const int over = sdv_plan(box.data(), K, P, want_sum, budget, &labels, &chunks, &need);
    if (over >= 0) { std::printf("over %d %zu %zu\n", over, need, labels.size()); return 0; }
    std::printf("ok %zu\n", chunks.size());
    for (const SdvChunk& c : chunks) std::printf("%d %d %lld %lld\n", c.k0, c.k1, c.vox, c.rows);
    for (const SdvLabel& l : labels) std::printf("%d %d %d %d %d %d %lld %lld\n", l.z0, l.y0, l.x0, l.bz, l.by, l.bx, l.vox, l.row);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 6 && !std::strcmp(argv[1], "plan")) return plan(argc, argv);
    return argc == 2 ? walk(argv[1]) : 2;
}
'''


@pytest.fixture(scope='module')
def volume_program(tmp_path_factory):
    """csrc/surface_dist.h - the host walk of the volume's three passes, tree, root, ranks and digit selection - and csrc/evaluate_plan.cpp as
    plain C++ behind a main of its own, under the address and undefined-behaviour sanitizers where the toolchain links them (nothing loaded into
    Python runs under one)."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    d = tmp_path_factory.mktemp('surface_volume')
    src = d / 'volume.cpp'
    src.write_text(f'#include "{os.path.join(CSRC, "surface_dist.h")}"\n#include "{os.path.join(CSRC, "evaluate_plan.cpp")}"\n' + PROGRAM)
    exe = d / 'volume'
    base = [cxx, '-x', 'c++', '-O1', '-g', '-std=c++17', '-Wno-unknown-pragmas', '-o', str(exe), str(src)]
    if subprocess.call(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    return str(exe)


def test_the_shared_header_forms_the_statement(volume_program, tmp_path):
    rng = np.random.default_rng(3430)
    cases = []
    for extent in EXTENTS + [(3, 23, 70)]:                                   # the last: more than 64 rows and columns for the tree
        for spacing in ((1.0, 1.0, 1.0), ANISO):
            ma, mb = rng.random(extent) < 0.45, rng.random(extent) < 0.3
            kind_a, kind_b = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            a = np.where(ma, 9, rng.integers(0, 9, extent)).astype(np.uint8) if kind_a else (ma * rng.integers(1, 256, extent)).astype(np.uint8)
            b = np.where(mb, 9, rng.integers(0, 9, extent)).astype(np.uint8) if kind_b else mb.astype(np.uint8)
            cases.append((kind_a, kind_b, a, b, spacing, [0.0, spacing[1], 2.0], list(QS) + [33.3, 99.9]))
    empty = np.zeros((3, 4, 5), np.uint8)
    cases.append((0, 0, empty, empty, (1.0, 1.0, 1.0), [2.0], [95.0]))
    cases.append((0, 0, (np.arange(60).reshape(3, 4, 5) == 27).astype(np.uint8), empty, (1.0, 1.0, 1.0), [2.0], [95.0]))
    path = tmp_path / 'cases.bin'
    with open(path, 'wb') as f:
        for kind_a, kind_b, a, b, spacing, tol, qs in cases:
            f.write(struct.pack('<8i', kind_a, kind_b, 9, *a.shape, len(tol), len(qs)))
            f.write(struct.pack(f'<{3 + len(tol) + len(qs)}d', *spacing, *[np.float64(t) * np.float64(t) for t in tol], *qs))
            f.write(a.tobytes()); f.write(b.tobytes())
    lines = subprocess.run([volume_program, str(path)], check=True, capture_output=True, text=True).stdout.split('\n')[:-1]
    assert len(lines) == 2 * len(cases)
    for i, (kind_a, kind_b, a, b, spacing, tol, qs) in enumerate(cases):
        st = E.volume_distance_profile_statement(a[None] if kind_a == 0 else a, kind_a, b[None] if kind_b == 0 else b, kind_b, [9], spacing, tol, qs)
        for d in range(2):
            got = [int(v) for v in lines[2 * i + d].split()]
            n = int(st['border'][0, d])
            want = [n, int(bits(st['d2_max'][0, d])) if n else 0] + st['within'][0, d].tolist() + [int(bits(st['dist_sum'][0, d]))]
            want += (bits(st['d2_rank'][0, d]).reshape(-1).tolist() + bits(st['rank_weight'][0, d]).tolist()) if n else [0] * (3 * len(qs))
            assert got == want, (i, d)


def _plan(program, P, want_sum, budget, boxes):
    flat = [str(v) for b in boxes for v in b]
    out = subprocess.run([program, 'plan', str(P), str(want_sum), str(budget), str(len(boxes))] + flat, check=True, capture_output=True, text=True).stdout
    rows = [[int(v) for v in line.split()[1:]] if line.split()[0] in ('ok', 'over') else [int(v) for v in line.split()] for line in out.strip().split('\n')]
    return out.split()[0], rows


def test_the_planner(volume_program):
    NONE = (-1, -1, -1, -1, -1, -1)                                          # a label that is empty on both sides, as the box kernel leaves it
    Z, H, W = 4, 6, 7
    full = (0, 0, 0, Z - 1, H - 1, W - 1)
    per = 38 * Z * H * W + 16 * Z * H
    # boxes that fill the volume, under a bound that holds them all: one chunk, the offsets in box voxels and box rows
    word, rows = _plan(volume_program, 2, 1, 3 * per, [full, full, full])
    assert word == 'ok' and rows[0] == [1] and rows[1] == [0, 3, 3 * Z * H * W, 3 * Z * H]
    assert rows[2:] == [[0, 0, 0, Z, H, W, k * Z * H * W, k * Z * H] for k in range(3)]
    # a bound that forces one label per chunk: every label starts at offset 0 of its own chunk
    word, rows = _plan(volume_program, 2, 1, 2 * per - 1, [full, full, full])
    assert word == 'ok' and rows[0] == [3] and rows[1:4] == [[k, k + 1, Z * H * W, Z * H] for k in range(3)]
    assert all(r[6:] == [0, 0] for r in rows[4:])
    # single-voxel boxes and an empty label between them: the empty one joins a chunk and takes nothing
    dot1, dot2 = (1, 2, 3, 1, 2, 3), (3, 5, 6, 3, 5, 6)
    word, rows = _plan(volume_program, 0, 0, 22, [dot1, NONE, dot2, NONE])
    assert word == 'ok' and rows[0] == [2] and rows[1:3] == [[0, 2, 1, 1], [2, 4, 1, 1]]
    assert rows[3:] == [[1, 2, 3, 1, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0, 1, 1], [3, 5, 6, 1, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0, 1, 1]]
    word, rows = _plan(volume_program, 0, 0, 44, [NONE, dot1, NONE, dot2])
    assert word == 'ok' and rows[0] == [1] and rows[1] == [0, 4, 2, 2] and [r[6:] for r in rows[2:]] == [[0, 0], [0, 0], [1, 1], [1, 1]]
    # all empty: one chunk without a voxel
    word, rows = _plan(volume_program, 8, 1, 1, [NONE, NONE])
    assert word == 'ok' and rows[:2] == [[1], [0, 2, 0, 0]]
    # the bytes: 22 per box voxel, 16 more with percentiles, 16 per box row with the sum; a label above the bound is refused, nothing planned
    box = (1, 1, 2, 2, 3, 5)                                                 # 2 x 3 x 4
    for P, want_sum, need in ((0, 0, 22 * 24), (1, 0, 38 * 24), (0, 1, 22 * 24 + 16 * 6), (8, 1, 38 * 24 + 16 * 6)):
        assert _plan(volume_program, P, want_sum, need, [dot1, box])[0] == 'ok'
        word, rows = _plan(volume_program, P, want_sum, need - 1, [dot1, box])
        assert word == 'over' and rows[0] == [1, need, 0]


# ------------------------------------------------------------------------------------------------ 6. the symbol
def test_the_symbol_is_optional_and_the_abi_version_stays():
    import ctypes
    from totalsegmentator2d_amd import _lib, engine
    with open(os.path.join(ROOT, 'include', 'ts2d_engine.h')) as f:
        hdr = f.read()
    assert _lib.ABI_VERSION == 9
    name = 'ts2d_volume_surface_distances'
    assert name in _lib.SIGNATURES and name in _lib.OPTIONAL and name in _lib.SYMBOLS and f'int {name}(' in hdr
    restype, argtypes = _lib.SIGNATURES[name]
    old = _lib.SIGNATURES['ts2d_surface_distance_profile'][1]
    i, d = ctypes.c_int, ctypes.c_double
    assert restype is i and argtypes == old[:7] + [i, i, i, d, d, d] + old[11:]          # Z, H, W and three spacings in the place of H, W and two
    lib = _lib.load()
    assert hasattr(lib, name) and engine.has_entry(name)
    assert engine.volume_scratch_per_label((2, 3, 4), 0, False) == 22 * 24 and engine.volume_scratch_per_label((2, 3, 4), 3, True) == 38 * 24 + 16 * 6
