"""The label morphology on the MI355X: the entry ts2d_label_morphology (csrc/kernels_morph.h) against the numpy statement
``morphology.label_morphology_statement`` - the output bytes and all four counters, byte for byte, no tolerance anywhere -, its chunks, its
selection and its refusals, and the wrappers against the host route."""
import ctypes
import os

import numpy as np
import pytest

from tests import morphology_util as U
from tests.conftest import GOLDEN
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, engine, image, nrrd
from totalsegmentator2d_amd import morphology as M
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu
A = os.path.join(GOLDEN, 'assets')
EXTENTS = [(1, 1), (1, 70), (70, 1), (5, 63), (5, 64), (5, 65), (9, 130), (67, 200)]
SPACINGS = [(1.0, 1.0), (0.8, 2.5), (2.5, 0.8)]
_wanted = {}


def radii(sp, extent):
    """0, below one spacing, on-circle equality (the 3-4-5 offset in units of the spacing), 2.5 spacings, beyond the image."""
    return [0.0, 0.99 * min(sp), float(np.hypot(3 * sp[0], 4 * sp[1])), 2.5 * max(sp), 2.0 * (extent[0] * sp[0] + extent[1] * sp[1])]


def check(seg, values, op, r, sp, select=None, max_scratch_bytes=0, must_change=False):
    """The entry on `seg`: the statement's bytes (computed once per input); the input is left alone.  Returns the device's pair."""
    seg = np.ascontiguousarray(seg, np.uint8)
    key = (seg.tobytes(), seg.shape, None if values is None else tuple(values), op, float(r), tuple(sp), None if select is None else tuple(select))
    if key not in _wanted:
        _wanted[key] = M.label_morphology_statement(seg, values, op, r, sp, select)
    want = _wanted[key]
    before = seg.copy()
    got = engine.label_morphology(seg, _lib.STATS_PLANES if values is None else _lib.STATS_LABELMAP, values, seg.shape[-2:], sp, M.OPS.index(op), r,
                                  select=select, max_scratch_bytes=max_scratch_bytes, device=0)
    assert np.array_equal(got[1], want[1]), (op, r, sp, got[1].tolist()[:8], want[1].tolist()[:8])
    assert np.array_equal(got[0], want[0]), (op, r, sp, seg.shape, int((got[0] != want[0]).sum()))
    assert U.same(got, want) and np.array_equal(seg, before)
    if must_change:
        assert got[0].tobytes() != seg.tobytes()
    return got


def test_the_entry_is_there():
    assert engine.has_entry('ts2d_label_morphology') and 'ts2d_label_morphology' in _lib.OPTIONAL


@pytest.mark.parametrize('extent', EXTENTS)
def test_speckle_of_both_kinds_every_op_radius_and_spacing(extent):
    rng = np.random.default_rng(sum(extent))
    H, W = extent
    changed = 0
    for j, density in enumerate((0.03, 0.4, 0.9)):
        sp = SPACINGS[j]
        planes = U.speckle_planes(rng, 3, H, W, density)
        values = [200, 3, 77]                                        # not 1 ... K
        lmap = U.speckle_map(rng, values, H, W, density, others=(9,))
        for r in radii(sp, extent):
            for op in M.OPS:
                a = check(planes, None, op, r, sp)
                b = check(lmap, values, op, r, sp)
                changed += int(a[1][:, 2:].sum() + b[1][:, 2:].sum())
                if r == 0.0:
                    assert a[0].tobytes() == planes.tobytes() and b[0].tobytes() == lmap.tobytes()
    assert changed > 0 or extent == (1, 1)


@pytest.mark.parametrize('K, extent', [(1, (9, 130)), (117, (5, 65)), (255, (9, 130))])
def test_many_labels(K, extent):
    rng = np.random.default_rng(K)
    H, W = extent
    planes = U.speckle_planes(rng, K, H, W, 0.1)
    values = [int(v) for v in rng.permutation(np.arange(1, 256))[:K]]
    lmap = U.speckle_map(rng, values, H, W, 0.5)
    if K > 1:
        planes[K // 2] = 0                                           # an absent label
        planes[0] = 255                                              # a full plane
        lmap[lmap == values[K // 2]] = 0
    for op in M.OPS:
        got = check(planes, None, op, 2.0, (0.8, 1.0))
        assert K == 1 or (got[1][K // 2].tolist() == [0, 0, 0, 0] and got[1][0].tolist() == [H * W, H * W, 0, 0])
        check(lmap, values, op, 2.0, (0.8, 1.0), must_change=True)


def test_edges_corners_and_the_carry_across_chunks():
    H, W = 9, 130
    masks = []
    for k in range(4):                                               # a band on each edge, a block in each corner
        band = np.zeros((H, W), np.uint8)
        (band[:3], band[-3:], band[:, :3], band[:, -3:])[k][...] = 5
        corner = np.zeros((H, W), np.uint8)
        corner[(slice(0, 4), slice(-4, None))[k // 2], (slice(0, 4), slice(-4, None))[k % 2]] = 6
        masks += [band, corner]
    ends = np.zeros((H, W), np.uint8)                                # a single pixel at each end of a 130-wide row
    ends[4, 0] = ends[4, W - 1] = 7
    left, right = ends.copy(), ends.copy()
    left[4, W - 1] = 0
    right[4, 0] = 0
    masks += [ends, left, right, np.full((H, W), 1, np.uint8), np.zeros((H, W), np.uint8)]
    planes = np.stack(masks)
    for r in (1.0, 64.0, 64.5, 65.0, 128.0, 129.0, 200.0):           # reaches that end inside a chunk, on its edge, and across two
        for op in M.OPS:
            check(planes, None, op, r, (1.0, 1.0))
    got = check(planes, None, 'dilate', 129.0, (1.0, 1.0))
    k = len(masks) - 4
    assert got[0][k, 4].all() and got[0][k - 1, 4].all() and got[0][k + 1, 4].all()      # 129 pixels away, exactly on the circle: inside
    assert got[0][k, 3, 128] == 1 and not got[0][k, 3, 129] and got[0][k, 4, 0] == 7 and got[0][k + 1, 5, 1] == 1 and not got[0][k + 1, 5, 0]
    got = check(planes, None, 'erode', 1.0, (1.0, 1.0))
    assert got[0][0, :2].all() and not got[0][0, 2:].any()           # the band at the top keeps its edge rows
    for m in (ends, left, right, masks[0], masks[1]):                # ... and as label maps
        for op in M.OPS:
            check(m, [5, 6, 7], op, 64.5, (1.0, 1.0))


def test_label_map_rules_on_the_device():
    seg = np.zeros((12, 70), np.uint8)
    seg[2:6, 10:20] = 4
    seg[2:6, 22:25] = 8                                              # the dilation of 4 crosses 8 ...
    seg[8, 30] = 9                                                   # ... and an unnamed value stands in the way
    seg[7:10, 50:69] = 200
    for values in ([4, 8, 200], [200, 8, 4], [8, 4, 200]):
        for op in M.OPS:
            for r in (1.0, 3.0, 7.5, 30.0):
                got = check(seg, values, op, r, (1.0, 1.0))
                assert ((got[0] == 9) == (seg == 9)).all()
                for select in ([True, False, True], [False, False, False], [False, True, False]):
                    part = check(seg, values, op, r, (1.0, 1.0), select=select)
                    for k, s in enumerate(select):
                        if not s:                                    # untouched, and an obstacle
                            assert ((part[0] == values[k]) == (seg == values[k])).all() and part[1][k, 2:].tolist() == [0, 0]
    grown = check(seg, [4, 8, 200], 'dilate', 7.5, (1.0, 1.0))[0]
    assert (grown[2:6, 20:22] == 4).all() and (grown[2:6, 22:25] == 8).all() and (grown[2:6, 25:27] == 4).all()      # across 8, which stays
    assert (grown[2:6, 27] == 8).all()                                                                               # beyond the reach of 4
    assert (check(seg, [8, 4, 200], 'dilate', 7.5, (1.0, 1.0))[0][2:6, 20:22] == 8).all()                             # the first in values wins


def test_select_subsets_of_planes():
    rng = np.random.default_rng(5)
    planes = U.speckle_planes(rng, 6, 9, 130, 0.2)
    for select in ([True] * 6, [False] * 6, [True, False, False, True, False, True], [False, False, False, False, False, True]):
        for op in M.OPS:
            got = check(planes, None, op, 2.0, (0.8, 2.5), select=select)
            for k, s in enumerate(select):
                assert s or got[0][k].tobytes() == planes[k].tobytes()
                assert got[1][k, 0] == np.count_nonzero(planes[k])


def test_chunks_through_max_scratch_bytes():
    rng = np.random.default_rng(6)
    H, W = 9, 130
    n = H * W
    planes = U.speckle_planes(rng, 4, H, W, 0.1)
    values = [40, 30, 20, 10]
    lmap = U.speckle_map(rng, values, H, W, 0.3, others=(5,))
    for op in M.OPS:
        two = op in ('open', 'close')
        for seg, vals, per in ((planes, None, n * (3 if two else 2)), (lmap, values, n * (4 if two else 3))):
            whole = check(seg, vals, op, 3.0, (1.0, 1.0))
            for bound in (2 * per, 3 * per - 1, per):                # 2, 2 and 4 chunks
                assert U.same(check(seg, vals, op, 3.0, (1.0, 1.0), max_scratch_bytes=bound), whole)
            part = check(seg, vals, op, 3.0, (1.0, 1.0), select=[True, False, True, True], max_scratch_bytes=per)
            assert not U.same(part, whole)
    # a painting conflict that straddles two chunks: both labels reach the gap, the first of `values` wins whichever chunk it is in
    gap = np.zeros((3, 70), np.uint8)
    gap[1, 10] = 1
    gap[1, 16] = 2
    for vals, winner in (([1, 2], 1), ([2, 1], 2)):
        for bound in (0, 3 * 3 * 70):
            got = check(gap, vals, 'dilate', 4.0, (1.0, 1.0), max_scratch_bytes=bound)
            assert (got[0][1, 12:15] == winner).all()


def _raw(seg=None, seg_null=False, kind=0, values=None, K=2, hw=(3, 4), sp=(1.0, 1.0), op=0, r=1.0, select=None, bound=0, out=None, counters=None):
    lib = _lib.load()
    vals = None if values is None else np.ascontiguousarray(values, np.uint8)
    sel = None if select is None else np.ascontiguousarray(select, np.uint8)
    return lib.ts2d_label_morphology(0, None if seg_null else seg.ctypes.data, kind, None if vals is None else vals.ctypes.data, K, hw[0], hw[1],
                                     sp[0], sp[1], op, r, None if sel is None else sel.ctypes.data, bound, None if out is None else out.ctypes.data,
                                     None if counters is None else counters.ctypes.data)


def test_every_refusal_by_name_leaves_the_outputs_untouched():
    seg = np.ones((2, 3, 4), np.uint8)
    out, counters = np.full_like(seg, 99), np.full((2, 4), -77, np.int64)
    ok = dict(seg=seg, out=out, counters=counters)
    lm = dict(ok, kind=1, K=2, hw=(6, 4), values=[1, 2])
    nan, inf = float('nan'), float('inf')
    bad = [(dict(seg_null=True), 'null'), (dict(out=None), 'null'), (dict(counters=None), 'null'), (dict(kind=2), 'kind'), (dict(kind=-1), 'kind'),
           (dict(op=4), 'op'), (dict(op=-1), 'op'), (dict(K=0), 'K = 0'), (dict(K=256), 'K = 256'), (dict(hw=(0, 4)), 'extents'),
           (dict(hw=(3, -4)), 'extents'), (dict(hw=(32768, 1)), 'extents'), (dict(hw=(1, 32768)), 'extents'), (dict(r=-1.0), 'radius'),
           (dict(r=nan), 'radius'), (dict(r=inf), 'radius'), (dict(sp=(0.0, 1.0)), 'spacing'), (dict(sp=(1.0, -1.0)), 'spacing'),
           (dict(sp=(nan, 1.0)), 'spacing'), (dict(sp=(1.0, inf)), 'spacing'), (dict(bound=23), 'max_scratch_bytes'),
           (dict(op=2, bound=35), 'max_scratch_bytes')]
    bad_lm = [(dict(values=None), 'values'), (dict(values=[1, 0]), 'background'), (dict(values=[5, 5]), 'repeats'), (dict(bound=71), 'max_scratch_bytes')]
    for base, cases in ((ok, bad), (lm, bad_lm)):
        for change, word in cases:
            assert _raw(**dict(base, **change)) == -1, change         # TS2D_ERR_INVALID
            assert word in _lib.last_error() and 'ts2d_label_morphology' in _lib.last_error(), (change, _lib.last_error())
            assert (out == 99).all() and (counters == -77).all()
    # (32767 x 32767 passes the extent check and is refused for its 2^30 pixels' scratch, not for a 32-bit index: 32767^2 < 2^31 - 1)
    assert _raw(**dict(ok, K=1, hw=(32767, 32767), bound=1 << 20)) == -1 and 'max_scratch_bytes' in _lib.last_error()
    assert (out == 99).all() and (counters == -77).all()
    assert _raw(**dict(ok, bound=24)) == 0 and (out == 1).all() and counters.tolist() == [[12, 12, 0, 0]] * 2
    assert _raw(**dict(lm, bound=72)) == 0 and counters.tolist() == [[24, 24, 0, 0], [0, 0, 0, 0]]


def _image(multilabel):
    rng = np.random.default_rng(12)
    eye = tuple(float(v) for v in np.eye(3).reshape(-1))
    if multilabel:                                                   # what TS2D.predict returns: a unit axis in the middle
        planes = np.ascontiguousarray((rng.random((3, 40, 1, 70)) < 0.2).astype(np.uint8) * 255)
        seg = nrrd.Image(np.moveaxis(planes, 0, -1), (0.8, 7.0, 2.5), (0.0,) * 3, eye, 3, {}, None)
        image.set_annotation_meta(seg, {1: 'a', 2: 'b', 3: 'c'}, {})
    else:
        arr = ((rng.random((40, 70)) < 0.3) * rng.integers(1, 4, (40, 70)) * 3).astype(np.uint8)
        seg = nrrd.Image(arr, (0.8, 2.5), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 1, {}, None)
        image.set_annotation_meta(seg, {3: 'three', 6: 'six', 9: 'nine'}, {})
    return seg


def test_the_image_wrapper_on_the_device_equals_the_host_route(monkeypatch):
    calls = []
    orig = engine.label_morphology
    monkeypatch.setattr(engine, 'label_morphology', lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    for multilabel in (True, False):
        seg = _image(multilabel)
        before = seg.array.tobytes()
        names = list(image.get_annotation_labels(seg))
        for op in M.OPS:
            for labels in ('all', names[1:]):
                n = len(calls)
                dev, dev_ctr = M.label_morphology(seg, op, 2.6, device=0, labels=labels)
                assert len(calls) == n + 1
                host, host_ctr = M.label_morphology(seg, op, 2.6, labels=labels)
                assert len(calls) == n + 1                           # the host route made none
                assert dev.array.tobytes() == host.array.tobytes() != before and dev_ctr == host_ctr and dev.array.shape == seg.array.shape
                assert dev.meta == seg.meta and seg.array.tobytes() == before
            assert M.label_morphology(seg, op, 0.0, device=0)[0].array.tobytes() == before


def test_result_morphology_on_the_device_equals_the_host_route():
    ids = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_ribs')
    models = {m: synthetic_model(m, 3 + i, 31 + i, patch=(64, 64), mirror=False)[0] for i, m in enumerate(ids)}
    with TS2D(models=models) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device == 0
        before = res.get_segmentation().array.tobytes()
        dev = {op: res.morphology(op, 3.0) for op in M.OPS}
        assert res.morphology('open', 0.0).get_segmentation().array.tobytes() == before and dev['open'].device == 0
        res.device = None
        for op in M.OPS:
            host = res.morphology(op, 3.0)
            for m in [None] + list(ids):
                assert dev[op].get_segmentation(m).array.tobytes() == host.get_segmentation(m).array.tobytes()
            assert dev[op].get_segmentation().array.tobytes() != before and res.get_segmentation().array.tobytes() == before


def test_dilate_then_erode_in_two_calls_is_close_in_one():
    rng = np.random.default_rng(9)
    planes = U.speckle_planes(rng, 3, 67, 200, 0.05)
    for r, sp in ((3.0, (1.0, 1.0)), (6.0, (0.8, 2.5))):
        grown = check(planes, None, 'dilate', r, sp)[0]
        twice = check(grown, None, 'erode', r, sp)[0]
        once = check(planes, None, 'close', r, sp, must_change=True)[0]
        assert np.array_equal(twice > 0, once > 0)
        assert np.array_equal(check(check(planes, None, 'erode', r, sp)[0], None, 'dilate', r, sp)[0] > 0, check(planes, None, 'open', r, sp)[0] > 0)
