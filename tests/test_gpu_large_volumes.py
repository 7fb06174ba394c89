"""The label and volume entries at the sizes where their 32-bit quantities end ("32-bit quantities of the label and volume entries", has
the audit these cases belong to): voxel indices up to 2^31 - 2, byte offsets past 2^31 and 2^32 inside a planes or an intensity array, the slot
caps of the statistics planners, launches of more than 2^32 threads, an extent of 32767, projections of more than 2^31 elements, and a refusal by
name one step past every fence.  tests/large_volume_util.py builds the inputs (two islands in a volume of zeros), their twins and the boxed
distance statement; tests/test_large_volumes_cpu.py proves on the host that the references used here are the statements.

Every case prints what it needs before it allocates (``pytest -s``), skips only where ``torch.cuda.mem_get_info()`` or ``MemAvailable`` shows less, and
prints its wall time and result.  Everything is compared bit for bit; no time is asserted.

Shapes: V16 = (2047, 1024, 1024), n = 2^31 - 2^20 (a multiple of 16); VODD = (2047, 1023, 1025), n = 2 146 433 025 (odd: the scalar paths of
sdv_box and overlap_count; 17 words a row, the last of one voxel); VTHIN = (8193, 8192, 1), Z * H > 2^26: stats_rows and every cc_* / lc_* kernel
would be launched with more than 2^32 threads.

WHAT THE CASES FOUND.  (1) The runtime does NOT refuse a launch of more than 2^32 - 1 work-items along x: the count wraps and a part of the grid
runs.  Before this module VTHIN gave, with status 0, the counts of the first z-slab alone (ts2d_label_components: 74 of 336 voxels).  Fix: the
grids of stats_rows and of every cc_* / lc_* kernel FOLD along z (csrc/entry_util.h: fold_grid; case e).  ts2d_volume_surface_distances, whose
sdv_planes / sdv_rows launch one wave per box row, and ts2d_project_coronal, one lane per output pixel, refuse such a box / plane by name (case h).
(2) Nothing else: every index, offset and cap below gave the statement's bits.

Departures from the issue's wording, each because the statement cannot be run as asked:
  * volume distances (a, f) and the 2-D profile (f) compare against ``large_volume_util.boxed_distance_statement``, not against the statement on a
    twin: the statement is O(voxels * H) and allocates [H, H] and [W, W] float64 tables - minutes on a twin of 1024 x 1024 slabs, 8.6 GB per table at
    an extent of 32767.  The boxed form is the statement's arithmetic at the border voxels only; the CPU module holds it to the statement's bits.
  * the integer-only cases on VODD (overlap, components) cut their twins without the multiple-of-64 rule (H = 1023 would leave a twin of 63 slabs,
    66 M voxels): no float sum is compared there.
  * c: "the same call with the default budget" is refused by name - ONE label's partials at (512, 512, 2) x 64 channels take 273.7 MB, above the
    default 256 MiB - so the slot-cap run is compared with a run whose budget decides (32 labels a chunk); and the shape is (515, 256, 2), the
    fewest rows at which the cap binds (the case's docstring).
  * g: ts2d_project_coronal_modes stops at rays of 8192 samples and 2^28 output samples, so its view of the same buffer is (8, 8192, 32769).
  * d: with a budget of two sets the second set of a chunk starts at byte 2^31 of parent / count (not 2^32); plane 2 starts at byte 2^30 of seg.

Long chains against kCcFindCap (part 4): status of ts2d_keep_largest_components / ts2d_label_components full / faces on the MI355X (256 CUs):
  (100000, 1, 1)  0 / 0 / 0        (1, 100000, 1)  0 / 0 / 0        serpentine of 65 792 voxels in (4, 256, 256)  0 / 0 / 0
No GIVE_UP was seen; the cases accept either status and hold the outputs to the statement (0) or to "untouched" (GIVE_UP).

Measured on an MI355X (288 GB, 287 GB free; the host shows 2.6 TB available), no case skipped, every result equal to its reference.  Need on the
device / on the host, wall time of the case (inputs, references, every device call):
  a overlap V16, VODD          4.0 / 4.1 GiB    0.44, 0.30 s         a overlap planes K = 5         6.0 / 6.1 GiB    0.45 s
  a distances V16, VODD        4.1 / 4.1 GiB    0.45, 0.49 s         b statistics V16, C = 0        2.3 / 2.1 GiB    0.17 s
  b C = 1 at (1025,1024,1024)  5.3 / 5.3 GiB    0.91 s (statistics, percentiles, the NaN call and its percentiles: four uploads)
  c statistics (515,256,2)     32.8 / 0.3 GiB   2.3 s  ((512, 512, 2) with three device calls: 14.0 s)
  c percentiles (4097,2048,2)  40.0 / 0.2 GiB   5.9 s  (rows > 2^23 with K = 255 sets the shape: 255 labels x 8 rounds over 16.8 M voxels, twice)
  d components VODD            20.3 / 6.1 GiB   1.5 s (three device calls)   d keep_largest VODD  20.3 / 6.1 GiB  0.50 s
  d planes K = 3               10.7 / 4.5 GiB   0.36 s               e VTHIN (five entries' calls)  4.2 / 0.5 GiB    1.6 s
  f volume distances           0.19, 0.34, 0.01 s                    f 2-D profile                  0.03, 0.01 s
  g projections                2.1 / 4.0 GiB    5.7 s, most of it numpy's six reductions over 2.1 GB on the host (n_elems > 2^31 sets the size)
  h refusals, chains           below 0.1 s each          h thin box  4.8 s: the served box of 2^26 - 2048 rows x 2048 candidates a voxel in pass 2
The whole module: 31 s.
"""
import ctypes

import numpy as np
import pytest

from tests import components_util as U
from tests import large_volume_util as L
from totalsegmentator2d_amd import _lib, engine, evaluate as E, image, nrrd, postprocess, statistics as S
from totalsegmentator2d_amd import components as C

pytestmark = pytest.mark.gpu

V16, VODD, VTHIN = (2047, 1024, 1024), (2047, 1023, 1025), (8193, 8192, 1)
KEEP = (3, 3)                                        # slabs the twins keep at either end: the island's two and an empty one
VALUES = [7, 200, 41]
NEAR, FAR = [7, 200], [41, 9]                        # labels confined to ONE island each (the distances)
SPACING, TOL, QS = (2.5, 0.8, 1.3), [0.8, 3.0], (0, 50, 95, 100)


def _n(shape):
    return int(np.prod(shape, dtype=np.int64))


def _free():
    import torch
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


def _nothing_held(before):
    """The free device memory has not dropped (by more than a MiB of runtime bookkeeping): the call holds no allocation."""
    return _free() >= before - (1 << 20)


# ------------------------------------------------------------------------------------------------------------------ a. overlap and box
@pytest.mark.parametrize('shape', [V16, VODD], ids=['V16', 'Vodd'])
def test_a_overlap_of_label_maps_at_the_index_edge(shape):
    n = _n(shape)
    assert (n % 16 == 0) == (shape == V16) and 2 ** 31 - 2 ** 21 < n <= 2 ** 31 - 1
    L.require(f'a overlap {shape}', 2 * n + (1 << 20), 2 * n + (64 << 20))
    with L.Clock(f'a overlap {shape}') as c:
        a, b = L.two_islands(shape, (2, 24, 70), 1, VALUES), L.two_islands(shape, (2, 24, 70), 2, VALUES)
        (at, _), (bt, _) = L.twin_of(a, *KEEP, integers_only=True), L.twin_of(b, *KEEP, integers_only=True)
        want = E.overlap_statement(at, E.LABELMAP, bt, E.LABELMAP, VALUES)
        got = E._device_overlap(a, E.LABELMAP, b, E.LABELMAP, VALUES, shape, 0)
        assert L.same_dict(got, want, ('n_a', 'n_b', 'n_both')), (got, want)
        assert want['n_both'].min() > 50 and a[-1, -1, -1] == b[-1, -1, -1] == VALUES[-1]
        c.result = f"n_both {want['n_both'].tolist()}"


def test_a_overlap_of_planes_whose_bytes_pass_2_32():
    shape, K = (1024, 1024, 1024), 5
    n = _n(shape)
    assert 2 * n == 2 ** 31 and 4 * n == 2 ** 32                                          # plane 2 starts at byte 2^31, plane 4 at byte 2^32
    L.require('a overlap planes K=5', (K + 1) * n + (1 << 20), (K + 1) * n + (64 << 20))
    with L.Clock('a overlap planes K=5') as c:
        a = np.zeros((K,) + shape, np.uint8)
        for k in range(K):
            L.two_islands(shape, (2, 24, 70), 10 + k, [1 + 50 * k], out=a[k])
        b = L.two_islands(shape, (2, 24, 70), 3, [3, 4, 5, 6, 7])
        values = [3, 4, 5, 6, 7]
        (at, _), (bt, _) = L.twin_of(a, *KEEP, axis=1), L.twin_of(b, *KEEP)
        want = E.overlap_statement(at, E.PLANES, bt, E.LABELMAP, values)
        got = E._device_overlap(a, E.PLANES, b, E.LABELMAP, values, shape, 0)
        assert L.same_dict(got, want, ('n_a', 'n_b', 'n_both')), (got, want)
        assert want['n_both'].min() > 20 and want['n_a'].min() > 1000
        c.result = f"n_a {want['n_a'].tolist()} n_both {want['n_both'].tolist()}"


def _boxed_islands(a, b, values, shape, window):
    """The distance statement of label maps whose labels NEAR live in the low corner and FAR in the high one: each from its own crop."""
    Z, H, W = shape
    s, wy, wx = (v + 1 for v in window)                                                  # (the crop: the window and a background shell)
    near = L.boxed_distance_statement(a[:s, :wy, :wx], E.LABELMAP, b[:s, :wy, :wx], E.LABELMAP, values, SPACING, TOL, QS, (0, 0, 0), shape)
    far = L.boxed_distance_statement(a[Z - s:, H - wy:, W - wx:], E.LABELMAP, b[Z - s:, H - wy:, W - wx:], E.LABELMAP, values, SPACING, TOL, QS,
                                     (Z - s, H - wy, W - wx), shape)
    return {f: np.concatenate([near[f][:len(NEAR)], far[f][len(NEAR):]]) for f in L.DISTANCE_FIELDS}


@pytest.mark.parametrize('shape', [V16, VODD], ids=['V16', 'Vodd'])
def test_a_volume_distances_with_a_box_corner_at_the_last_voxel(shape):
    n, window, values = _n(shape), (2, 12, 70), NEAR + FAR
    L.require(f'a distances {shape}', 2 * n + (64 << 20), 2 * n + (64 << 20))
    with L.Clock(f'a distances {shape}') as c:
        a, b = L.two_islands(shape, window, 5, NEAR, FAR), L.two_islands(shape, window, 6, NEAR, FAR)
        want = _boxed_islands(a, b, values, shape, window)
        got = E._device_volume_distances(a, E.LABELMAP, b, E.LABELMAP, values, shape, SPACING, TOL, QS, True, 0)
        assert L.same_dict(got, want, L.DISTANCE_FIELDS), {f: (got[f], want[f]) for f in L.DISTANCE_FIELDS if not L.same_dict(got, want, (f,))}
        assert want['border'].min() > 10 and np.isfinite(want['dist_sum']).all() and a[-1, -1, -1] == b[-1, -1, -1] == FAR[-1]
        plain = E._device_volume_distances(a, E.LABELMAP, b, E.LABELMAP, values, shape, SPACING, TOL, None, False, 0)
        assert L.same_dict(plain, want, L.DISTANCE_FIELDS[:3])
        c.result = f"border {want['border'].tolist()} dist_sum {want['dist_sum'][:, 0].tolist()}"


# ------------------------------------------------------------------------------------------------------------------ b. statistics at the index edge
def test_b_statistics_of_a_label_map_at_the_index_edge():
    shape, values = V16, VALUES + [99]                                                    # 99 is absent
    n = _n(shape)
    L.require('b statistics V16 C=0', n + (256 << 20), n + (64 << 20))
    with L.Clock('b statistics V16 C=0') as c:
        big = L.two_islands(shape, (2, 24, 70), 4, VALUES)
        twin, removed = L.twin_of(big, *KEEP)
        want = L.shifted_statistics(S.label_statistics_statement(twin, None, (1, 1, 1), values), twin, values, KEEP[0], removed, shape[0])
        got = S._device_statistics(big, values, shape, None, (1, 1, 1), 0)
        assert got is not None and L.same_dict(got, want, L.STATISTICS_FIELDS), (got, want)
        assert want['bbox_max'][2].tolist() == [shape[0] - 1, shape[1] - 1, shape[2] - 1] and want['index_sum'][:3, 0].min() > 2040 * 100
        c.result = f"count {want['count'].tolist()} z sums {want['index_sum'][:, 0].tolist()}"


def _raw_statistics(seg, values, shape, x, out_int, out_f64):
    vals = np.ascontiguousarray(values, np.uint8)
    status = ctypes.c_int(-77)
    rc = _lib.load().ts2d_label_statistics(0, seg.ctypes.data, _lib.STATS_LABELMAP, vals.ctypes.data, len(values), *shape, x.ctypes.data, x.shape[0], 0,
                                           out_int.ctypes.data, out_f64.ctypes.data, ctypes.byref(status))
    return rc, status.value


def test_b_statistics_and_percentiles_with_intensities_past_2_32_bytes():
    shape, values = (1025, 1024, 1024), VALUES
    n, window = _n(shape), (2, 24, 70)
    assert n * 4 > 2 ** 32
    L.require('b statistics C=1 at (1025, 1024, 1024)', 5 * n + (256 << 20), 5 * n + (256 << 20))
    with L.Clock('b statistics C=1 at (1025, 1024, 1024)') as c:
        big = L.two_islands(shape, window, 7, values)
        x = np.zeros((1,) + shape, np.float32)
        rng = np.random.default_rng(8)
        s, wy, wx = window
        for where in ((slice(0, s), slice(0, wy), slice(0, wx)), (slice(shape[0] - s, None), slice(shape[1] - wy, None), slice(shape[2] - wx, None))):
            x[0][where] = (rng.normal(size=window) * rng.choice([1e-3, 1.0, 1e4], size=window)).astype(np.float32)
        twin, removed = L.twin_of(big, *KEEP)
        xt, _ = L.twin_of(x, *KEEP, axis=1)
        want = L.shifted_statistics(S.label_statistics_statement(twin, xt, (1, 1, 1), values), twin, values, KEEP[0], removed, shape[0])
        got = S._device_statistics(big, values, shape, x, (1, 1, 1), 0)
        assert got is not None and L.same_dict(got, want, L.STATISTICS_FIELDS), {f: (got[f], want[f]) for f in L.STATISTICS_FIELDS}
        qs = (0, 5, 50, 95, 100)
        got_p = S._device_percentiles(big, values, shape, x, qs, 0)
        assert got_p is not None and L.same_dict(got_p, S.label_percentiles_statement(twin, xt, qs, values), L.PERCENTILE_FIELDS)
        # a NaN under the label of the last voxel: the status bit, and the outputs stay as they were
        assert big[-1, -1, -1] == values[-1]
        x[0, -1, -1, -1] = np.nan
        out_int, out_f64 = np.full((3, 10), -77, np.int64), np.full((3, 1, 6), -77.0, np.float64)
        rc, status = _raw_statistics(big, values, shape, x, out_int, out_f64)
        assert rc == 0 and status == _lib.STATS_NONFINITE and (out_int == -77).all() and (out_f64 == -77.0).all()
        assert S._device_percentiles(big, values, shape, x, qs, 0) is None
        c.result = f"sum {want['sum'][:, 0].tolist()} std {want['std'][:, 0].tolist()}"


# ------------------------------------------------------------------------------------------------------------------ c. the slot caps
def test_c_the_slot_cap_of_the_statistics_decides_the_chunk():
    """The cap binds once K * C * rows passes 2^31 - 1, and the kernels' work is K * C * rows wave passes whatever the shape: at the issue's
    (512, 512, 2) the case took 14 s on the MI355X, so the rows are the fewest that cross with K = 255 and C = 64 - 515 * 256 = 131 840 (131 587 would
    do): 254 labels a chunk, then one."""
    shape, K, Cn = (515, 256, 2), 255, 64
    n, rows = _n(shape), 515 * 256
    per = rows * (20 + 16 * Cn)
    budget = 255 * per                                                                    # room for all 255 labels: (2^31 - 1) // (rows * C) = 254 decides
    assert engine.statistics_chunk_labels(shape, K, Cn, budget) == (254, 'slot_cap') and (2 ** 31 - 1) // (rows * Cn) == 254
    assert 254 * Cn * rows <= 2 ** 31 - 1 < K * Cn * rows and K * Cn * (rows - 254) <= 2 ** 31 - 1          # the fewest rows but 253
    assert engine.statistics_chunk_labels(shape, K, Cn, 32 * per) == (32, 'budget')
    assert engine.statistics_chunk_labels((512, 512, 2), K, Cn, 0)[0] == 0                # the issue's shape under the default budget: refused by name
    L.require('c statistics K=255 C=64', 254 * per + K * n + 4 * Cn * n + (64 << 20), 2 * (K * n + 4 * Cn * n))
    with L.Clock('c statistics K=255 C=64') as c:
        rng = np.random.default_rng(9)
        planes = (rng.integers(0, 50, (K,) + shape, dtype=np.uint8) == 0).astype(np.uint8) * 255
        x = rng.standard_normal((Cn,) + shape, dtype=np.float32)
        capped = engine.label_statistics(planes, _lib.STATS_PLANES, None, shape, x, budget)
        by_budget = engine.label_statistics(planes, _lib.STATS_PLANES, None, shape, x, 32 * per)
        assert capped is not None and by_budget is not None
        assert capped[0].tobytes() == by_budget[0].tobytes() and capped[1].tobytes() == by_budget[1].tobytes()
        ks, cs = [0, 253, 254], [0, 63]                                                   # the labels on either side of the chunk boundary
        want = S.label_statistics_statement(planes[ks], x[cs], (1, 1, 1))
        oi, of = capped[0][ks], capped[1][ks][:, cs]
        assert oi[:, 0].tobytes() == want['count'].tobytes() and oi[:, 1:4].tobytes() == want['index_sum'].tobytes()
        assert np.array_equal(oi[:, 4:10:2], want['bbox_min']) and np.array_equal(oi[:, 5:10:2], want['bbox_max'])
        for j, f in enumerate(('sum', 'ssq', 'mean', 'std')):
            assert np.ascontiguousarray(of[:, :, j]).tobytes() == want[f].tobytes(), f
        assert np.array_equal(of[:, :, 4].astype(np.float32), want['min']) and np.array_equal(of[:, :, 5].astype(np.float32), want['max'])
        assert want['count'].min() > 1000
        small = np.ones((1, 512, 512, 2), np.uint8)                                       # ONE label of the issue's shape: above the default 256 MiB
        with pytest.raises(RuntimeError, match='above max_scratch_bytes = 268435456'):
            engine.label_statistics(small, _lib.STATS_PLANES, None, (512, 512, 2), np.zeros((Cn, 512, 512, 2), np.float32), 0)
        c.result = f"count {want['count'].tolist()}"


def test_c_the_slot_cap_of_the_percentiles_decides_the_chunk():
    shape, K, P = (4097, 2048, 2), 255, 8
    n, rows = _n(shape), 4097 * 2048
    assert rows > 2 ** 23 and (2 ** 31 - 1) // rows == 255
    one = 2 * P * 1040 + rows * 20
    budget = 256 * one
    assert engine.percentiles_chunk_labels(shape, K, 1, P, budget) == (255, 'slot_cap')
    assert engine.percentiles_chunk_labels(shape, K, 1, P, 16 * one) == (16, 'budget')
    L.require('c percentiles K=255 rows > 2^23', 255 * one + 5 * n + (64 << 20), 12 * n)
    with L.Clock('c percentiles K=255 rows > 2^23') as c:
        rng = np.random.default_rng(10)
        values = [int(v) for v in rng.permutation(np.arange(1, 256))]
        seg = np.where(rng.random(shape) < 0.5, np.asarray(values, np.uint8)[rng.integers(0, K, shape)], 0).astype(np.uint8)
        x = rng.normal(size=(1,) + shape).astype(np.float32)
        qs = (0, 5, 25, 50, 75, 95, 99.9, 100)
        capped = engine.label_percentiles(seg, _lib.STATS_LABELMAP, values, shape, x, qs, budget)
        by_budget = engine.label_percentiles(seg, _lib.STATS_LABELMAP, values, shape, x, qs, 16 * one)
        assert capped is not None and by_budget is not None and all(p.tobytes() == q.tobytes() for p, q in zip(capped, by_budget))
        ks = [0, 15, 16, 254]
        want = S.label_percentiles_statement(seg, x, qs, [values[k] for k in ks])
        assert capped[0][ks].tobytes() == want['count'].tobytes() and capped[1][ks].tobytes() == want['rank_value'].tobytes()
        assert capped[2][ks].tobytes() == want['rank_weight'].tobytes() and want['count'].min() > 10000
        c.result = f"count {want['count'].tolist()}"


# ------------------------------------------------------------------------------------------------------------------ d. components at the index edge
def _check_components(tag, big, values, shape, twin, removed, conn, rule, capacity, scratch):
    n_slab = shape[1] * shape[2]
    want = C.label_components_statement(twin, values, conn, **rule)
    got = engine.label_components(big, _lib.STATS_LABELMAP, values, shape, C.CONNECTIVITIES.index(conn), rule.get('keep_largest', False),
                                  rule.get('min_voxels'), max_scratch_bytes=scratch, capacity=capacity)
    assert got is not None, f'{tag}: TS2D_COMP_GIVE_UP'
    assert np.array_equal(got[1], want[1]), (tag, got[1].tolist(), want[1].tolist())
    assert np.array_equal(got[2], L.shifted_components(want[2], KEEP[0] * n_slab, removed * n_slab)), tag
    assert np.array_equal(got[0][:KEEP[0]], want[0][:KEEP[0]]) and np.array_equal(got[0][shape[0] - KEEP[1]:], want[0][KEEP[0]:]), tag
    assert L.middle_is_empty(got[0], *KEEP), tag
    assert (got[2][:, 1] >= (shape[0] - KEEP[1] + 1) * n_slab).any() and want[1][:, 3].min() > 0, tag      # roots in the last slabs; something was removed
    return want


def test_d_components_of_a_label_map_at_the_index_edge():
    shape = VODD
    n = _n(shape)
    scratch = engine.components_state_bytes(shape)
    assert scratch >= 9 * n + n // 8 and n % 2 == 1 and (shape[2] + 63) // 64 == 17
    L.require('d components Vodd', n + scratch + (64 << 20), 3 * n + (64 << 20))
    with L.Clock('d components Vodd') as c:
        big = L.two_islands(shape, (2, 24, 70), 11, VALUES)
        twin, removed = L.twin_of(big, *KEEP, integers_only=True)
        rule = dict(keep_largest=True, min_voxels=[2, 3, 2])
        total = len(C.label_components_statement(twin, VALUES, 'full')[2])
        assert 50 < total < 65536
        want = _check_components('full, a list of 40 rows is full once', big, VALUES, shape, twin, removed, 'full', rule, 40, scratch)
        _check_components('faces, the default list is never full', big, VALUES, shape, twin, removed, 'faces', rule, None, scratch)
        with pytest.raises(RuntimeError, match='above max_scratch_bytes'):
            engine.label_components(big, _lib.STATS_LABELMAP, VALUES, shape, max_scratch_bytes=scratch - 1, want_seg=False)
        c.result = f'components {want[1][:, 1].tolist()} removed {want[1][:, 4].tolist()}'


def test_d_keep_largest_with_two_steps_at_the_index_edge():
    shape = VODD
    n = _n(shape)
    L.require('d keep_largest Vodd', n + engine.components_state_bytes(shape) + (64 << 20), 3 * n + (64 << 20))
    with L.Clock('d keep_largest Vodd') as c:
        big = L.two_islands(shape, (2, 24, 70), 12, VALUES)
        twin, _ = L.twin_of(big, *KEEP, integers_only=True)
        plan = postprocess.PostprocessingPlan([([7, 200], 0), ([41], 9)])
        want, want_stats = postprocess.keep_largest_components_statement(twin, plan)
        out, stats, status = engine.keep_largest_components(big, *plan.compiled)
        assert status == 0 and np.array_equal(stats, want_stats) and want_stats[:, 3].min() > 0
        assert np.array_equal(out[:KEEP[0]], want[:KEEP[0]]) and np.array_equal(out[shape[0] - KEEP[1]:], want[KEEP[0]:]) and L.middle_is_empty(out, *KEEP)
        c.result = f'stats {want_stats.tolist()}'


def test_d_components_of_planes_in_chunks_of_two_sets():
    shape, K = (1024, 1024, 512), 3
    n = _n(shape)
    one = engine.components_state_bytes(shape)
    assert 2 * n == 2 ** 30 and n * 4 == 2 ** 31                                           # plane 2 at byte 2^30 of seg; set 1 of a chunk at byte 2^31 of parent / count
    L.require('d components planes K=3', K * n + 2 * one + (64 << 20), 3 * K * n)
    with L.Clock('d components planes K=3') as c:
        planes = np.zeros((K,) + shape, np.uint8)
        for k in range(K):
            L.two_islands(shape, (2, 24, 70), 20 + k, [1 + 100 * k], out=planes[k])
        twin, removed = L.twin_of(planes, *KEEP, axis=1, integers_only=True)
        n_slab = shape[1] * shape[2]
        want = C.label_components_statement(twin, None, 'full', True, None)
        got = engine.label_components(planes, _lib.STATS_PLANES, None, shape, 0, True, None, max_scratch_bytes=2 * one + one // 2)
        assert got is not None and np.array_equal(got[1], want[1]) and want[1][:, 3].min() > 0
        assert np.array_equal(got[2], L.shifted_components(want[2], KEEP[0] * n_slab, removed * n_slab))
        assert np.array_equal(got[0][:, :KEEP[0]], want[0][:, :KEEP[0]]) and np.array_equal(got[0][:, shape[0] - KEEP[1]:], want[0][:, KEEP[0]:])
        assert L.middle_is_empty(got[0], *KEEP, axis=1)
        c.result = f'components {want[1][:, 1].tolist()}'


# ------------------------------------------------------------------------------------------------------------------ e. more than 2^32 threads
def test_e_launches_of_more_than_2_32_threads_fold_their_grids():
    """Found by this case: the runtime cuts such a launch short instead of refusing it (the module docstring).  The grids fold (csrc/entry_util.h)."""
    shape, window = VTHIN, (2, 4000, 1)
    n = _n(shape)
    assert shape[0] * shape[1] * 64 > 2 ** 32 and (n + 3) // 4 * 256 > 2 ** 32
    L.require('e Vthin', 3 * 20 * n + 6 * n + (64 << 20), 8 * n)
    assert engine.components_state_bytes(shape) == 17 * n
    with L.Clock('e Vthin') as c:
        big = L.two_islands(shape, window, 13, VALUES)
        twin, removed = L.twin_of(big, *KEEP)
        want = L.shifted_statistics(S.label_statistics_statement(twin, None, (1, 1, 1), VALUES), twin, VALUES, KEEP[0], removed, shape[0])
        got = S._device_statistics(big, VALUES, shape, None, (1, 1, 1), 0, 3 * 20 * n)
        assert got is not None and L.same_dict(got, want, L.STATISTICS_FIELDS), (got, want)
        assert want['count'].min() > 1000 and want['bbox_max'][:, 0].tolist() == [shape[0] - 1] * 3
        x = np.zeros((1,) + shape, np.float32)                                             # the same rows through ts2d_label_percentiles
        x[0, :2], x[0, -2:] = 1.5, -2.5
        got_p = S._device_percentiles(big, VALUES, shape, x, (50,), 0, 3 * (2 * 1040 + 20 * n))
        assert got_p is not None and np.array_equal(got_p['count'], want['count'])
        for conn in C.CONNECTIVITIES:
            _check_components(f'Vthin {conn}', big, VALUES, shape, twin, removed, conn, dict(keep_largest=True, min_voxels=[2, 2, 2]), None,
                              engine.components_state_bytes(shape))          # (17 bytes a voxel at W = 1: above the default GiB)
        plan = postprocess.PostprocessingPlan([([7, 200], 0), ([41], 9)])
        want_seg, want_stats = postprocess.keep_largest_components_statement(twin, plan)
        out, stats, status = engine.keep_largest_components(big, *plan.compiled)
        assert status == 0 and np.array_equal(stats, want_stats) and want_stats[:, 0].min() > 1000
        assert np.array_equal(out[:KEEP[0]], want_seg[:KEEP[0]]) and np.array_equal(out[shape[0] - KEEP[1]:], want_seg[KEEP[0]:]) and L.middle_is_empty(out, *KEEP)
        c.result = f"count {want['count'].tolist()} keep_largest {want_stats.tolist()}"


# ------------------------------------------------------------------------------------------------------------------ f. extent 32767
def _ends(shape, seed):
    """Side A: a voxel at the first corner and a few around it; side B: one at the last corner and a few around it.  Planes, K = 1."""
    rng = np.random.default_rng(seed)
    a, b = np.zeros((1,) + tuple(shape), np.uint8), np.zeros((1,) + tuple(shape), np.uint8)
    lo = tuple(slice(0, min(3, s)) for s in shape)
    hi = tuple(slice(max(0, s - 3), s) for s in shape)
    a[0][lo] = rng.random(a[0][lo].shape) < 0.6
    b[0][hi] = (rng.random(b[0][hi].shape) < 0.6) * 200
    a[(0,) + (0,) * len(shape)] = 1
    b[(0,) + tuple(s - 1 for s in shape)] = 200
    return a, b


@pytest.mark.parametrize('shape', [(32767, 2, 65), (2, 32767, 65), (2, 3, 32767)])
def test_f_volume_distances_at_an_extent_of_32767(shape):
    with L.Clock(f'f volume distances {shape}') as c:
        a, b = _ends(shape, sum(shape))
        want = L.boxed_distance_statement(a, E.PLANES, b, E.PLANES, None, SPACING, TOL, QS)
        got = E._device_volume_distances(a, E.PLANES, b, E.PLANES, None, shape, SPACING, TOL, QS, True, 0, 1 << 32)
        assert L.same_dict(got, want, L.DISTANCE_FIELDS), {f: (got[f], want[f]) for f in L.DISTANCE_FIELDS if not L.same_dict(got, want, (f,))}
        i = int(np.argmax(shape))
        assert want['d2_max'][0, 0] >= ((shape[i] - 6) * SPACING[i]) ** 2 and want['within'].sum() == 0      # line distances of 32761 and more
        c.result = f"d2_max {want['d2_max'].tolist()} dist_sum {want['dist_sum'].tolist()}"


@pytest.mark.parametrize('shape', [(32767, 3), (3, 32767)])
def test_f_distance_profile_at_an_extent_of_32767(shape):
    with L.Clock(f'f distance profile {shape}') as c:
        a, b = _ends(shape, sum(shape))
        want = L.boxed_distance_statement(a, E.PLANES, b, E.PLANES, None, SPACING[1:], TOL, QS)
        got = E._device_profile(a, E.PLANES, b, E.PLANES, None, shape, SPACING[1:], TOL, QS, True, 0)
        assert L.same_dict(got, want, L.DISTANCE_FIELDS), {f: (got[f], want[f]) for f in L.DISTANCE_FIELDS if not L.same_dict(got, want, (f,))}
        plain = E._device_surface(a, E.PLANES, b, E.PLANES, None, shape, SPACING[1:], TOL, 0)
        assert L.same_dict(plain, want, L.DISTANCE_FIELDS[:3])
        c.result = f"d2_max {want['d2_max'].tolist()}"


def _raw_distances(entry, extents, spacing):
    """The entry on a one-byte segmentation it must refuse before it reads it.  Returns the status code; the message is ``_lib.last_error()``."""
    seg, tol = np.ones(1, np.uint8), np.ones(1, np.float64)
    oi, of = np.zeros(8, np.int64), np.zeros(8, np.float64)
    head = (0, seg.ctypes.data, _lib.STATS_PLANES, seg.ctypes.data, _lib.STATS_PLANES, None, 1) + tuple(extents) + tuple(float(s) for s in spacing) + (tol.ctypes.data, 1)
    fn = getattr(_lib.load(), entry)
    if entry == 'ts2d_surface_distances':
        return fn(*head, 0, oi.ctypes.data, of.ctypes.data)
    return fn(*head, None, 0, 0, 0, oi.ctypes.data, of.ctypes.data, None, None, None)


def test_f_an_extent_of_32768_is_refused_by_name_on_every_axis():
    before = _free()
    for axis in range(3):
        ext = [2, 2, 2]
        ext[axis] = 32768
        assert _raw_distances('ts2d_volume_surface_distances', ext, (1, 1, 1)) == -1
        assert 'outside 1 ... 32767' in _lib.last_error() and 'ts2d_volume_surface_distances' in _lib.last_error(), _lib.last_error()
    for entry in ('ts2d_surface_distances', 'ts2d_surface_distance_profile'):
        for ext in ((32768, 2), (2, 32768)):
            assert _raw_distances(entry, ext, (1, 1)) == -1
            assert 'outside 1 ... 32767' in _lib.last_error() and entry in _lib.last_error(), _lib.last_error()
    assert _nothing_held(before)
    assert _raw_distances('ts2d_volume_surface_distances', (1, 1, 1), (1, 1, 1)) == 0        # ... and a good small call


# ------------------------------------------------------------------------------------------------------------------ g. projections past 2^31 elements
N_ELEMS = 2 ** 31 + 2 ** 16


def _view(buf, extents, strides, base):
    return np.lib.stride_tricks.as_strided(buf[base:], extents, strides, writeable=False)      # (uint8: element strides are byte strides)


def test_g_projections_of_a_volume_past_2_31_elements():
    """The flipped view (every stride negative, base the last element) IS ``v[::-1, ::-1, ::-1]`` of the plain view - asserted on address and strides - so
    its reference is numpy's result on the plain view flipped along the two output axes: a reduction along y does not care for the order along y."""
    ext, mext = (2, 32769, 32768), (8, 8192, 32769)
    assert _n(ext) == N_ELEMS and _n(mext) == N_ELEMS
    L.require('g projections', N_ELEMS + (64 << 20), 2 * N_ELEMS)
    lib = _lib.load()
    with L.Clock('g projections') as c:
        rng = np.random.default_rng(14)
        buf = np.zeros(N_ELEMS, np.uint8)
        buf[:1 << 16] = rng.integers(0, 4, 1 << 16)
        buf[-(1 << 16):] = rng.integers(0, 4, 1 << 16)
        buf[0], buf[-1] = 5, 4                                                             # the samples that decide the maximum of their columns
        refs = {}
        for e in (ext, mext):
            strides = (e[1] * e[2], e[2], 1)
            v = _view(buf, e, strides, 0)
            f = _view(buf, e, tuple(-s for s in strides), N_ELEMS - 1)
            r = v[::-1, ::-1, ::-1]
            assert f.strides == r.strides and f.__array_interface__['data'][0] == r.__array_interface__['data'][0] and f.shape == r.shape
            mean = (v.sum(axis=1, dtype=np.int64).astype(np.float64) / np.float64(e[1])).astype(np.float32)
            refs[e] = {'max': v.max(axis=1).astype(np.float32), 'mean': mean}
            if e == ext:
                at = np.nonzero(v)                                                       # the statement of the label projection (evaluate.project_labels)
                planes = np.zeros((5, e[0], e[2]), np.uint8)
                planes[v[at].astype(np.intp) - 1, at[0], at[2]] = 1
                refs[e]['labels'] = planes
            else:
                refs[e]['min'] = v.min(axis=1).astype(np.float32)
        assert refs[ext]['max'][0, 0] == 5.0 and refs[ext]['max'][-1, -1] == 4.0 and refs[ext]['labels'][4].sum() == 1 and refs[ext]['labels'][4, 0, 0] == 1
        for flip in (False, True):
            def want(e, name):
                return refs[e][name][..., ::-1, ::-1] if flip else refs[e][name]
            strides, base = ((ext[1] * ext[2], ext[2], 1), 0) if not flip else ((-ext[1] * ext[2], -ext[2], -1), N_ELEMS - 1)
            omax, omean = np.empty((ext[0], ext[2]), np.float32), np.empty((ext[0], ext[2]), np.float32)
            _lib.check(lib.ts2d_project_coronal(0, buf.ctypes.data, buf.size, 1, *ext, *strides, base, omax.ctypes.data, omean.ctypes.data), 'ts2d_project_coronal')
            assert np.array_equal(omax, want(ext, 'max')) and np.array_equal(omean, want(ext, 'mean')), flip
            planes, status = engine.project_labels_coronal(buf, ext, strides, base, 5)
            assert status == 0 and np.array_equal(planes, want(ext, 'labels')), flip
            # one kernel of kernels_project_modes.h (project_modes_stream: max, min, mean) on the same buffer as (8, 8192, 32769)
            ms, mbase = ((mext[1] * mext[2], mext[2], 1), 0) if not flip else ((-mext[1] * mext[2], -mext[2], -1), N_ELEMS - 1)
            codes, sidx = np.array([0, 1, 2], np.int32), np.zeros(3, np.int32)              # TS2D_PROJECT_MAX, _MIN, _MEAN
            out, st = np.empty((3, mext[0], mext[2]), np.float32), np.zeros(1, np.int32)
            _lib.check(lib.ts2d_project_coronal_modes(0, buf.ctypes.data, buf.size, 1, *mext, *ms, mbase, codes.ctypes.data, sidx.ctypes.data, 3,
                                                      out.ctypes.data, None, None, None, st.ctypes.data), 'ts2d_project_coronal_modes')
            assert st[0] == 0 and np.array_equal(out[0], want(mext, 'max')) and np.array_equal(out[1], want(mext, 'min')), flip
            assert np.array_equal(out[2], want(mext, 'mean')) and out[0].max() == 5.0, flip
        c.result = 'max, mean, labels and the modes equal numpy on the strided view, plain and flipped'


# ------------------------------------------------------------------------------------------------------------------ h. refusals one past each fence
def _raw_volume_entries(Z, H, W):
    """Every volume entry on a one-byte segmentation with the extents (Z, H, W): name -> status code and message."""
    lib = _lib.load()
    seg, vals = np.ones(1, np.uint8), np.ones(1, np.uint8)
    x, q = np.ones(1, np.float32), np.array([50.0])
    i64, f64, f32 = np.zeros(16, np.int64), np.zeros(16, np.float64), np.zeros(16, np.float32)
    status, total = ctypes.c_int(0), ctypes.c_int64(0)
    step = (_lib.CcStep * 1)()
    calls = {
        'ts2d_label_statistics': lambda: lib.ts2d_label_statistics(0, seg.ctypes.data, 1, vals.ctypes.data, 1, Z, H, W, None, 0, 0, i64.ctypes.data, None, ctypes.byref(status)),
        'ts2d_label_percentiles': lambda: lib.ts2d_label_percentiles(0, seg.ctypes.data, 1, vals.ctypes.data, 1, Z, H, W, x.ctypes.data, 1, q.ctypes.data, 1, 0,
                                                                     i64.ctypes.data, f32.ctypes.data, f64.ctypes.data, ctypes.byref(status)),
        'ts2d_keep_largest_components': lambda: lib.ts2d_keep_largest_components(0, seg.ctypes.data, Z, H, W, ctypes.cast(step, ctypes.c_void_p), 1, i64.ctypes.data,
                                                                                 ctypes.byref(status)),
        'ts2d_label_components': lambda: lib.ts2d_label_components(0, seg.ctypes.data, 1, vals.ctypes.data, 1, Z, H, W, 0, 0, None, 0, None, i64.ctypes.data, None, 0,
                                                                   ctypes.byref(total), ctypes.byref(status)),
        'ts2d_label_overlap': lambda: lib.ts2d_label_overlap(0, seg.ctypes.data, 1, seg.ctypes.data, 1, vals.ctypes.data, 1, Z, H, W, i64.ctypes.data),
        'ts2d_volume_surface_distances': lambda: _raw_distances('ts2d_volume_surface_distances', (Z, H, W), (1, 1, 1)),
    }
    return {name: (call(), _lib.last_error()) for name, call in calls.items()}


def test_h_one_past_every_fence_is_refused_by_name_before_anything_is_allocated():
    before = _free()
    lib = _lib.load()
    for Z, H, W in ((2048, 1024, 1024), (65536, 32768, 1), (65536, 32768, 2 ** 31 - 1), (32767, 32767, 3)):
        assert Z * H * W > 2 ** 31 - 1
        for name, (rc, msg) in _raw_volume_entries(Z, H, W).items():
            assert rc == -1 and name in msg and f'{Z} x {H} x {W}' in msg, (name, rc, msg)
            assert ('2^31 - 1' in msg) or (name == 'ts2d_volume_surface_distances' and 'outside 1 ... 32767' in msg), (name, msg)
    # the projections: nz * nx * num = 2^31 planes bytes; nz * nx = 2^31 pixels.  A one-element buffer and zero strides make the view valid
    one, o8, st = np.ones(1, np.uint8), np.zeros(4, np.uint8), np.zeros(1, np.int32)
    assert lib.ts2d_project_labels_coronal(0, one.ctypes.data, 1, 1, 32768, 1, 32768, 0, 0, 0, 0, 2, o8.ctypes.data, st.ctypes.data) == -1
    assert 'more than 2^31 - 1 bytes' in _lib.last_error() and 'ts2d_project_labels_coronal' in _lib.last_error()
    f4 = np.zeros(4, np.float32)
    assert lib.ts2d_project_coronal(0, one.ctypes.data, 1, 1, 65536, 1, 32768, 0, 0, 0, 0, f4.ctypes.data, f4.ctypes.data) == -1
    assert 'more than 2^31 - 1 pixels' in _lib.last_error() and 'ts2d_project_coronal' in _lib.last_error()
    assert _nothing_held(before)
    # a good small call of every entry follows
    for name, (rc, msg) in _raw_volume_entries(1, 1, 1).items():
        assert rc == 0, (name, msg)
    assert lib.ts2d_project_labels_coronal(0, one.ctypes.data, 1, 1, 1, 1, 1, 0, 0, 0, 0, 2, o8.ctypes.data, st.ctypes.data) == 0 and o8[0] == 1
    assert lib.ts2d_project_coronal(0, one.ctypes.data, 1, 1, 1, 1, 1, 0, 0, 0, 0, f4.ctypes.data, f4.ctypes.data) == 0 and f4[0] == 1.0


def test_h_a_box_of_more_than_2_26_rows_is_refused_by_name():
    """sdv_planes / sdv_rows run one wave per box row: 2^26 rows are 2^32 lanes, which the runtime would cut short.  W < 32 at such a box."""
    shape = (32767, 2049, 1)
    assert shape[0] * shape[1] > 2 ** 26 and _n(shape) < 2 ** 31
    before = _free()
    a, b = np.zeros((1,) + shape, np.uint8), np.zeros((1,) + shape, np.uint8)
    a[0, 0, 0, 0] = b[0, -1, -1, -1] = 1
    with pytest.raises(RuntimeError, match=r'label 0: its box 32767 x 2049 x 1 has 67139583 rows, above the 67108863 rows one launch takes'):
        E._device_volume_distances(a, E.PLANES, b, E.PLANES, None, shape, SPACING, TOL, QS, True, 0, 1 << 34)
    assert _nothing_held(before)
    # 32767 x 2048 = 2^26 - 2048 rows are served.  One voxel a side: each is its side's border, and the definition's d2 is the one candidate
    # ((dz * sz) * (dz * sz) + (dy * sy) * (dy * sy)) + (0 * sx) * (0 * sx) in float64 (evaluate.plane_distance, d2_from_planes) - the statement itself
    # takes the host 13 s at this extent
    b[0, -1, -1, -1], b[0, -1, 2047, 0] = 0, 1
    got = E._device_volume_distances(a, E.PLANES, b, E.PLANES, None, shape, SPACING, TOL, QS, True, 0, 1 << 34)
    rz, ry = np.float64(32766) * np.float64(SPACING[0]), np.float64(2047) * np.float64(SPACING[1])
    d2 = (rz * rz + ry * ry) + np.float64(0.0)
    assert got['border'].tolist() == [[1, 1]] and got['within'].tolist() == [[[0, 0], [0, 0]]] and got['d2_max'].tobytes() == np.array([[d2, d2]]).tobytes()
    assert got['d2_rank'].tobytes() == np.full((1, 2, len(QS), 2), d2).tobytes() and not got['rank_weight'].any()
    assert got['dist_sum'].tobytes() == np.array([[np.sqrt(d2), np.sqrt(d2)]]).tobytes()          # one term: the tree adds +0.0 to it


# ------------------------------------------------------------------------------------------------------------------ part 4: long chains
def _chain_cases():
    line_z, line_y = np.ones((100000, 1, 1), np.uint8), np.ones((1, 100000, 1), np.uint8)
    s = U.serpentine(4, 256, 256)
    assert s.sum() > 2 ** 16
    return {'(100000, 1, 1)': line_z, '(1, 100000, 1)': line_y, 'serpentine (4, 256, 256)': s}


@pytest.mark.parametrize('name', list(_chain_cases()))
def test_long_chains_end_in_the_statement_or_in_give_up_with_every_output_untouched(name):
    """cc_find has no path compression and a cap of 2^15 steps: a one-voxel line of more voxels than that may or may not reach it, depending on the order
    in which its links land.  Either outcome is legal; the module docstring records which one the MI355X gave."""
    seg = _chain_cases()[name] * 5
    shape = seg.shape
    lib = _lib.load()
    with L.Clock(f'chain {name}') as c:
        plan = postprocess.PostprocessingPlan([([5], 0)])
        want_seg, want_stats = postprocess.keep_largest_components_statement(seg, plan)
        out, stats, status = seg.copy(), np.full((1, 4), -77, np.int64), ctypes.c_int(-77)
        step = (_lib.CcStep * 1)()
        ctypes.memmove(step[0].member, plan.compiled[0][0].ctypes.data, 256)
        step[0].background = 0
        assert lib.ts2d_keep_largest_components(0, out.ctypes.data, *shape, ctypes.cast(step, ctypes.c_void_p), 1, stats.ctypes.data, ctypes.byref(status)) == 0
        statuses = [status.value]
        assert status.value in (0, _lib.CC_GIVE_UP)
        if status.value == 0:
            assert np.array_equal(out, want_seg) and np.array_equal(stats, want_stats) and stats[0].tolist() == [int(seg.astype(bool).sum()), 1, int(seg.astype(bool).sum()), 0]
        else:
            assert np.array_equal(out, seg) and (stats == -77).all()
        got = postprocess.apply_postprocessing(seg, plan, device=0)
        assert np.array_equal(got[0], want_seg) and np.array_equal(got[1], want_stats) and got[2] == ('device' if status.value == 0 else 'host')
        for conn in C.CONNECTIVITIES:
            want = C.label_components_statement(seg, [5], conn, True, None)
            vals = np.array([5], np.uint8)
            o, ctr, rows = np.full_like(seg, 99), np.full((1, 5), -77, np.int64), np.full((8, 3), -77, np.int64)
            total, st = ctypes.c_int64(-77), ctypes.c_int(-77)
            assert lib.ts2d_label_components(0, seg.ctypes.data, 1, vals.ctypes.data, 1, *shape, C.CONNECTIVITIES.index(conn), 1, None, 0, o.ctypes.data,
                                             ctr.ctypes.data, rows.ctypes.data, 8, ctypes.byref(total), ctypes.byref(st)) == 0
            statuses.append(st.value)
            assert st.value in (0, _lib.COMP_GIVE_UP)
            if st.value == 0:
                assert np.array_equal(o, want[0]) and np.array_equal(ctr, want[1]) and total.value == len(want[2]) == 1
                assert np.array_equal(rows[:1], want[2]) and (rows[1:] == -77).all()
            else:
                assert (o == 99).all() and (ctr == -77).all() and (rows == -77).all() and total.value == -77
            img = nrrd.Image(seg, (1.0, 1.0, 1.0), (0.0,) * 3, tuple(float(v) for v in np.eye(3).reshape(-1)), 1, {}, None)
            image.set_annotation_meta(img, {5: 'line'}, {})
            assert C.label_components(img, device=0, connectivity=conn) == C.label_components(img, connectivity=conn)
            assert C.label_components(img, device=0, connectivity=conn)['line']['components'] == 1
        c.result = f'status keep_largest / components full / faces: {statuses}'
