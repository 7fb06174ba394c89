"""What tests/test_gpu_large_volumes.py relies on, proven on the host at moderate size (tests/large_volume_util.py has the argument):

  * the TWIN relation of every statement the large cases compare against - statistics, percentiles, components (both entries' statements), overlap,
    volume distances and their profile: the statement of a volume with two islands equals the statement of its twin, integers shifted as
    ``large_volume_util`` shifts them, the float64 fields bit for bit where the removed rows are a multiple of 64 - and that this condition is
    needed: with other row counts the float sums of seeded cases change their bits;
  * the boxed distance statement equals ``evaluate``'s statements bit for bit, in 2-D and 3-D, crops and offsets included;
  * the planners at their caps: ``ls_plan`` and ``st_plan`` (csrc/stats_plan.cpp) through the stand-alone driver of
    tests/test_statistics_percentiles_cpu.py, and ``engine.statistics_chunk_labels`` / ``engine.percentiles_chunk_labels`` against them.
"""
import subprocess

import numpy as np
import pytest

from tests import large_volume_util as L
from tests.test_statistics_percentiles_cpu import driver          # noqa: F401  (the fixture: label_select_driver.cpp + stats_plan.cpp, sanitized)
from totalsegmentator2d_amd import components as C, engine, evaluate as E, postprocess, statistics as S

SHAPE, WINDOW, KEEP = (40, 64, 70), (3, 30, 40), (8, 8)          # 24 slabs of 64 rows are removed: a multiple of 64
VALUES = [7, 200, 41]


def _pair(shape=SHAPE, window=WINDOW, keep=KEEP, seed=0, near=VALUES, far=None, integers_only=False):
    big = L.two_islands(shape, window, seed, near, far)
    assert L.middle_is_empty(big, *keep) and big[-1, -1, -1] != 0
    twin, removed = L.twin_of(big, *keep, integers_only=integers_only)
    return big, twin, removed


def _intensities(shape, C_, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(C_,) + tuple(shape)) * rng.choice([1e-3, 1.0, 1e4], size=(C_,) + tuple(shape))).astype(np.float32)


def _cut(x, keep, axis):
    return L.twin_of(x, *keep, axis=axis, integers_only=True)[0]


@pytest.mark.parametrize('kind', ['labelmap', 'planes'])
def test_statistics_and_percentiles_of_the_twin_are_those_of_the_volume(kind):
    big, twin, removed = _pair()
    x = _intensities(SHAPE, 2, 1)
    xt = _cut(x, KEEP, 1)
    if kind == 'planes':
        big, twin, values = np.stack([(big == v) * 3 for v in VALUES]).astype(np.uint8), np.stack([(twin == v) * 3 for v in VALUES]).astype(np.uint8), None
    else:
        values = VALUES + [99]                                                           # an absent label
    want = S.label_statistics_statement(big, x, (1, 1, 1), values)
    got = L.shifted_statistics(S.label_statistics_statement(twin, xt, (1, 1, 1), values), twin, values, KEEP[0], removed, SHAPE[0])
    assert L.same_dict(got, want, L.STATISTICS_FIELDS), {f: (got[f], want[f]) for f in L.STATISTICS_FIELDS if not L.same_dict(got, want, (f,))}
    assert want['count'][:3].min() > 100 and want['bbox_max'][:3, 0].max() == SHAPE[0] - 1
    qs = (0, 5, 50, 95, 100)
    assert L.same_dict(S.label_percentiles_statement(twin, xt, qs, values), S.label_percentiles_statement(big, x, qs, values), L.PERCENTILE_FIELDS)


def test_the_float_sums_need_the_removed_rows_to_be_a_multiple_of_64():
    """H = 50: 32 removed slabs are 1600 = 25 * 64 rows and every sum keeps its bits; 23 removed slabs are 1150 rows, the surviving far rows change
    their lanes, and float sums change their bits in at least one of the seeded cases (all of them here) - while the integers still hold."""
    differ = 0
    for seed in range(4):
        for removed_slabs, holds in ((32, True), (23, False)):
            shape, keep = (6 + 6 + removed_slabs, 50, 70), (6, 6)
            big, twin, removed = _pair(shape, (3, 30, 40), keep, seed, integers_only=True)
            assert removed == removed_slabs and (removed * 50 % 64 == 0) == holds
            x = _intensities(shape, 1, 10 + seed)
            want = S.label_statistics_statement(big, x, (1, 1, 1), VALUES)
            got = L.shifted_statistics(S.label_statistics_statement(twin, _cut(x, keep, 1), (1, 1, 1), VALUES), twin, VALUES, keep[0], removed, shape[0])
            assert L.same_dict(got, want, ('count', 'index_sum', 'bbox_min', 'bbox_max', 'min', 'max'))
            if holds:
                assert L.same_dict(got, want, L.STATISTICS_FIELDS)
            else:
                differ += not L.same_dict(got, want, ('sum', 'ssq'))
                assert np.allclose(got['sum'], want['sum'], rtol=1e-9) and np.allclose(got['ssq'], want['ssq'], rtol=1e-9)
    assert differ >= 1


@pytest.mark.parametrize('conn', C.CONNECTIVITIES)
def test_components_of_the_twin_are_those_of_the_volume_with_the_far_roots_shifted(conn):
    big, twin, removed = _pair(seed=3)
    n_slab = SHAPE[1] * SHAPE[2]
    for rule in (dict(), dict(keep_largest=True, min_voxels=[2, 3, 2])):
        want = C.label_components_statement(big, VALUES, conn, **rule)
        got = C.label_components_statement(twin, VALUES, conn, **rule)
        assert np.array_equal(got[1], want[1])
        assert np.array_equal(L.shifted_components(got[2], KEEP[0] * n_slab, removed * n_slab), want[2])
        assert np.array_equal(_cut(want[0], KEEP, 0), got[0]) and L.middle_is_empty(want[0], *KEEP)
        assert (want[2][:, 1] >= (SHAPE[0] - KEEP[1]) * n_slab).any() and (want[2][:, 1] < KEEP[0] * n_slab).any()
    plan = [([7, 200], 0), ([41], 9)]
    want, got = postprocess.keep_largest_components_statement(big, plan), postprocess.keep_largest_components_statement(twin, plan)
    assert np.array_equal(got[1], want[1]) and np.array_equal(_cut(want[0], KEEP, 0), got[0]) and want[1][:, 3].min() > 0
    assert int(np.count_nonzero(want[0][KEEP[0]:SHAPE[0] - KEEP[1]])) == 0


def test_overlap_and_volume_distances_of_the_twin_are_those_of_the_volume():
    """Labels 7 and 200 live in the near island only, 41 and 9 in the far one only: no distance crosses the removed slabs."""
    values = [7, 200, 41, 9]
    a = L.two_islands(SHAPE, (3, 10, 40), 5, [7, 200], [41, 9])
    b = L.two_islands(SHAPE, (3, 10, 40), 6, [7, 200], [41, 9])
    at, removed = L.twin_of(a, *KEEP)
    bt, _ = L.twin_of(b, *KEEP)
    for f, v in E.overlap_statement(a, E.LABELMAP, b, E.LABELMAP, values).items():
        assert np.array_equal(v, E.overlap_statement(at, E.LABELMAP, bt, E.LABELMAP, values)[f]) and v.min() > 0
    spacing, tol, qs = (2.5, 0.8, 1.3), [0.8, 3.0], (0, 50, 95, 100)
    want = E.volume_distance_profile_statement(a, E.LABELMAP, b, E.LABELMAP, values, spacing, tol, qs)
    got = E.volume_distance_profile_statement(at, E.LABELMAP, bt, E.LABELMAP, values, spacing, tol, qs)
    assert L.same_dict(got, want, L.DISTANCE_FIELDS) and want['border'].min() > 10 and np.isfinite(want['dist_sum']).all()
    # ... and the boxed statement: the far labels from their crop at its place in the full extent, the near ones from theirs
    Z, H, W = SHAPE
    for lab, crop, origin in (((2, 3), (slice(Z - 4, Z), slice(H - 12, H), slice(W - 45, W)), (Z - 4, H - 12, W - 45)),
                              ((0, 1), (slice(0, 5), slice(0, 11), slice(0, 64)), (0, 0, 0))):
        boxed = L.boxed_distance_statement(a[crop], E.LABELMAP, b[crop], E.LABELMAP, values, spacing, tol, qs, origin, SHAPE)
        for f in L.DISTANCE_FIELDS:
            assert boxed[f][list(lab)].tobytes() == want[f][list(lab)].tobytes(), (f, lab)


@pytest.mark.parametrize('shape', [(5, 9, 70), (3, 66, 7), (67, 4, 5), (1, 6, 6), (9, 70), (66, 7)])
def test_the_boxed_distance_statement_is_the_statement(shape):
    rng = np.random.default_rng(sum(shape))
    K = 3
    pa = (rng.random((K,) + shape) < 0.3).astype(np.uint8)
    pb = (rng.random((K,) + shape) < 0.3).astype(np.uint8) * 200
    pb[1] = 0                                                                            # a side without a border: +inf
    pa[2], pb[2] = 0, 0                                                                  # an absent label
    values = None
    spacing = (2.5, 0.8, 1.3)[3 - len(shape):]
    statement = E.volume_distance_profile_statement if len(shape) == 3 else E.distance_profile_statement
    for sp in (spacing, (1.0,) * len(shape)):
        want = statement(pa, E.PLANES, pb, E.PLANES, values, sp, [0.0, 1.0, 2.5], (0, 5, 50, 97.5, 100))
        got = L.boxed_distance_statement(pa, E.PLANES, pb, E.PLANES, values, sp, [0.0, 1.0, 2.5], (0, 5, 50, 97.5, 100))
        assert L.same_dict(got, want, L.DISTANCE_FIELDS), {f: (got[f], want[f]) for f in L.DISTANCE_FIELDS if not L.same_dict(got, want, (f,))}
    assert want['d2_max'][1, 0] == np.inf and want['border'][2].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------------ the planners at their caps
def _lines(driver, mode, tmp_path, text):                                                # noqa: F811
    path = tmp_path / f'{mode}.txt'
    path.write_text(text)
    return subprocess.run([driver, mode, str(path)], check=True, capture_output=True, text=True).stdout.split('\n')[:-1]


def test_ls_plan_at_the_slot_cap(driver, tmp_path):                                      # noqa: F811
    huge = 1 << 46
    queries = [(255, 1, 8, 2 ** 23 + 1, huge), (255, 1, 8, 2 ** 23, huge), (255, 1, 8, 4097 * 2048, huge), (255, 64, 8, 2 ** 31 - 1, huge),
               (255, 1, 1, 2 ** 30, huge), (255, 1, 1, 2 ** 30 + 1, huge), (200, 1, 8, 2 ** 23 + 1, 0)]
    out = _lines(driver, 'plan', tmp_path, ''.join('%d %d %d %d %d\n' % q for q in queries))
    sizes = []
    for line, (K, Cn, P, rows, bound) in zip(out, queries):
        f = line.split()
        chunks = [tuple(int(v) for v in c.split(':')) for c in f[3:]]
        assert int(f[0]) == 0 and chunks[0][0] == 0 and chunks[-1][1] == K and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        sizes.append([k1 - k0 for k0, k1 in chunks])
        cap, by = engine.percentiles_chunk_labels((rows, 1, 1), K, Cn, P, bound)
        assert sizes[-1][0] == cap and all(s == cap for s in sizes[-1][:-1]) and sizes[-1][0] * rows <= 2 ** 31 - 1
        assert by == ('budget' if bound == 0 else 'slot_cap')
    assert sizes[0] == [255] and sizes[1] == [255] and sizes[2] == [255]                 # (2^31 - 1) // (2^23 + 1) = 255: the cap, and all K labels
    assert sizes[3] == [1] * 255                                                         # rows = 2^31 - 1: one label at a time
    assert sizes[4] == [1] * 255 and sizes[5] == [1] * 255                               # (2^31 - 1) // 2^30 = 1
    assert sizes[6][0] == (256 << 20) // (2 * 8 * 1040 + (2 ** 23 + 1) * 20) == 1        # the default budget decides long before the cap


def test_st_plan_is_the_arithmetic_the_entry_had_inline(driver, tmp_path):               # noqa: F811
    queries = []
    for K in (1, 3, 255):
        for Cn in (0, 1, 2, 64):
            for rows in (1, 337, 512 * 512, 2 ** 23 + 1, 2 ** 25, 2 ** 26, 2 ** 31 - 1):
                per = rows * (20 + 16 * Cn)
                for bound in (0, per - 1, per, 2 * per + 1, K * per, 127 * per, 128 * per, 1 << 46):
                    queries.append((K, Cn, rows, bound))
    out = _lines(driver, 'chunk', tmp_path, ''.join('%d %d %d %d\n' % q for q in queries))
    assert len(out) == len(queries)
    seen = set()
    for line, (K, Cn, rows, bound) in zip(out, queries):
        rc, labels, need, budget = (int(v) for v in line.split())
        per = rows * (20 + 16 * Cn)
        b = bound or 256 << 20
        by_budget, slot_cap = min(b // per, K), (2 ** 31 - 1) // (rows * max(Cn, 1))      # stats.hip before the move: labels_per_chunk, then the slot cap
        assert need == per and budget == b
        if by_budget < 1:
            assert (rc, labels) == (-1, 0)
        elif slot_cap < 1:
            assert (rc, labels) == (-2, 0)
        else:
            assert (rc, labels) == (0, min(by_budget, slot_cap)) and labels * rows * max(Cn, 1) <= 2 ** 31 - 1
        got, by = engine.statistics_chunk_labels((rows, 1, 1), K, Cn, bound)
        assert got == (labels if rc == 0 else min(b // per, slot_cap, K)), (K, Cn, rows, bound)
        seen.add((rc, by))
    assert {(0, 'budget'), (0, 'slot_cap'), (0, 'labels'), (-1, 'budget'), (-2, 'slot_cap')} <= seen
    # the case of tests/test_gpu_large_volumes.py: 512 x 512 x 2, K = 255, C = 64 - the cap of 127 decides once the budget allows 128 labels
    per = 512 * 512 * (20 + 16 * 64)
    assert engine.statistics_chunk_labels((512, 512, 2), 255, 64, 128 * per) == (127, 'slot_cap')
    assert engine.statistics_chunk_labels((512, 512, 2), 255, 64, 127 * per - 1) == (126, 'budget')
    assert engine.statistics_chunk_labels((512, 512, 2), 255, 64, 0) == (0, 'budget')   # the default 256 MiB hold no label of 273 MB
