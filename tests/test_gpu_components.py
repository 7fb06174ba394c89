"""The components of every label at once on the MI355X: the entry ts2d_label_components (csrc/kernels_components.h) against the numpy/scipy
statement ``components.label_components_statement`` - the cleaned array, all five counters and the sorted list, byte for byte, no tolerance
anywhere -, its chunks, list capacities and refusals, the wrappers, and the old entry ts2d_keep_largest_components run label by label.
TS2D_COMP_GIVE_UP is never observed on these inputs (none is built to reach a cap)."""
import ctypes
import os

import numpy as np
import pytest

from tests import components_util as U
from tests.conftest import GOLDEN
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, engine, image, nrrd
from totalsegmentator2d_amd import components as C
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu
A = os.path.join(GOLDEN, 'assets')
EXTENTS = [(1, 9, 70), (1, 66, 7), (3, 5, 130), (2, 2, 2), (1, 1, 64), (1, 7, 1), (3, 70, 65)]
RULES = (dict(), dict(keep_largest=True), dict(min_voxels=2), dict(keep_largest=True, min_voxels=3))
_wanted = {}


def check(seg, values, conn='full', keep_largest=False, min_voxels=None, max_scratch_bytes=0, must_remove=False):
    """The entry on `seg`: the statement's bytes (computed once per input and rule); the input is left alone.  Returns the device's triple."""
    seg = np.ascontiguousarray(seg, np.uint8)
    K = seg.shape[0] if values is None else len(values)
    if isinstance(min_voxels, int):
        min_voxels = [min_voxels] * K
    spatial = seg.shape[1:] if values is None else seg.shape
    key = (seg.tobytes(), seg.shape, None if values is None else tuple(values), conn, keep_largest, None if min_voxels is None else tuple(min_voxels))
    if key not in _wanted:
        _wanted[key] = C.label_components_statement(seg, values, conn, keep_largest, min_voxels)
    want = _wanted[key]
    before = seg.copy()
    got = engine.label_components(seg, _lib.STATS_PLANES if values is None else _lib.STATS_LABELMAP, values, ((1,) + tuple(spatial))[-3:],
                                  C.CONNECTIVITIES.index(conn), keep_largest, min_voxels, max_scratch_bytes=max_scratch_bytes, device=0)
    assert got is not None, 'TS2D_COMP_GIVE_UP'
    print(f'{seg.shape} K={K} {conn} keep={keep_largest} min={min_voxels}: components {int(got[1][:, 1].sum())} removed {int(got[1][:, 4].sum())}')
    assert np.array_equal(got[1], want[1]), (got[1].tolist(), want[1].tolist())
    assert np.array_equal(got[2], want[2]), (got[2].tolist()[:10], want[2].tolist()[:10])
    assert np.array_equal(got[0], want[0]), int((got[0] != want[0]).sum())
    assert U.same(got, want) and np.array_equal(seg, before)
    if must_remove:
        assert got[1][:, 3].sum() > 0
    return got


def test_the_entry_is_there():
    assert engine.has_entry('ts2d_label_components') and 'ts2d_label_components' in _lib.OPTIONAL


@pytest.mark.parametrize('extent', EXTENTS)
def test_random_speckle_of_both_kinds_on_every_extent(extent):
    rng = np.random.default_rng(sum(extent))
    for j, density in enumerate((0.15, 0.45, 0.85)):
        for kind in ('planes', 'labelmap'):
            K = (1, 3, 5)[(j + (kind == 'planes')) % 3]
            for spatial in ((extent,) if extent[0] > 1 else (extent, extent[1:])):          # Z = 1 also as a 2-D array
                seg, values = U.random_case(rng, kind, spatial, K, density)
                for r, rule in enumerate(RULES):
                    check(seg, values, ('full', 'faces')[(j + r) % 2], **rule)
                check(seg, values, ('faces', 'full')[j % 2], keep_largest=True, min_voxels=[int(v) for v in rng.integers(0, 5, K)])


@pytest.mark.parametrize('K', [117, 255])
def test_many_labels(K):
    rng = np.random.default_rng(K)
    values = [int(v) for v in rng.permutation(np.arange(1, 256))[:K]]
    lm = np.where(rng.random((1, 9, 70)) < 0.9, np.asarray(values, np.uint8)[rng.integers(0, K, (1, 9, 70))], 0).astype(np.uint8)
    lm[0, 4, 10:30] = values[K - 1]
    got = check(lm, values, 'full', keep_largest=True)
    assert got[1][K - 1, 2] >= 20
    check(lm, values, 'faces', min_voxels=2)
    planes, _ = U.random_case(rng, 'planes', (1, 9, 70), K, 0.4)
    check(planes, None, 'full', keep_largest=True, must_remove=True)
    check(planes, None, 'faces', keep_largest=True, min_voxels=3)


def test_checkerboard_serpentine_rings_and_the_degenerate_maps():
    for spatial in ((1, 9, 70), (3, 5, 130), (2, 2, 2)):
        n = int(np.prod(spatial))
        for values in ([9, 4], [200, 3, 17]):
            board = U.checkerboard(spatial, values)
            got = check(board, values, 'faces')
            assert got[1][:, 1].sum() == n and (got[1][:, 2] == 1).all()          # the maximal number: every voxel is a piece
            got = check(board, values, 'full')
            if len(values) == 2:
                assert (got[1][:, 1] == 1).all()          # two colours: every label is one piece through its diagonals
            check(board, values, 'faces', keep_largest=True)          # every piece ties for the largest: all stay
            ring = U.rings(spatial, values)
            check(ring, values, 'full', keep_largest=True)
            check(ring, values, 'faces', min_voxels=9)
    s = U.serpentine(4, 32, 32)
    for conn in C.CONNECTIVITIES:
        got = check(s * 5, [5], conn)
        assert got[1][0, 1] == 1 and got[1][0, 2] == s.sum()          # one corridor
        check(np.stack([s, 1 - s]) * 3, None, conn, keep_largest=True)
    z = np.zeros((3, 5, 130), np.uint8)
    got = check(z, [3, 8], 'full', keep_largest=True, min_voxels=4)
    assert not got[1].any() and got[2].shape == (0, 3)
    check(np.stack([z, z]), None, 'faces')
    full = np.full((3, 5, 130), 8, np.uint8)
    got = check(full, [3, 8], 'full', keep_largest=True)          # a label absent, a label filling everything
    assert got[1].tolist() == [[0] * 5, [1950, 1, 1950, 0, 0]] and got[2].tolist() == [[1, 0, 1950]]
    check(np.stack([z, full]), None, 'faces', min_voxels=1950)


def test_rules_thresholds_and_ties():
    row = np.zeros((1, 3, 200), np.uint8)
    for start, length in ((0, 5), (10, 5), (60, 10), (126, 4), (150, 10), (190, 3)):          # (60, 10) and (126, 4) cross a word end
        row[0, 1, start:start + length] = 6
    row[0, 0, 62:66] = 6          # joins the run below it under both connectivities
    for conn in C.CONNECTIVITIES:
        got = check(row, [6], conn)
        assert got[2][:, 2].tolist() == [14, 10, 5, 5, 4, 3]
        got = check(row, [6], conn, min_voxels=5)          # exactly at the threshold: the two of 5 stay, 4 and 3 go
        assert got[1].tolist() == [[41, 6, 14, 7, 2]]
        check(row, [6], conn, min_voxels=6, must_remove=True)
        got = check(row, [6], conn, keep_largest=True)
        assert got[1].tolist() == [[41, 6, 14, 27, 5]]
        got = check(row, [6], conn, keep_largest=True, min_voxels=15)          # both together: the largest goes too
        assert got[1].tolist() == [[41, 6, 14, 41, 6]] and not got[0].any()
    tie = np.zeros((2, 4, 70), np.uint8)
    tie[0, 0, 60:68] = tie[1, 3, 0:8] = 2
    tie[0, 1, 30:33] = 2
    tie[1, 1, 1:5] = 9
    got = check(tie, [9, 2], 'full', keep_largest=True)          # the two of 8 tie and stay
    assert got[1].tolist() == [[4, 1, 4, 0, 0], [19, 3, 8, 3, 1]]
    check(tie, [9, 2], 'faces', keep_largest=True, min_voxels=[5, 8])          # a per-label vector: 9 loses its only piece, 2 keeps the tie
    check(np.stack([tie == 2, tie == 9]).astype(np.uint8), None, 'full', keep_largest=True, min_voxels=[8, 5])


def test_isolation_between_planes_and_between_labels():
    p = np.zeros((3, 1, 4, 66), np.uint8)
    p[0, 0, 3, 60:] = 1          # ends plane 0 ...
    p[1, 0, 0, :9] = 1           # ... and starts plane 1: two pieces, one per plane
    p[1, 0, 3, :] = 1
    p[2, 0, 0, :] = 1
    for conn in C.CONNECTIVITIES:
        got = check(p, None, conn)
        assert got[1][:, 1].tolist() == [1, 2, 1] and got[2].tolist() == [[0, 258, 6], [1, 198, 66], [1, 0, 9], [2, 0, 66]]
        check(p, None, conn, keep_largest=True, max_scratch_bytes=engine.components_state_bytes((1, 4, 66)))          # one plane per chunk
    lm = np.zeros((1, 8, 70), np.uint8)
    lm[0, 0::2] = 4
    lm[0, 1::2] = 250          # two labels interleaved row by row: every row is a piece of its own
    for conn in C.CONNECTIVITIES:
        got = check(lm, [250, 4], conn, keep_largest=True)
        assert got[1].tolist() == [[280, 4, 70, 0, 0]] * 2


def test_chunks_give_identical_outputs_and_a_bound_below_one_label_is_refused():
    rng = np.random.default_rng(5)
    extent = (3, 5, 130)
    one = engine.components_state_bytes(extent)
    assert one == 9 * 1950 + 8 * 15 * 3
    planes, _ = U.random_case(rng, 'planes', extent, 4, 0.4)
    lm, values = U.random_case(rng, 'labelmap', extent, 4, 0.6)
    for bound in (0, 4 * one, 2 * one + 7, one):          # 1, 1, 2 and 4 chunks
        check(planes, None, 'full', keep_largest=True, min_voxels=2, max_scratch_bytes=bound, must_remove=True)
        check(lm, values, 'faces', keep_largest=True, max_scratch_bytes=bound)          # a label map is one set whatever K is
    for seg, vals in ((planes, None), (lm, values)):
        with pytest.raises(RuntimeError, match='max_scratch_bytes'):
            check(seg, vals, max_scratch_bytes=one - 1)


def _raw(seg, kind, values, K, zhw, conn=0, keep=0, minv=None, bound=0, out_seg=None, counters=None, rows=None, capacity=0, total=None, status=None,
         seg_null=False):
    lib = _lib.load()
    vals = None if values is None else np.asarray(values, np.uint8)
    mv = None if minv is None else np.asarray(minv, np.int64)
    return lib.ts2d_label_components(0, None if seg_null else seg.ctypes.data, kind, None if vals is None else vals.ctypes.data, K, *zhw, conn, keep,
                                     None if mv is None else mv.ctypes.data, bound, None if out_seg is None else out_seg.ctypes.data,
                                     None if counters is None else counters.ctypes.data, None if rows is None else rows.ctypes.data, capacity,
                                     None if total is None else ctypes.byref(total), None if status is None else ctypes.byref(status))


def test_list_capacity_and_the_wrappers_second_call(monkeypatch):
    rng = np.random.default_rng(8)
    seg, values = U.random_case(rng, 'labelmap', (3, 5, 130), 3, 0.5)
    want = C.label_components_statement(seg, values, 'faces', True, None)
    N = len(want[2])
    assert N > 50
    for capacity, rows in ((0, None), (N, np.full((N, 3), -77, np.int64)), (N - 1, np.full((N - 1, 3), -77, np.int64)), (N + 9, np.full((N + 9, 3), -77, np.int64))):
        out, counters = np.full_like(seg, 99), np.full((3, 5), -77, np.int64)
        total, status = ctypes.c_int64(-77), ctypes.c_int(-77)
        assert _raw(seg, 1, values, 3, (3, 5, 130), 1, 1, None, 0, out, counters, rows, capacity, total, status) == 0
        assert status.value == (_lib.COMP_LIST_FULL if capacity < N else 0) and total.value == N
        assert np.array_equal(out, want[0]) and np.array_equal(counters, want[1])          # valid whatever the capacity is
        if rows is not None and capacity < N:
            assert (rows == -77).all()          # the list is untouched
        elif rows is not None:
            assert np.array_equal(rows[:N], want[2]) and (rows[N:] == -77).all()
    # the wrapper: a first capacity that is too small costs exactly one more call, with the exact total
    calls = []
    lib = _lib.load()
    orig = lib.ts2d_label_components

    class Spy:
        def __getattr__(self, name):
            if name != 'ts2d_label_components':
                return getattr(lib, name)
            return lambda *a: (calls.append(int(a[15])), orig(*a))[1]
    monkeypatch.setattr(_lib, '_lib', Spy())
    got = engine.label_components(seg, 1, values, (3, 5, 130), 1, True, None, device=0, capacity=7)
    assert calls == [7, N] and U.same(got, want)
    got = engine.label_components(seg, 1, values, (3, 5, 130), 1, True, None, device=0)
    assert calls == [7, N, engine.COMPONENTS_FIRST_CAPACITY] and U.same(got, want)
    got = engine.label_components(seg, 1, values, (3, 5, 130), 1, True, None, device=0, want_list=False)
    assert calls[-1] == 0 and got[2] is None and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_every_refusal_by_name_leaves_the_outputs_untouched():
    seg = np.ones((2, 3, 4), np.uint8)
    out, counters, rows = np.full_like(seg, 99), np.full((2, 5), -77, np.int64), np.full((4, 3), -77, np.int64)
    total, status = ctypes.c_int64(-77), ctypes.c_int(-77)
    ok = dict(seg=seg, kind=1, values=[1, 2], K=2, zhw=(2, 3, 4), out_seg=out, counters=counters, rows=rows, capacity=4, total=total, status=status)
    bad = [(dict(seg_null=True), 'null'), (dict(counters=None), 'null'), (dict(total=None), 'null'), (dict(status=None), 'null'),
           (dict(kind=2), 'kind'), (dict(conn=2), 'connectivity'), (dict(conn=-1), 'connectivity'), (dict(K=0), 'K = 0'), (dict(K=256), 'K = 256'),
           (dict(zhw=(0, 3, 4)), 'voxels'), (dict(zhw=(2, 3, -4)), 'voxels'), (dict(zhw=(2048, 1024, 1024)), 'voxels'),
           (dict(values=None), 'values'), (dict(values=[1, 0]), 'background'), (dict(values=[5, 5]), 'repeats'),
           (dict(minv=[0, -1]), 'min_voxels'), (dict(capacity=-1), 'capacity'), (dict(rows=None), 'without a list'),
           (dict(bound=100), 'max_scratch_bytes')]
    for change, word in bad:
        assert _raw(**dict(ok, **change)) == -1, change          # TS2D_ERR_INVALID
        assert word in _lib.last_error() and 'ts2d_label_components' in _lib.last_error(), (change, _lib.last_error())
        assert (out == 99).all() and (counters == -77).all() and (rows == -77).all() and total.value == -77 and status.value == -77
    assert _raw(**ok) == 0 and status.value == 0 and total.value == 1 and rows[0].tolist() == [0, 0, 24] and (rows[1:] == -77).all()
    assert counters.tolist() == [[24, 1, 24, 0, 0], [0] * 5] and (out == 1).all()


def _image(multilabel):
    rng = np.random.default_rng(12)
    if multilabel:
        planes = np.ascontiguousarray((rng.random((3, 40, 70)) < 0.45).astype(np.uint8) * 255)
        seg = nrrd.Image(np.moveaxis(planes, 0, -1), (0.8, 2.5), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 3, {}, None)
        image.set_annotation_meta(seg, {1: 'a', 2: 'b', 3: 'c'}, {})
    else:
        arr = (rng.integers(0, 4, (4, 20, 70)) * 3).astype(np.uint8)
        seg = nrrd.Image(arr, (1.5, 0.8, 0.8), (0.0,) * 3, tuple(float(v) for v in np.eye(3).reshape(-1)), 1, {}, None)
        image.set_annotation_meta(seg, {3: 'three', 6: 'six', 9: 'nine'}, {})
    return seg


def test_the_image_wrappers_on_the_device_equal_the_host_route(monkeypatch):
    calls = []
    orig = engine.label_components
    monkeypatch.setattr(engine, 'label_components', lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    for multilabel in (True, False):
        seg = _image(multilabel)
        before = seg.array.tobytes()
        mm = float(np.prod(seg.spacing))
        for conn in C.CONNECTIVITIES:
            n = len(calls)
            dev = C.label_components(seg, device=0, connectivity=conn)
            dev_clean, dev_ctr = C.clean_components(seg, device=0, connectivity=conn, keep_largest=True, min_size_mm=2.5 * mm)
            assert len(calls) == n + 2
            host = C.label_components(seg, connectivity=conn)
            host_clean, host_ctr = C.clean_components(seg, connectivity=conn, keep_largest=True, min_size_mm=2.5 * mm)
            assert len(calls) == n + 2          # the host route made none
            assert dev == host and dev_ctr == host_ctr and any(c['voxels_removed'] for c in dev_ctr.values())
            assert dev_clean.array.tobytes() == host_clean.array.tobytes() and dev_clean.array.shape == seg.array.shape
            assert dev_clean.meta == seg.meta and seg.array.tobytes() == before
            assert C.clean_components(seg, device=0, connectivity=conn)[0].array.tobytes() == before


def test_result_components_and_cleaned_on_the_device_equal_the_host_route(tmp_path):
    ids = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_ribs')
    models = {m: synthetic_model(m, 3 + i, 31 + i, patch=(64, 64), mirror=False)[0] for i, m in enumerate(ids)}
    with TS2D(models=models) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device == 0
        before = res.get_segmentation().array.tobytes()
        dev = res.components()
        dev_clean = res.cleaned(keep_largest=True, min_size_mm=4.0)
        dev_files = res.save_components(str(tmp_path / 'dev'), 'case', models='all', connectivity='faces')
        assert res.cleaned().get_segmentation().array.tobytes() == before and dev_clean.device == 0
        res.device = None
        host = res.components()
        host_clean = res.cleaned(keep_largest=True, min_size_mm=4.0)
        host_files = res.save_components(str(tmp_path / 'host'), 'case', models='all', connectivity='faces')
        assert dev == host and len(dev) == 7 and any(e['components'] > 1 for e in dev.values())
        for m in [None] + list(ids):
            assert dev_clean.get_segmentation(m).array.tobytes() == host_clean.get_segmentation(m).array.tobytes()
        assert dev_clean.get_segmentation().array.tobytes() != before and res.get_segmentation().array.tobytes() == before
        assert [os.path.basename(f) for f in dev_files] == ['case.components.json', 'case-cardiac.components.json', 'case-ribs.components.json']
        for a, b in zip(dev_files, host_files):
            with open(a, 'rb') as fa, open(b, 'rb') as fb:
                assert fa.read() == fb.read()


def test_the_old_entry_label_by_label_gives_the_new_entrys_bytes():
    rng = np.random.default_rng(21)
    seg, values = U.random_case(rng, 'labelmap', (3, 70, 65), 5, 0.55)
    new = check(seg, values, 'full', keep_largest=True, must_remove=True)
    tables = np.zeros((5, 256), np.uint8)
    tables[np.arange(5), values] = 1
    old, stats, status = engine.keep_largest_components(seg, tables, np.zeros(5, np.uint8), device=0)          # one single-label step per label
    assert status == 0 and old.tobytes() == new[0].tobytes()
    assert np.array_equal(stats, new[1][:, :4])          # voxels, components, largest, voxels removed: the same four counters
