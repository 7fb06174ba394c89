"""ts2d_volume_surface_distances (csrc/kernels_evaluate_volume.h) against evaluate.volume_surface_statement and
evaluate.volume_distance_profile_statement, bit for bit and without a tolerance anywhere: border counts, counts within the tolerances, the float64
bits of the largest squared distance, of the sum in the fixed tree, of the order statistics and of their weights; the boxes, the label chunks,
the refusals, the device route of evaluate(volume_distances=True), and the 2-D entries that share the row walk."""
import itertools

import numpy as np
import pytest

from totalsegmentator2d_amd import _lib, engine, evaluate as E, nrrd

pytestmark = pytest.mark.gpu
QS8 = (0, 5, 50, 95, 97.5, 100, 33.3, 99.9)
FIELDS = ('border', 'within', 'd2_max', 'dist_sum', 'd2_rank', 'rank_weight')
ANISO, ISO = (2.5, 0.8, 1.3), (1.0, 1.0, 1.0)


def _blobs(rng, shape, n=3):
    """a mask of a few balls and boxes, some of which touch the faces of the volume"""
    grid = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    m = np.zeros(shape, bool)
    for _ in range(n):
        c = [int(rng.integers(0, s)) for s in shape]
        r = int(rng.integers(1, max(2, max(shape) // 3 + 1)))
        if rng.random() < 0.5:
            m |= sum((g - ci) ** 2 for g, ci in zip(grid, c)) <= r * r
        else:
            m |= np.logical_and.reduce([abs(g - ci) <= r // (1 + i) for i, (g, ci) in enumerate(zip(grid, c))])
    return m


def _sides(rng, K, shape):
    """planes and label maps of K labels with values that are not 1 ... K.  Label 1: blobs and two opposite corner voxels on side a, so its box
    touches every face of the volume.  Label 2 (K >= 4): side a in one corner, side b in the opposite one - the joint box is the volume.  Label
    K - 1 (K >= 3) is absent on side b, label K (K >= 2) on both sides."""
    values = [int(v) for v in rng.permutation(np.arange(K + 1, 256))[:K]]
    pa = np.stack([_blobs(rng, shape) for _ in range(K)])
    pb = np.stack([np.roll(pa[k], tuple(int(v) for v in rng.integers(-1, 2, 3)), (0, 1, 2)) | (_blobs(rng, shape, 1) & (rng.random() < 0.4)) for k in range(K)])
    pa[0][0, 0, 0] = pa[0][-1, -1, -1] = True
    if K >= 4:
        pa[1], pb[1] = False, False
        pa[1][:max(1, shape[0] // 3), :max(1, shape[1] // 3), :max(1, shape[2] // 3)] = True
        pb[1][-max(1, shape[0] // 3):, -max(1, shape[1] // 3):, -max(1, shape[2] // 3):] = True
    if K >= 3:
        pb[K - 2] = False
    if K >= 2:
        pa[K - 1], pb[K - 1] = False, False
    la, lb = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for k in range(K):                                                      # the maps: later labels paint over earlier ones
        la[pa[k]], lb[pb[k]] = values[k], values[k]
    return {E.PLANES: ((pa * rng.integers(1, 256, pa.shape)).astype(np.uint8), pb.astype(np.uint8)), E.LABELMAP: (la, lb)}, values


def _assert_same(got, want, what, fields=FIELDS):
    for f in fields:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        assert got[f].tobytes() == want[f].tobytes(), (what, f, got[f], want[f])          # bit for bit, the float64 ones included


def _device(a, kind_a, b, kind_b, values, shape, spacing, tol, qs, want_sum, scratch=0):
    return E._device_volume_distances(a, kind_a, b, kind_b, values, shape, spacing, tol, qs, want_sum, 0, scratch)


# (5, 9, 70) and (3, 66, 7): a row and a y' range across a wave's 64; (67, 4, 5): a z line longer than 64, and more than 64 rows for the tree
@pytest.mark.parametrize('shape,K', [((5, 9, 70), 5), ((3, 66, 7), 5), ((67, 4, 5), 3), ((1, 6, 6), 1), ((2, 2, 2), 1)])
def test_the_entry_equals_the_statements(shape, K):
    rng = np.random.default_rng(3400 + 100 * shape[0] + shape[1] + K)
    sides, values = _sides(rng, K, shape)
    tol2 = [0.8, 3.0]                                                       # the tie: a neighbour one row away lies at exactly spacing_h
    for kind_a, kind_b in itertools.product((E.PLANES, E.LABELMAP), repeat=2):
        a, b = sides[kind_a][0], sides[kind_b][1]
        want = E.volume_distance_profile_statement(a, kind_a, b, kind_b, values, ANISO, tol2, QS8)
        _assert_same(_device(a, kind_a, b, kind_b, values, shape, ANISO, tol2, QS8, True), want, (kind_a, kind_b))
        _assert_same(_device(a, kind_a, b, kind_b, values, shape, ANISO, tol2, None, False), want, ('plain', kind_a, kind_b), FIELDS[:3])
    a, b = sides[E.PLANES][0], sides[E.LABELMAP][1]                         # unit spacing: many ties; T = 0 and 8, P = 0 and 1, the sum on and off
    tol8 = [0.0, 1.0, 1.5, 2.0, 2.5, 3.0, 5.0, 100.0]
    want = E.volume_distance_profile_statement(a, E.PLANES, b, E.LABELMAP, values, ISO, tol8, [95])
    _assert_same(_device(a, E.PLANES, b, E.LABELMAP, values, shape, ISO, tol8, [95], True), want, 'T = 8, P = 1')
    only_ranks = _device(a, E.PLANES, b, E.LABELMAP, values, shape, ISO, [], [95], False)
    assert 'dist_sum' not in only_ranks and only_ranks['within'].shape == (K, 2, 0)
    _assert_same(only_ranks, want, 'the ranks alone', ('border', 'd2_max', 'd2_rank', 'rank_weight'))
    only_sum = _device(a, E.PLANES, b, E.LABELMAP, values, shape, ISO, [], [], True)
    assert only_sum['d2_rank'].shape == (K, 2, 0, 2)
    _assert_same(only_sum, want, 'the sum alone', ('border', 'd2_max', 'dist_sum'))
    if K >= 3:                                                              # the cases the sides promise
        assert want['border'][K - 1].tolist() == [0, 0] and (want['d2_max'][K - 1] == -np.inf).all()
        assert want['border'][K - 2, 1] == 0 and want['d2_max'][K - 2, 0] == np.inf and want['dist_sum'][K - 2, 0] == np.inf


def test_a_box_off_the_lanes_of_the_tree():
    """A label whose box starts at x = 65 and at row 7 of a (3, 5, 140) volume: the sum's lanes are those of the FULL extent.  And one across
    x = 64 ... 130, whose rows take two chunks of 64 that start inside the box's first."""
    shape = (3, 5, 140)
    a, b = np.zeros((2,) + shape, np.uint8), np.zeros((2,) + shape, np.uint8)
    rng = np.random.default_rng(3401)
    a[0, 1:3, 2:5, 65:100] = rng.random((2, 3, 35)) < 0.6
    b[0, 1:3, 2:4, 70:101] = rng.random((2, 2, 31)) < 0.6
    a[0, 1, 2, 65] = 1                                                      # the box's first corner, whatever the draw
    a[1, 0:3, 1:4, 63:131] = rng.random((3, 3, 68)) < 0.7
    b[1, 0:2, 0:4, 64:120] = rng.random((2, 4, 56)) < 0.7
    for spacing in (ANISO, ISO):
        want = E.volume_distance_profile_statement(a, E.PLANES, b, E.PLANES, None, spacing, [1.0], [0, 50, 95, 100])
        assert want['border'].min() > 3 and np.isfinite(want['dist_sum']).all()
        _assert_same(_device(a, E.PLANES, b, E.PLANES, None, shape, spacing, [1.0], [0, 50, 95, 100], True), want, spacing)


def test_the_result_does_not_depend_on_the_chunks():
    rng = np.random.default_rng(3402)
    K, shape = 5, (4, 7, 9)
    sides, values = _sides(rng, K, shape)
    a, b = sides[E.PLANES][0].copy(), sides[E.LABELMAP][1]
    a[:K - 1, 0, 0, 0] = a[:K - 1, -1, -1, -1] = 1                          # every label but the absent one has the volume as its box
    qs = [50, 95]
    want = E.volume_distance_profile_statement(a, E.PLANES, b, E.LABELMAP, values, ANISO, [1.0], qs)
    one = engine.volume_scratch_per_label(shape, len(qs), True)
    assert one == 38 * 4 * 7 * 9 + 16 * 4 * 7
    for labels in (4, 2, 1):                                                # the four labels with a box in 1, 2 and 4 chunks
        got = _device(a, E.PLANES, b, E.LABELMAP, values, shape, ANISO, [1.0], qs, True, scratch=one * labels + one - 1)
        _assert_same(got, want, ('chunks of', labels))
    _assert_same(_device(a, E.PLANES, b, E.LABELMAP, values, shape, ANISO, [1.0], qs, True), want, 'the default bound')
    plain_one = engine.volume_scratch_per_label(shape, 0, False)
    assert plain_one == 22 * 4 * 7 * 9
    _assert_same(_device(a, E.PLANES, b, E.LABELMAP, values, shape, ANISO, [1.0], None, False, scratch=plain_one), want, 'plain, one by one', FIELDS[:3])
    # a bound below one label: refused by name, the outputs untouched
    lib = _lib.load()
    oi = np.full((K, 2, 2), -77, np.int64); of = np.full((K, 2), -77.5)
    osum = np.full((K, 2), -77.5); orank = np.full((K, 2, 2, 2), -77.5); ow = np.full((K, 2, 2), -77.5)
    t2, q2, vals = np.array([1.0]), np.array(qs, np.float64), np.array(values, np.uint8)
    rc = lib.ts2d_volume_surface_distances(0, a.ctypes.data, 0, b.ctypes.data, 1, vals.ctypes.data, K, *shape, *ANISO, t2.ctypes.data, 1, q2.ctypes.data, 2,
                                           1, one - 1, oi.ctypes.data, of.ctypes.data, osum.ctypes.data, orank.ctypes.data, ow.ctypes.data)
    assert rc == -1 and 'ts2d_volume_surface_distances' in _lib.last_error() and 'ONE label' in _lib.last_error()      # TS2D_ERR_INVALID
    assert (oi == -77).all() and all((x == -77.5).all() for x in (of, osum, orank, ow))
    with pytest.raises(RuntimeError, match='ONE label'):
        _device(a, E.PLANES, b, E.LABELMAP, values, shape, ANISO, [1.0], None, False, scratch=plain_one - 1)


def test_refusals_leave_the_outputs_untouched():
    lib = _lib.load()
    a = np.zeros((1, 3, 5, 9), np.uint8); b = np.zeros((1, 3, 5, 9), np.uint8)
    a[0, 1, 2, 3], b[0, 2, 2, 5] = 1, 1
    oi = np.full((1, 2, 2), -77, np.int64); of = np.full((1, 2), -77.5)
    osum = np.full((1, 2), -77.5); orank = np.full((1, 2, 8, 2), -77.5); ow = np.full((1, 2, 8), -77.5)
    t2 = np.array([4.0], np.float64); neg = np.array([-1.0], np.float64)
    qs = np.array([95.0, 50.0], np.float64); q101 = np.array([95.0, 101.0], np.float64)
    pa, pb, pt, pq = a.ctypes.data, b.ctypes.data, t2.ctypes.data, qs.ctypes.data
    outs = (oi.ctypes.data, of.ctypes.data, osum.ctypes.data, orank.ctypes.data, ow.ctypes.data)
    nan, inf = float('nan'), float('inf')

    def args(pa=pa, pb=pb, kind_a=0, K=1, zhw=(3, 5, 9), sp=(1.0, 1.0, 1.0), pt=pt, T=1, pq=pq, P=2, want_sum=1, scratch=0):
        return (pa, kind_a, pb, 0, None, K, *zhw, *sp, pt, T, pq, P, want_sum, scratch)
    cases = [
        (args(pa=None), outs), (args(pb=None), outs), (args(), (None,) + outs[1:]), (args(), (outs[0], None) + outs[2:]),      # a null pointer
        (args(), outs[:2] + (None,) + outs[3:]), (args(), outs[:3] + (None, outs[4])), (args(), outs[:4] + (None,)),
        (args(pq=None), outs), (args(pt=None), outs),
        (args(zhw=(0, 5, 9)), outs), (args(zhw=(3, 0, 9)), outs), (args(zhw=(3, 5, 0)), outs),                                # an extent 0
        (args(zhw=(40000, 5, 9)), outs), (args(zhw=(3, 40000, 9)), outs), (args(zhw=(3, 5, 40000)), outs),                    # ... above the limit
        (args(zhw=(2000, 2000, 2000)), outs),                                                                                 # Z * H * W above 2^31 - 1
        (args(sp=(0.0, 1.0, 1.0)), outs), (args(sp=(1.0, inf, 1.0)), outs), (args(sp=(1.0, 1.0, nan)), outs),                  # the spacing
        (args(sp=(-1.0, 1.0, 1.0)), outs),
        (args(pt=neg.ctypes.data), outs), (args(T=9), outs), (args(T=-1), outs),                                              # the tolerances
        (args(pq=q101.ctypes.data), outs), (args(P=9), outs), (args(P=-1), outs),                                             # the percentiles
        (args(kind_a=2), outs), (args(kind_a=1), outs), (args(K=0), outs), (args(K=256), outs),                               # kinds, values, K
    ]
    for call, out in cases:
        assert lib.ts2d_volume_surface_distances(0, *call, *out) == -1, call                                                  # TS2D_ERR_INVALID
        assert 'ts2d_volume_surface_distances' in _lib.last_error()
        assert (oi == -77).all() and all((x == -77.5).all() for x in (of, osum, orank, ow)), call
    # the plain form: the outputs that are not asked for may be null
    assert lib.ts2d_volume_surface_distances(0, *args(sp=ANISO, pq=None, P=0, want_sum=0), outs[0], outs[1], None, None, None) == 0
    want = E.volume_surface_statement(a, E.PLANES, b, E.PLANES, None, ANISO, [2.0])
    assert np.array_equal(oi[:, :, 0], want['border']) and np.array_equal(oi[:, :, 1:], want['within']) and of.tobytes() == want['d2_max'].tobytes()
    d2 = (np.float64(1) * 2.5) * (np.float64(1) * 2.5) + (np.float64(0) * 0.8) * (np.float64(0) * 0.8) + (np.float64(2) * 1.3) * (np.float64(2) * 1.3)
    assert of.tolist() == [[d2, d2]] and (osum == -77.5).all() and (orank == -77.5).all() and (ow == -77.5).all()


def _volume_pair(multilabel_pred, multilabel_ref, shape, K, seed):
    rng = np.random.default_rng(seed)
    sides, drawn = _sides(rng, K, shape)
    remap = np.zeros(256, np.uint8)
    remap[drawn] = np.arange(1, K + 1)                                      # label k of the maps gets the value k + 1

    def make(which, multi):
        arr = np.ascontiguousarray(np.moveaxis(sides[E.PLANES][which], 0, -1)) if multi else remap[sides[E.LABELMAP][which]]
        return nrrd.Image(arr, (1.3, 0.8, 2.5), (0.0,) * 3, tuple(np.eye(3).reshape(-1)), K if multi else 1, {}, None)
    pred, ref = make(0, multilabel_pred), make(1, multilabel_ref)
    pred.meta = {k: v for i in range(K) for k, v in ((f'Segment{i}_ID', str(i)), (f'Segment{i}_Name', f'l{i + 1}'),
                                                      (f'Segment{i}_LabelValue', '1' if multilabel_pred else str(i + 1)),
                                                      (f'Segment{i}_Layer', str(i) if multilabel_pred else '0'))}
    return pred, ref


@pytest.mark.parametrize('multilabel_pred,multilabel_ref', [(True, True), (True, False), (False, True), (False, False)])
def test_evaluate_on_the_device_equals_the_host_route(multilabel_pred, multilabel_ref, monkeypatch):
    K = 5
    pred, ref = _volume_pair(multilabel_pred, multilabel_ref, (5, 9, 70), K, 3403)
    calls = []
    for name in ('label_overlap', 'surface_distances', 'surface_distance_profile', 'volume_surface_distances'):
        orig = getattr(engine, name)
        monkeypatch.setattr(engine, name, lambda *a, _o=orig, _n=name, **kw: (calls.append(_n), _o(*a, **kw))[1])
    dev = E.evaluate(pred, ref, device=0, tolerances=(1.0, 2.5), percentiles=(95,), average_distance=True, volume_distances=True)
    assert calls == ['label_overlap', 'volume_surface_distances']           # ONE call for the distance part
    host = E.evaluate(pred, ref, device=None, tolerances=(1.0, 2.5), percentiles=(95,), average_distance=True, volume_distances=True)
    assert len(calls) == 2 and dev == host and len(dev) == K
    assert any(e['hausdorff_percentile']['95.0'] not in (None, float('inf')) for e in dev.values())
    assert any(e['assd'] not in (None, float('inf')) for e in dev.values()) and any(e['masd'] is None for e in dev.values())
    assert dev['l5']['hausdorff'] is None and dev['l4']['hausdorff'] == float('inf')
    plain_dev = E.evaluate(pred, ref, device=0, tolerances=(1.0, 2.5), volume_distances=True)
    assert plain_dev == E.evaluate(pred, ref, device=None, tolerances=(1.0, 2.5), volume_distances=True)
    without = E.evaluate(pred, ref, device=0)
    assert all(set(e) - set(without[n]) == {'surface_dice', 'hausdorff'} for n, e in plain_dev.items())
    assert calls[2:] == ['label_overlap', 'volume_surface_distances', 'label_overlap']


def test_the_2d_entries_still_equal_their_statements():
    """The sanity line for the row walk the 2-D kernels now share with the volume's: one 2-D case, both entries (tests/test_gpu_evaluate.py and
    tests/test_gpu_evaluate_profile.py remain the yardstick)."""
    rng = np.random.default_rng(3404)
    H, W, K = 37, 70, 3
    pa = np.stack([_blobs(rng, (H, W)) for _ in range(K)]).astype(np.uint8)
    pb = np.stack([np.roll(p, (1, -2), (0, 1)) for p in pa]).astype(np.uint8)
    pb[K - 1] = 0
    want = E.distance_profile_statement(pa, E.PLANES, pb, E.PLANES, None, (2.5, 0.8), [0.8, 3.0], QS8)
    _assert_same(E._device_profile(pa, E.PLANES, pb, E.PLANES, None, (H, W), (2.5, 0.8), [0.8, 3.0], QS8, True, 0), want, 'profile')
    _assert_same(E._device_surface(pa, E.PLANES, pb, E.PLANES, None, (H, W), (2.5, 0.8), [0.8, 3.0], 0), want, 'plain', FIELDS[:3])
