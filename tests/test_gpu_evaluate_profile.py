"""ts2d_surface_distance_profile (csrc/kernels_evaluate_profile.h) against evaluate.distance_profile_statement, bit for bit and without a
tolerance anywhere: the sum of the distances in the fixed tree, the order statistics at the percentiles and their weights, the outputs it shares
with ts2d_surface_distances, the label chunks, the refusals, the device's square root against np.sqrt on the values the distances take, and the
device route of evaluate() and of TS2D.Result.evaluate with percentiles and average distances."""
import itertools
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, engine, evaluate as E, nrrd
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu
A = os.path.join(GOLDEN, 'assets')
QS = (0, 5, 50, 95, 97.5, 100)
QS8 = (0, 5, 50, 95, 97.5, 100, 33.3, 99.9)
FIELDS = ('border', 'within', 'd2_max', 'dist_sum', 'd2_rank', 'rank_weight')


def _blobs(rng, H, W, n=3):
    """a mask of a few discs and boxes, some of which touch the image edge"""
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(2, min(H, W) // 2 + 1))
        m |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r) if rng.random() < 0.6 else ((abs(yy - cy) <= r) & (abs(xx - cx) <= r // 2 + 1))
    return m


def _surface_sides(rng, K, H, W):
    """planes and label maps of K labels: blobs; label K empty on both sides, K - 1 in A, K - 2 in B (where K allows); label 1 touches the edge"""
    values = [int(v) for v in rng.permutation(np.arange(1, 256))[:K]]
    pa = np.stack([_blobs(rng, H, W) for _ in range(K)])
    pb = np.stack([np.roll(pa[k], (rng.integers(-2, 3), rng.integers(-2, 3)), (0, 1)) | (_blobs(rng, H, W, 1) & (rng.random() < 0.3)) for k in range(K)])
    pa[0, 0, :] = True
    pb[0, :, W - 1] = True
    if K > 1:
        pa[K - 1], pb[K - 1] = False, False
    if K > 3:
        pa[K - 2], pb[K - 3] = False, False
    la, lb = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    for k in range(K):                                                      # the maps: later labels paint over earlier ones
        la[pa[k]], lb[pb[k]] = values[k], values[k]
    return {E.PLANES: ((pa * rng.integers(1, 256, pa.shape)).astype(np.uint8), pb.astype(np.uint8)), E.LABELMAP: (la, lb)}, values


def _seed(H, W, K):
    return 3050 + 100 * H + W + K


def _assert_profile(got, want, what):
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        assert got[f].tobytes() == want[f].tobytes(), (what, f)              # bit for bit, the float64 ones included


def case_bites(want) -> bool:
    """Does the statement's own output exercise the selection?  A (label, direction) with n >= 3 and 0 < t < 1; one whose two selected d2
    differ; one with a tie at the selected rank (d2 at i equals d2 at j with j > i, or two percentiles select one value); an infinite and a
    -inf entry (one side empty; both empty)."""
    n, t, r = want['border'], want['rank_weight'], want['d2_rank']
    finite = np.isfinite(r[..., 0]) & np.isfinite(r[..., 1])
    inner = (n[:, :, None] >= 3) & (t > 0) & (t < 1)
    return bool(inner.any() and (finite & (r[..., 0] != r[..., 1])).any() and (finite & inner & (r[..., 0] == r[..., 1])).any()
                and np.isposinf(r).any() and np.isneginf(r).any())


@pytest.mark.parametrize('H,W', [(1, 1), (1, 70), (37, 1), (16, 16), (37, 70), (70, 130)])
@pytest.mark.parametrize('K', [1, 18])
def test_profile_equals_the_statement(H, W, K):
    rng = np.random.default_rng(_seed(H, W, K))
    sides, values = _surface_sides(rng, K, H, W)
    spacing = (2.5, 0.8)
    tol = [0.0, spacing[1], 3.0]                                            # the tie: a neighbour one column away lies at exactly spacing_w
    for kind_a, kind_b in itertools.product((E.PLANES, E.LABELMAP), repeat=2):
        a, b = sides[kind_a][0], sides[kind_b][1]
        want = E.distance_profile_statement(a, kind_a, b, kind_b, values, spacing, tol, QS)
        if K == 18 and min(H, W) >= 37 and (kind_a, kind_b) == (E.PLANES, E.PLANES):
            assert case_bites(want)
        got = E._device_profile(a, kind_a, b, kind_b, values, (H, W), spacing, tol, QS, True, 0)
        _assert_profile(got, want, (kind_a, kind_b))
        old = E._device_surface(a, kind_a, b, kind_b, values, (H, W), spacing, tol, 0)
        for f in old:                                                       # what the two entries share: byte for byte
            assert got[f].tobytes() == old[f].tobytes(), (kind_a, kind_b, f)
    a, b = sides[E.PLANES][0], sides[E.LABELMAP][1]                         # the last pair again, piecewise: P = 8; the sum alone; the ranks alone
    want8 = E.distance_profile_statement(a, E.PLANES, b, E.LABELMAP, values, (1.0, 1.0), [], QS8)
    _assert_profile(E._device_profile(a, E.PLANES, b, E.LABELMAP, values, (H, W), (1.0, 1.0), [], QS8, True, 0), want8, 'P = 8')
    only_sum = E._device_profile(a, E.PLANES, b, E.LABELMAP, values, (H, W), (1.0, 1.0), [], [], True, 0)
    assert only_sum['dist_sum'].tobytes() == want8['dist_sum'].tobytes() and only_sum['d2_rank'].shape == (K, 2, 0, 2)
    only_ranks = E._device_profile(a, E.PLANES, b, E.LABELMAP, values, (H, W), (1.0, 1.0), [], QS8, False, 0)
    assert 'dist_sum' not in only_ranks and only_ranks['d2_rank'].tobytes() == want8['d2_rank'].tobytes()
    assert only_ranks['rank_weight'].tobytes() == want8['rank_weight'].tobytes()


def test_the_result_does_not_depend_on_the_chunks():
    rng = np.random.default_rng(3060)
    K, H, W = 255, 9, 11
    sides, values = _surface_sides(rng, K, H, W)
    a, b = sides[E.PLANES][0], sides[E.LABELMAP][1]
    want = E.distance_profile_statement(a, E.PLANES, b, E.LABELMAP, values, (2.5, 0.8), [1.0], QS)
    whole = E._device_profile(a, E.PLANES, b, E.LABELMAP, values, (H, W), (2.5, 0.8), [1.0], QS, True, 0)
    _assert_profile(whole, want, 'one chunk')
    one = engine.surface_profile_scratch_per_label((H, W), len(QS), True)
    assert one == 22 * H * W + 4096 * len(QS) + 16 * H
    for labels in (1, 100):                                                 # 255 chunks of one label; 100, 100, 55
        part = E._device_profile(a, E.PLANES, b, E.LABELMAP, values, (H, W), (2.5, 0.8), [1.0], QS, True, 0, max_scratch_bytes=one * labels + one - 1)
        _assert_profile(part, want, ('chunks', labels))
    with pytest.raises(RuntimeError, match='ONE label'):
        E._device_profile(a, E.PLANES, b, E.LABELMAP, values, (H, W), (2.5, 0.8), [1.0], QS, True, 0, max_scratch_bytes=one - 1)


def test_refusals_leave_the_outputs_untouched():
    lib = _lib.load()
    a = np.zeros((1, 5, 9), np.uint8); b = np.zeros((1, 5, 9), np.uint8)
    a[0, 2, 3], b[0, 2, 4] = 1, 1
    oi = np.full((1, 2, 2), -77, np.int64); of = np.full((1, 2), -77.5)
    osum = np.full((1, 2), -77.5); orank = np.full((1, 2, 8, 2), -77.5); ow = np.full((1, 2, 8), -77.5)
    t2 = np.array([4.0], np.float64); neg = np.array([-1.0], np.float64)
    qs = np.array([95.0, 50.0], np.float64)
    pa, pb, pt, pq = a.ctypes.data, b.ctypes.data, t2.ctypes.data, qs.ctypes.data
    outs = (oi.ctypes.data, of.ctypes.data, osum.ctypes.data, orank.ctypes.data, ow.ctypes.data)

    def bad_q(v):
        return np.array([95.0, v], np.float64)
    keep = [bad_q(v) for v in (-0.5, 100.5, float('nan'), float('inf'))]
    cases = [
        # what ts2d_surface_distances refuses
        ((pa, 0, pb, 0, None, 1, 5, 40000, 1.0, 1.0, pt, 1, pq, 2, 1, 0), outs), ((pa, 0, pb, 0, None, 1, 5, 9, 0.0, 1.0, pt, 1, pq, 2, 1, 0), outs),
        ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, float('nan'), pt, 1, pq, 2, 1, 0), outs), ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, neg.ctypes.data, 1, pq, 2, 1, 0), outs),
        ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 9, pq, 2, 1, 0), outs), ((pa, 1, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, pq, 2, 1, 0), outs),
        ((pa, 0, pb, 0, None, 256, 5, 9, 1.0, 1.0, pt, 1, pq, 2, 1, 0), outs), ((None, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, pq, 2, 1, 0), outs),
        ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, pq, 2, 1, 6 * 45 - 1), outs),
        # P outside 0 ... 8, percentiles missing
        ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, pq, 9, 1, 0), outs), ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, pq, -1, 1, 0), outs),
        ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, None, 2, 1, 0), outs),
        # a null output that is asked for
        ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, pq, 2, 1, 0), outs[:2] + (None,) + outs[3:]),
        ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, pq, 2, 1, 0), outs[:3] + (None, outs[4])),
        ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, pq, 2, 1, 0), outs[:4] + (None,)),
        ((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, pq, 2, 1, 0), (None,) + outs[1:]),
    ]
    cases += [((pa, 0, pb, 0, None, 1, 5, 9, 1.0, 1.0, pt, 1, q.ctypes.data, 2, 1, 0), outs) for q in keep]      # a percentile outside 0 ... 100 or not finite
    for args, out in cases:
        assert lib.ts2d_surface_distance_profile(0, *args, *out) != 0, args
        assert 'ts2d_surface_distance_profile' in _lib.last_error()
        assert (oi == -77).all() and all((x == -77.5).all() for x in (of, osum, orank, ow)), args
    # ... and outputs that are not asked for may be null
    assert lib.ts2d_surface_distance_profile(0, pa, 0, pb, 0, None, 1, 5, 9, 2.5, 0.8, pt, 1, None, 0, 0, 0, oi.ctypes.data, of.ctypes.data, None, None, None) == 0
    old = E._device_surface(a, E.PLANES, b, E.PLANES, None, (5, 9), (2.5, 0.8), [2.0], 0)
    assert np.array_equal(oi[:, :, 0], old['border']) and np.array_equal(oi[:, :, 1:], old['within']) and of.tobytes() == old['d2_max'].tobytes()
    assert (osum == -77.5).all() and (orank == -77.5).all() and (ow == -77.5).all()


def test_the_root_is_numpys():
    """The device's sd_sqrt against np.sqrt, every bit, on d2 = (g sy)^2 + (dx sx)^2 for g, dx = 0 ... 40 and four spacings: a one-pixel mask on
    either side prescribes the distance, and the sum of a one-term tree is that root.  The sweep covers the structured values the distances of
    this feature take (6 724 of them), not all doubles."""
    N = 41
    pairs = [(g, dx) for g in range(N) for dx in range(N)]
    spacings = ((1.0, 1.0), (2.5, 0.8), (0.7, 1.3), (0.9765625, 3.3))
    checked = 0
    for k0 in range(0, len(pairs), 255):                                    # the cases travel as the labels of one call
        part = pairs[k0:k0 + 255]
        a = np.zeros((len(part), N, N), np.uint8)
        b = np.zeros((len(part), N, N), np.uint8)
        a[:, 0, 0] = 1
        for k, (g, dx) in enumerate(part):
            b[k, g, dx] = 1
        g, dx = np.array(part, np.float64).T
        for sy, sx in spacings:
            _, _, sums, _, _ = engine.surface_distance_profile(a, E.PLANES, b, E.PLANES, None, (N, N), (sy, sx), [], [], True, 0, 0)
            ry, rx = g * np.float64(sy), dx * np.float64(sx)
            want = np.sqrt(ry * ry + rx * rx)
            assert sums[:, 0].tobytes() == want.tobytes() and sums[:, 1].tobytes() == want.tobytes(), (k0, sy, sx)
            checked += len(part)
    assert checked == 4 * N * N


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('multilabel_pred,multilabel_ref,dim3', [(True, True, True), (True, False, False), (False, True, True), (False, False, False)])
def test_evaluate_on_the_device_equals_the_host_route(multilabel_pred, multilabel_ref, dim3, monkeypatch):
    rng = np.random.default_rng(3070)
    H, W, K = 37, 70, 5
    sides, drawn = _surface_sides(rng, K, H, W)
    remap = np.zeros(256, np.uint8)
    remap[drawn] = np.arange(1, K + 1)                                      # label k of the maps gets the value k + 1
    spatial, sp = ((H, 1, W), (0.8, 2.0, 2.5)) if dim3 else ((H, W), (0.8, 2.5))
    nd = len(spatial)

    def make(which, multi):
        if multi:
            arr = np.ascontiguousarray(np.moveaxis(sides[E.PLANES][which].reshape((K,) + spatial), 0, -1))
        else:
            arr = remap[sides[E.LABELMAP][which]].reshape(spatial)
        return nrrd.Image(arr, sp, (0.0,) * nd, tuple(np.eye(nd).reshape(-1)), K if multi else 1, {}, None)
    pred, ref = make(0, multilabel_pred), make(1, multilabel_ref)
    pred.meta = {k: v for i in range(K) for k, v in ((f'Segment{i}_ID', str(i)), (f'Segment{i}_Name', f'l{i + 1}'),
                                                      (f'Segment{i}_LabelValue', '1' if multilabel_pred else str(i + 1)),
                                                      (f'Segment{i}_Layer', str(i) if multilabel_pred else '0'))}
    calls = []
    for name in ('label_overlap', 'surface_distances', 'surface_distance_profile'):
        orig = getattr(engine, name)
        monkeypatch.setattr(engine, name, lambda *a, _o=orig, _n=name, **kw: (calls.append(_n), _o(*a, **kw))[1])
    dev = E.evaluate(pred, ref, device=0, tolerances=(1.0, 2.5), percentiles=(95,), average_distance=True)
    assert calls == ['label_overlap', 'surface_distance_profile']           # ONE call for the distance part, the old entry not a second time
    host = E.evaluate(pred, ref, device=None, tolerances=(1.0, 2.5), percentiles=(95,), average_distance=True)
    assert len(calls) == 2 and dev == host and len(dev) == K
    assert any(e['hausdorff_percentile']['95.0'] not in (None, float('inf')) for e in dev.values())
    assert any(e['assd'] not in (None, float('inf')) for e in dev.values()) and any(e['masd'] is None for e in dev.values())
    plain = E.evaluate(pred, ref, device=0, tolerances=(1.0, 2.5))         # the defaults: the calls and the dict of before
    assert calls[2:] == ['label_overlap', 'surface_distances']
    assert all({k: v for k, v in e.items() if k in plain[n]} == plain[n] and len(e) == len(plain[n]) + 5 for n, e in dev.items())


def test_result_evaluate_on_the_device_equals_the_host_route(tmp_path, monkeypatch):
    ids = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_ribs')
    models = {m: synthetic_model(m, 3 + i, 31 + i, patch=(64, 64), mirror=False)[0] for i, m in enumerate(ids)}
    case = nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))
    rng = np.random.default_rng(3080)
    lab = np.zeros(case.array.shape, np.int16)
    for v in range(1, 7):                                                   # label 7 stays absent
        lo = [int(rng.integers(0, s // 2)) for s in lab.shape]
        lab[tuple(slice(o, o + int(rng.integers(3, s // 2))) for o, s in zip(lo, lab.shape))] = v
    vol = nrrd.Image(lab, case.spacing, case.origin, case.direction, 1, {}, case.space)
    calls = []
    for name in ('project_labels_coronal', 'label_overlap', 'surface_distances', 'surface_distance_profile'):
        orig = getattr(engine, name)
        monkeypatch.setattr(engine, name, lambda *a, _o=orig, _n=name, **kw: (calls.append(_n), _o(*a, **kw))[1])
    with TS2D(models=models) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device == 0
        dev = res.evaluate(vol, percentiles=(95, 50), average_distance=True)
        dev_files = res.save_evaluation(str(tmp_path / 'dev'), 'case', vol, percentiles=(95, 50), average_distance=True)
        assert calls == ['project_labels_coronal', 'label_overlap', 'surface_distance_profile'] * 2
        res.device = None
        host = res.evaluate(vol, percentiles=(95, 50), average_distance=True)
        host_files = res.save_evaluation(str(tmp_path / 'host'), 'case', vol, percentiles=(95, 50), average_distance=True)
        assert len(calls) == 6 and dev == host and len(dev) == 7
        assert all(list(e['hausdorff_percentile']) == ['95.0', '50.0'] and 'assd' in e for e in dev.values())
        assert any(e['assd'] not in (None, float('inf')) for e in dev.values())
        with open(dev_files[0], 'rb') as fa, open(host_files[0], 'rb') as fb:
            assert fa.read() == fb.read()
