"""ts2d_project_labels_coronal, ts2d_label_overlap and ts2d_surface_distances (csrc/kernels_evaluate.h) against their statements in
totalsegmentator2d_amd/evaluate.py, byte for byte and bit for bit - the float64 bits of the largest squared distance included -, the range
status, the label chunks, and the device route of evaluate() and of TS2D.Result.evaluate."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, engine, evaluate as E, image, nrrd
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu
A = os.path.join(GOLDEN, 'assets')
EYE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
DTYPES = ('int16', 'uint8', 'uint16', 'int32')


def _direction(perm, signs):
    """image axis ax points along physical axis perm[ax] with sign signs[ax]"""
    D = np.zeros((3, 3))
    for ax in range(3):
        D[perm[ax], ax] = signs[ax]
    return tuple(float(v) for v in D.reshape(-1))


# the six permutations - every view axis gets the unit stride once with the ray and once without -, each axis flipped in two of them
DIRECTIONS = [_direction(p, s) for p, s in zip(itertools.permutations(range(3)),
                                               ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, 1), (-1, -1, -1)))]


def _labels(rng, shape, num, dtype, must=()):
    a = (rng.integers(1, num + 1, shape) * (rng.random(shape) < 0.05)).astype(dtype)
    flat = a.reshape(-1)
    for i, v in enumerate(must):                                            # these labels are present for sure
        flat[(i * 7919) % flat.size] = v
    return a


def _check_projection(vol, num):
    want = E.project_labels(image.reorient_image(vol), num, 'coronal')
    got = E.project_labels_coronal_gpu(vol, num, 0)
    assert got.array.dtype == np.uint8 and got.array.shape == want.array.shape and got.components == want.components
    assert got.array.tobytes() == want.array.tobytes()
    assert got.spacing == want.spacing and np.allclose(got.origin, want.origin) and np.allclose(got.direction, want.direction)
    return got


@pytest.mark.parametrize('dtype', DTYPES)
def test_projection_equals_the_statement(dtype):
    rng = np.random.default_rng(2900 + DTYPES.index(dtype))
    vol = nrrd.Image(_labels(rng, (5, 7, 9), 3, dtype, (1, 2, 3)), (1.0, 2.0, 3.0), (5.0, -7.0, 11.0), EYE, 1, {}, None)
    _check_projection(vol, 3)
    for num in (117, 255):                                                  # the bit set crosses the 32-, 64- and 96-bit words
        if num > np.iinfo(dtype).max:
            continue
        must = (1, 32, 33, 64, 65, 96, 97, num)
        a = _labels(rng, (33, 70, 65), num, dtype, must)
        got = _check_projection(nrrd.Image(a, (1.0, 2.0, 3.0), (5.0, -7.0, 11.0), EYE, 1, {}, None), num)
        assert all(got.array[..., v - 1].any() for v in must) and got.array.shape == (33, 1, 65, num)
    for num in (32, 33, 64, 65, 128, 129):                                  # where the number of words changes
        if num <= np.iinfo(dtype).max:
            _check_projection(nrrd.Image(_labels(rng, (4, 5, 6), num, dtype, (1, num)), (1.0, 2.0, 3.0), (0.0, 0.0, 0.0), EYE, 1, {}, None), num)


@pytest.mark.parametrize('direction', DIRECTIONS)
def test_projection_through_every_view(direction):
    rng = np.random.default_rng(2910 + DIRECTIONS.index(direction))
    for shape in ((6, 10, 13), (8, 3, 12)):                                 # nz * nx: odd sizes (byte stores) and multiples of 4 (packed stores)
        for dtype in ('int16', 'uint8'):
            vol = nrrd.Image(_labels(rng, shape, 40, dtype, (1, 40)), (1.0, 2.0, 3.0), (5.0, -7.0, 11.0), direction, 1, {}, None)
            _check_projection(vol, 40)


def test_projection_edges_and_the_range_status():
    rng = np.random.default_rng(2920)
    for shape in ((5, 1, 9), (1, 4, 1), (3, 6, 67), (2, 6, 130), (1, 300, 2)):      # ny = 1; one pixel; an odd nx (the scalar tail); a packed nx
        _check_projection(nrrd.Image(_labels(rng, shape, 9, 'int16', (9,)), (1.0, 2.0, 3.0), (0.0, 0.0, 0.0), EYE, 1, {}, None), 9)
    _check_projection(nrrd.Image(np.zeros((4, 5, 6), np.uint8), (1.0, 2.0, 3.0), (0.0, 0.0, 0.0), EYE, 1, {}, None), 1)
    for bad in (4, -1, 30000):
        a = _labels(rng, (5, 7, 9), 3, 'int16')
        a[3, 4, 5] = bad
        vol = nrrd.Image(a, (1.0, 2.0, 3.0), (0.0, 0.0, 0.0), EYE, 1, {}, None)
        with pytest.raises(ValueError, match='outside 0 ... 3'):
            E.project_labels_coronal_gpu(vol, 3, 0)
        planes, status = engine.project_labels_coronal(a, (5, 7, 9), (63, 9, 1), 0, 3, 0)
        assert status == _lib.LABELS_RANGE
    lib = _lib.load()
    a = np.zeros((5, 7, 9), np.float32)
    out = np.full((3, 5, 9), 77, np.uint8)
    status = np.zeros(1, np.int32)
    for dtype, num, n_elems in ((2, 3, a.size), (0, 0, a.size), (0, 256, a.size), (0, 3, a.size - 1)):      # float, num, a view that leaves the buffer
        assert lib.ts2d_project_labels_coronal(0, a.ctypes.data, n_elems, dtype, 5, 7, 9, 63, 9, 1, 0, num, out.ctypes.data, status.ctypes.data) != 0
        assert (out == 77).all() and 'ts2d_project_labels_coronal' in _lib.last_error()


# ------------------------------------------------------------------------------------------------ overlap
def _two_sides(rng, K, spatial):
    """planes and a label map for each side with K distinct values; label K absent on both sides, K - 1 on side b (where K allows)."""
    values = [int(v) for v in rng.permutation(np.arange(1, 256))[:K]]
    pool = np.array([0] + values, np.uint8)
    ia = rng.integers(0, K + 1, spatial)
    ib = np.where(rng.random(spatial) < 0.7, ia, rng.integers(0, K + 1, spatial))
    if K > 1:
        ia[ia == K] = 0
        ib[ib == K] = 0
    if K > 2:
        ib[ib == K - 1] = 0
    la, lb = pool[ia], pool[ib]
    pa = np.stack([(la == v) * rng.integers(1, 256, spatial) for v in values]).astype(np.uint8)      # any value > 0 counts
    pb = np.stack([(lb == v) for v in values]).astype(np.uint8)
    return {E.PLANES: (pa, pb), E.LABELMAP: (la, lb)}, values


@pytest.mark.parametrize('K', [1, 3, 117, 255])
def test_overlap_equals_the_statement(K):
    rng = np.random.default_rng(2930 + K)
    for spatial in ((1, 1, 1), (1, 7, 65), (3, 33, 130), (2, 8, 64)):       # (the last: a multiple of 16 samples, the 16-byte loads)
        sides, values = _two_sides(rng, K, spatial)
        for kind_a, kind_b in itertools.product((E.PLANES, E.LABELMAP), repeat=2):
            a, b = sides[kind_a][0], sides[kind_b][1]
            want = E.overlap_statement(a, kind_a, b, kind_b, values)
            got = E._device_overlap(a, kind_a, b, kind_b, values, spatial, 0)
            for f in want:
                assert got[f].dtype == np.int64 and np.array_equal(got[f], want[f]), (spatial, kind_a, kind_b, f)
        if K == 3 and spatial == (3, 33, 130):                              # a label absent on both sides, and one absent on side b only
            assert want['n_a'][2] == 0 and want['n_b'][2] == 0 and want['n_b'][1] == 0 and want['n_a'][1] > 0 and want['n_both'][0] > 0


def test_overlap_of_full_planes_and_refusals():
    full = np.full((2, 4, 16, 64), 255, np.uint8)
    got = E._device_overlap(full, E.PLANES, np.full((4, 16, 64), 9, np.uint8), E.LABELMAP, [9, 8], (4, 16, 64), 0)
    assert got['n_a'].tolist() == [4096, 4096] and got['n_b'].tolist() == [4096, 0] and got['n_both'].tolist() == [4096, 0]
    lib = _lib.load()
    out = np.full((2, 3), -77, np.int64)
    vals = np.array([9, 0], np.uint8)
    for args in ((full.ctypes.data, 2, full.ctypes.data, 0, None, 2, 4, 16, 64), (full.ctypes.data, 0, full.ctypes.data, 0, None, 256, 4, 16, 64),
                 (full.ctypes.data, 1, full.ctypes.data, 0, None, 2, 4, 16, 64), (full.ctypes.data, 1, full.ctypes.data, 0, vals.ctypes.data, 2, 4, 16, 64),
                 (full.ctypes.data, 0, full.ctypes.data, 0, None, 2, 65536, 65536, 1), (None, 0, full.ctypes.data, 0, None, 2, 4, 16, 64)):
        assert lib.ts2d_label_overlap(0, *args, out.ctypes.data) != 0 and (out == -77).all() and 'ts2d_label_overlap' in _lib.last_error()


# ------------------------------------------------------------------------------------------------ surface distances
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


def _assert_surface(got, want, what):
    assert got['border'].dtype == np.int64 and np.array_equal(got['border'], want['border']), what
    assert got['within'].dtype == np.int64 and np.array_equal(got['within'], want['within']), what
    assert got['d2_max'].dtype == np.float64 and np.array_equal(got['d2_max'].view(np.uint64), want['d2_max'].view(np.uint64)), what


@pytest.mark.parametrize('H,W', [(1, 1), (1, 70), (37, 1), (16, 16), (37, 70)])
@pytest.mark.parametrize('K', [1, 18])
def test_surface_distances_equal_the_statement(H, W, K):
    rng = np.random.default_rng(2950 + 100 * H + W + K)
    sides, values = _surface_sides(rng, K, H, W)
    for spacing in ((1.0, 1.0), (2.5, 0.8)):
        tol = [0.0, spacing[1], 3.0]                                        # the tie: a neighbour one column away lies at exactly spacing_w
        for kind_a, kind_b in itertools.product((E.PLANES, E.LABELMAP), repeat=2):
            a, b = sides[kind_a][0], sides[kind_b][1]
            want = E.surface_statement(a, kind_a, b, kind_b, values, spacing, tol)
            got = E._device_surface(a, kind_a, b, kind_b, values, (H, W), spacing, tol, 0)
            _assert_surface(got, want, (spacing, kind_a, kind_b))
            if K == 18 and (kind_a, kind_b) == (E.PLANES, E.PLANES):
                assert want['border'][K - 1].tolist() == [0, 0] and want['border'][K - 2, 0] == 0 and want['border'][K - 3, 1] == 0
                assert (want['d2_max'][K - 1] == -np.inf).all() and want['d2_max'][0, 0] >= 0
                for labels in (5, 1):                                       # 4 chunks (5, 5, 5, 3); one label at a time
                    part = E._device_surface(a, kind_a, b, kind_b, values, (H, W), spacing, tol, 0, max_scratch_bytes=6 * H * W * labels + 3)
                    _assert_surface(part, want, ('chunks', labels))


def test_surface_tie_and_refusals():
    a = np.zeros((1, 5, 9), np.uint8); b = np.zeros((1, 5, 9), np.uint8)
    a[0, 2, 3], b[0, 2, 4] = 1, 1
    sx = 0.8
    tol = [sx, float(np.nextafter(sx, 0.0))]
    got = E._device_surface(a, E.PLANES, b, E.PLANES, None, (5, 9), (2.5, sx), tol, 0)
    _assert_surface(got, E.surface_statement(a, E.PLANES, b, E.PLANES, None, (2.5, sx), tol), 'tie')
    assert got['within'][0].tolist() == [[1, 0], [1, 0]]
    with pytest.raises(RuntimeError, match='ONE label'):
        E._device_surface(a, E.PLANES, b, E.PLANES, None, (5, 9), (2.5, sx), tol, 0, max_scratch_bytes=6 * 45 - 1)
    lib = _lib.load()
    oi = np.full((1, 2, 2), -77, np.int64); of = np.full((1, 2), -77.5)
    t2 = np.array([4.0], np.float64); neg = np.array([-1.0], np.float64)
    for args in ((a.ctypes.data, 0, b.ctypes.data, 0, None, 1, 5, 40000, 1.0, 1.0, t2.ctypes.data, 1), (a.ctypes.data, 0, b.ctypes.data, 0, None, 1, 5, 9, 0.0, 1.0, t2.ctypes.data, 1),
                 (a.ctypes.data, 0, b.ctypes.data, 0, None, 1, 5, 9, 1.0, float('nan'), t2.ctypes.data, 1), (a.ctypes.data, 0, b.ctypes.data, 0, None, 1, 5, 9, 1.0, 1.0, neg.ctypes.data, 1),
                 (a.ctypes.data, 0, b.ctypes.data, 0, None, 1, 5, 9, 1.0, 1.0, t2.ctypes.data, 9), (a.ctypes.data, 1, b.ctypes.data, 0, None, 1, 5, 9, 1.0, 1.0, t2.ctypes.data, 1)):
        assert lib.ts2d_surface_distances(0, *args, 0, oi.ctypes.data, of.ctypes.data) != 0
        assert (oi == -77).all() and (of == -77.5).all() and 'ts2d_surface_distances' in _lib.last_error()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('multilabel_pred,multilabel_ref,dim3', [(True, True, True), (True, False, False), (False, True, True), (False, False, False)])
def test_evaluate_on_the_device_equals_the_host_route(multilabel_pred, multilabel_ref, dim3, monkeypatch):
    rng = np.random.default_rng(2970)
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
    for name in ('label_overlap', 'surface_distances'):
        orig = getattr(engine, name)
        monkeypatch.setattr(engine, name, lambda *a, _o=orig, _n=name, **kw: (calls.append(_n), _o(*a, **kw))[1])
    dev = E.evaluate(pred, ref, device=0, tolerances=(1.0, 2.5, 4.0))
    assert calls == ['label_overlap', 'surface_distances']
    host = E.evaluate(pred, ref, device=None, tolerances=(1.0, 2.5, 4.0))
    assert calls == ['label_overlap', 'surface_distances'] and dev == host and len(dev) == K
    assert any(e['hausdorff'] not in (None, float('inf')) for e in dev.values()) and any(e['dice'] for e in dev.values())


def test_result_evaluate_on_the_device_equals_the_host_route(tmp_path, monkeypatch):
    ids = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_ribs')
    models = {m: synthetic_model(m, 3 + i, 31 + i, patch=(64, 64), mirror=False)[0] for i, m in enumerate(ids)}
    case = nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))
    rng = np.random.default_rng(2980)
    lab = np.zeros(case.array.shape, np.int16)
    for v in range(1, 7):                                                   # label 7 stays absent
        lo = [int(rng.integers(0, s // 2)) for s in lab.shape]
        lab[tuple(slice(o, o + int(rng.integers(3, s // 2))) for o, s in zip(lo, lab.shape))] = v
    vol = nrrd.Image(lab, case.spacing, case.origin, case.direction, 1, {}, case.space)
    calls = []
    for name in ('project_labels_coronal', 'label_overlap', 'surface_distances'):
        orig = getattr(engine, name)
        monkeypatch.setattr(engine, name, lambda *a, _o=orig, _n=name, **kw: (calls.append(_n), _o(*a, **kw))[1])
    with TS2D(models=models) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device == 0
        seg = res.get_segmentation()
        before = seg.array.tobytes()
        dev = res.evaluate(vol)
        dev_files = res.save_evaluation(str(tmp_path / 'dev'), 'case', vol)
        assert calls == ['project_labels_coronal', 'label_overlap', 'surface_distances'] * 2
        res.device = None
        host = res.evaluate(vol)
        host_files = res.save_evaluation(str(tmp_path / 'host'), 'case', vol)
        assert len(calls) == 6 and dev == host and len(dev) == 7 and any(e['count_both'] > 0 for e in dev.values())
        assert [os.path.basename(f) for f in dev_files] == [os.path.basename(f) for f in host_files] == ['case.evaluation.json']
        with open(dev_files[0], 'rb') as fa, open(host_files[0], 'rb') as fb:
            assert fa.read() == fb.read()
        assert seg.array.tobytes() == before
