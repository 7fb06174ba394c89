"""ts2d_label_confusion (csrc/kernels_confusion.h: the confusion matrix as ONE integer matrix product, v_mfma_i32_32x32x32_i8) against
evaluate.confusion_statement, integer for integer: the tile edges of K, the load and step widths of N, unaligned planes, several sample chunks,
every pairing of kinds in both orders, the bytes a plane may hold, planes past byte 2^32, the refusals, and the device route of
evaluate.confusion and TS2D.Result.confusion.

The inputs have unequal label frequencies on the two sides, and the sweep asserts that the expected matrix is asymmetric with pairwise different
rows and columns: a transposed write of the result tile, a swapped or permuted row, or a dropped tile then changes the matrix - this is the check
of the instruction's lane maps with exact integer data."""
import os

import numpy as np
import pytest

from tests import large_volume_util as L
from tests.confusion_util import PAIRINGS, random_side, stray_byte
from tests.conftest import GOLDEN
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, engine, evaluate as E, nrrd
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu
A = os.path.join(GOLDEN, 'assets')
# the launch constants of csrc/kernels_confusion.h: a wave's chunk has at least 1024 samples, and more where that keeps the launch near 4096 waves
CHUNK_MIN, WAVES_AIM = 1024, 4096
ERR_INVALID = -1                                                            # TS2D_ERR_INVALID of include/ts2d_engine.h


def values_of(rng, K, plain=False):
    return list(range(1, K + 1)) if plain else sorted(int(v) for v in rng.choice(np.arange(1, 256), K, replace=False))


def device(a, kind_a, b, kind_b, values, spatial):
    zhw = (1,) * (3 - len(spatial)) + tuple(spatial)
    got = engine.label_confusion(np.ascontiguousarray(a), kind_a, np.ascontiguousarray(b), kind_b, values, zhw, 0)
    assert got.dtype == np.int64
    return got


def distinct(M) -> bool:
    """asymmetric, rows pairwise different, columns pairwise different"""
    return bool((M != M.T).any()) and len({r.tobytes() for r in M}) == len(M) and len({c.tobytes() for c in M.T}) == len(M)


def sweep_case(rng, K, spatial, kind_a, kind_b):
    values = values_of(rng, K, plain=K == 255)
    return random_side(rng, kind_a, K, spatial, values, present=True), random_side(rng, kind_b, K, spatial, values, present=True), values


# ------------------------------------------------------------------------------------------------ the kernels against the statement
@pytest.mark.parametrize('K', [1, 30, 31, 62, 63, 117, 254, 255])          # K + 2 rows: 3, 32 | 33, 64 | 65, 119, 256 | 257
def test_every_tile_edge_of_K(K):
    rng = np.random.default_rng(3700 + K)
    for spatial in ((3, 17, 33), (2, 64, 64)):                             # 1683 samples: N % 16 = 3, every plane k >= 1 unaligned; 8192: aligned
        for kind_a, kind_b in PAIRINGS:                                     # (planes, map) and (map, planes): each side as a and as b
            a, b, values = sweep_case(rng, K, spatial, kind_a, kind_b)
            want = E.confusion_statement(a, kind_a, b, kind_b, values)
            # two label maps put every sample into ONE cell: with fewer than 64 samples a label, rows of one or two samples coincide, and
            # only the asymmetry is asked of the input; every pairing with a planes side must have pairwise different rows and columns
            if K > 1 and (E.PLANES in (kind_a, kind_b) or int(np.prod(spatial)) >= 64 * K):
                assert distinct(want), (K, spatial, kind_a, kind_b)
            else:
                assert (want != want.T).any()
            assert np.array_equal(device(a, kind_a, b, kind_b, values, spatial), want), (K, spatial, kind_a, kind_b)


@pytest.mark.parametrize('N', [1, 15, 16, 17, 31, 32, 33, 63, 65])         # around the load width 16 and the step 32
def test_every_width_of_N(N):
    rng = np.random.default_rng(3720 + N)
    for K in (3, 33):
        for kind_a, kind_b in PAIRINGS:
            values = values_of(rng, K)
            a, b = random_side(rng, kind_a, K, (N,), values), random_side(rng, kind_b, K, (N,), values)
            want = E.confusion_statement(a, kind_a, b, kind_b, values)
            assert np.array_equal(device(a, kind_a, b, kind_b, values, (1, 1, N)), want), (N, K, kind_a, kind_b)


@pytest.mark.parametrize('K,spatial', [(3, (5, 61, 67)), (40, (5, 61, 67)), (255, (1, 231, 259))])
def test_several_sample_chunks_per_tile(K, spatial):
    """20435 samples are 20 chunks of CHUNK_MIN for one tile pair (K = 3) and for four (K = 40), the last one short and ending inside a step
    (20435 % 32 = 19).  K = 255 has 81 tile pairs, 4096 / 81 = 50 waves a pair: 59829 samples make the chunk ceil(59829 / 50) = 1197 -> 1280, the
    path where the chunk grows beyond CHUNK_MIN, and 47 chunks."""
    n = int(np.prod(spatial))
    pairs = ((K + 2 + 31) // 32) ** 2
    per_wave = -(-n // max(1, WAVES_AIM // pairs))
    chunk = max(CHUNK_MIN, -(-per_wave // 128) * 128)
    assert -(-n // chunk) >= 20 and (chunk > CHUNK_MIN) == (K == 255)
    rng = np.random.default_rng(3740 + K)
    for kind_a, kind_b in PAIRINGS if K < 255 else PAIRINGS[1:3]:
        a, b, values = sweep_case(rng, K, spatial, kind_a, kind_b)
        want = E.confusion_statement(a, kind_a, b, kind_b, values)
        assert distinct(want)
        assert np.array_equal(device(a, kind_a, b, kind_b, values, spatial), want), (K, kind_a, kind_b)


def test_plane_bytes_map_bytes_and_absent_labels():
    rng = np.random.default_rng(3760)
    K, spatial = 6, (3, 17, 33)
    values = [2, 9, 128, 200, 254, 255]                                     # not 1 ... K; values with the high bit
    for kind_a, kind_b in PAIRINGS:
        # label 1 absent on side a only, label 4 on both; the maps hold a byte that is none of the values
        a, b = random_side(rng, kind_a, K, spatial, values, absent=(1, 4)), random_side(rng, kind_b, K, spatial, values, absent=(4,))
        if kind_a == E.PLANES:
            assert set(np.unique(a)) == {0, 1, 127, 128, 255}
        else:
            assert stray_byte(values) in a
        want = E.confusion_statement(a, kind_a, b, kind_b, values)
        assert not want[2].any() and not want[5].any() and not want[:, 5].any() and want[:, 2].any()
        assert np.array_equal(device(a, kind_a, b, kind_b, values, spatial), want), (kind_a, kind_b)
    # every plane byte value at once against itself: 256 samples of plane 0 hold the bytes 0 ... 255
    p = np.zeros((2, 1, 1, 256), np.uint8)
    p[0, 0, 0] = np.arange(256)
    p[1, 0, 0, 128:] = np.arange(128, 256)
    assert device(p, E.PLANES, p, E.PLANES, None, (1, 1, 256)).tolist() == [[1, 0, 0, 1], [0, 255, 128, 255], [0, 128, 128, 128], [1, 255, 128, 256]]


def test_empty_and_full_sides_and_the_same_array():
    rng = np.random.default_rng(3770)
    K, spatial = 33, (2, 9, 35)
    values = values_of(rng, K)
    n = int(np.prod(spatial))
    for kind in (E.PLANES, E.LABELMAP):
        other = random_side(rng, E.PLANES, K, spatial, values, present=True)
        zero = np.zeros(((K,) if kind == E.PLANES else ()) + spatial, np.uint8)
        full = zero.copy()
        if kind == E.PLANES:
            full[7] = 255
        else:
            full[:] = values[7]
        for side in (zero, full):
            for swap in (False, True):
                x, kx, y, ky = (other, E.PLANES, side, kind) if swap else (side, kind, other, E.PLANES)
                want = E.confusion_statement(x, kx, y, ky, values)
                assert np.array_equal(device(x, kx, y, ky, values, spatial), want), (kind, swap)
        assert E.confusion_statement(zero, kind, other, E.PLANES, values)[0, K + 1] == n
        assert E.confusion_statement(full, kind, other, E.PLANES, values)[8, K + 1] == n
        same = random_side(rng, kind, K, spatial, values, present=True)     # a and b the same array (the same pointer)
        got = engine.label_confusion(same, kind, same, kind, values, spatial, 0)
        assert np.array_equal(got, E.confusion_statement(same, kind, same, kind, values)) and (got == got.T).all()


def test_margins_and_diagonal_are_the_overlap_entrys():
    rng = np.random.default_rng(3780)
    K, spatial = 40, (3, 17, 33)
    for kind_a, kind_b in PAIRINGS:
        a, b, values = sweep_case(rng, K, spatial, kind_a, kind_b)
        M = device(a, kind_a, b, kind_b, values, spatial)
        ov = engine.label_overlap(np.ascontiguousarray(a), kind_a, np.ascontiguousarray(b), kind_b, values, spatial, 0)
        d = np.arange(1, K + 1)
        assert np.array_equal(M[d, K + 1], ov[:, 0]) and np.array_equal(M[K + 1, d], ov[:, 1]) and np.array_equal(M[d, d], ov[:, 2])
        assert M[K + 1, K + 1] == int(np.prod(spatial))


def test_planes_past_byte_2_to_the_32():
    """130 planes of 2^25 + 17 samples on side a: plane 129 starts at byte 129 * (2^25 + 17) > 2^32, and no plane but the first is 16-byte aligned.
    Mostly zeros, marks in the first and in the last plane; side b a label map of the two marked labels' values and a stray byte.  Expected: the
    statement restricted to the marked planes (every other row of a is empty, every other column of b too)."""
    K, n = 130, 2 ** 25 + 17
    L.require('confusion K = 130, N = 2^25 + 17', K * n + 3 * n + (1 << 20), K * n + 16 * n)
    rng = np.random.default_rng(3790)
    values = values_of(rng, K)
    stray = stray_byte(values)
    a = np.zeros((K, n), np.uint8)
    for k, byte in ((0, 255), (K - 1, 128)):
        a[k, :4099] = (rng.random(4099) < 0.4) * byte
        a[k, n - 4099:] = (rng.random(4099) < 0.6) * byte
    a[K - 1, n - 1] = 1                                                     # the last byte of the last plane
    b = np.zeros(n, np.uint8)
    for lo in (0, n - 5000):
        b[lo:lo + 5000] = rng.choice(np.array([0, values[0], values[K - 1], stray], np.uint8), 5000, p=[0.1, 0.4, 0.3, 0.2])
    small = E.confusion_statement(np.stack([a[0], a[K - 1]]), E.PLANES, b, E.LABELMAP, [values[0], values[K - 1]])
    want = np.zeros((K + 2, K + 2), np.int64)
    at = np.array([0, 1, K, K + 1])
    want[np.ix_(at, at)] = small
    assert small[3, 3] == n and (small != small.T).any() and small[1, 1] > 0 and small[2, 2] > 0 and small[2, 1] > 0 and small[0, 0] > n - 20000
    with L.Clock('confusion K = 130, N = 2^25 + 17') as c:
        got = engine.label_confusion(a.reshape(K, 1, 1, n), E.PLANES, b.reshape(1, 1, n), E.LABELMAP, values, (1, 1, n), 0)
        c.result = f'corner {got[K + 1, K + 1]}'
    assert np.array_equal(got, want)


def test_refusals_by_name_leave_the_output_untouched():
    lib = _lib.load()
    K = 2
    p = np.ones((K, 4, 16, 64), np.uint8)
    m = np.ones((4, 16, 64), np.uint8)
    out = np.full((K + 2, K + 2), -77, np.int64)
    good, zero = np.array([9, 8], np.uint8), np.array([9, 0], np.uint8)
    P, M_ = p.ctypes.data, m.ctypes.data
    cases = {'null a': (None, 0, P, 0, None, K, 4, 16, 64), 'null b': (P, 0, None, 0, None, K, 4, 16, 64),
             'kind a': (P, 2, P, 0, None, K, 4, 16, 64), 'kind b': (P, 0, P, -1, None, K, 4, 16, 64),
             'K = 0': (P, 0, P, 0, None, 0, 4, 16, 64), 'K = 256': (P, 0, P, 0, None, 256, 4, 16, 64),
             'Z = 0': (P, 0, P, 0, None, K, 0, 16, 64), 'H = 0': (P, 0, P, 0, None, K, 4, 0, 64), 'W = -1': (P, 0, P, 0, None, K, 4, 16, -1),
             '2^31 samples': (P, 0, P, 0, None, K, 65536, 32768, 1),        # by arguments only: refused before a byte is read
             'map a without values': (M_, 1, P, 0, None, K, 4, 16, 64), 'map b without values': (P, 0, M_, 1, None, K, 4, 16, 64),
             'value 0': (M_, 1, M_, 1, zero.ctypes.data, K, 4, 16, 64)}
    for what, args in cases.items():
        assert lib.ts2d_label_confusion(0, *args, out.ctypes.data) == ERR_INVALID, what
        assert (out == -77).all() and 'ts2d_label_confusion' in _lib.last_error(), what
    assert lib.ts2d_label_confusion(0, P, 0, P, 0, None, K, 4, 16, 64, None) == ERR_INVALID and 'ts2d_label_confusion' in _lib.last_error()
    assert lib.ts2d_label_confusion(0, M_, 1, P, 0, good.ctypes.data, K, 4, 16, 64, out.ctypes.data) == 0          # ... and the call that is fine
    assert out.tolist() == [[0, 4096, 4096, 4096], [0, 0, 0, 0], [0, 0, 0, 0], [0, 4096, 4096, 4096]]


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('multilabel_pred,multilabel_ref,dim3', [(True, True, True), (True, False, False), (False, True, True), (False, False, False)])
def test_confusion_on_the_device_equals_the_host_route(multilabel_pred, multilabel_ref, dim3, monkeypatch):
    rng = np.random.default_rng(3800)
    K = 5
    spatial, sp = ((37, 1, 70), (0.8, 2.0, 2.5)) if dim3 else ((37, 70), (0.8, 2.5))
    nd = len(spatial)
    values = list(range(1, K + 1))

    def make(multi):
        side = random_side(rng, E.PLANES if multi else E.LABELMAP, K, spatial, values, absent=(3,), stray=False)
        arr = np.ascontiguousarray(np.moveaxis(side, 0, -1)) if multi else side
        return nrrd.Image(arr, sp, (0.0,) * nd, tuple(np.eye(nd).reshape(-1)), K if multi else 1, {}, None)
    pred, ref = make(multilabel_pred), make(multilabel_ref)
    pred.meta = {k: v for i in range(K) for k, v in ((f'Segment{i}_ID', str(i)), (f'Segment{i}_Name', f'l{i + 1}'),
                                                      (f'Segment{i}_LabelValue', '1' if multilabel_pred else str(i + 1)),
                                                      (f'Segment{i}_Layer', str(i) if multilabel_pred else '0'))}
    calls = []
    orig = engine.label_confusion
    monkeypatch.setattr(engine, 'label_confusion', lambda *a, **kw: (calls.append('label_confusion'), orig(*a, **kw))[1])
    dev = E.confusion(pred, ref, device=0)
    assert calls == ['label_confusion']
    host = E.confusion(pred, ref)
    assert calls == ['label_confusion'] and dev == host and len(dev['labels']) == K and dev['samples'] == 37 * 70
    assert dev['exclusive'] == (not multilabel_pred and not multilabel_ref) and (dev['kappa'] is not None) == dev['exclusive']
    assert any(l['predicted_as'] for l in dev['labels'].values()) and np.array(dev['matrix']).tolist() != np.array(dev['matrix']).T.tolist()
    own = E.confusion(pred, pred, device=0)                                 # the co-occurrence inside one result: one array on both sides
    assert own == E.confusion(pred, pred) and np.array(own['matrix']).tolist() == np.array(own['matrix']).T.tolist() and len(calls) == 2


def test_result_confusion_on_the_device_equals_the_host_route(tmp_path, monkeypatch):
    ids = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_ribs')
    models = {m: synthetic_model(m, 3 + i, 31 + i, patch=(64, 64), mirror=False)[0] for i, m in enumerate(ids)}
    case = nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))
    rng = np.random.default_rng(3810)
    lab = np.zeros(case.array.shape, np.int16)
    for v in range(1, 7):                                                   # label 7 stays absent
        lo = [int(rng.integers(0, s // 2)) for s in lab.shape]
        lab[tuple(slice(o, o + int(rng.integers(3, s // 2))) for o, s in zip(lo, lab.shape))] = v
    vol = nrrd.Image(lab, case.spacing, case.origin, case.direction, 1, {}, case.space)
    calls = []
    orig = engine.label_confusion
    monkeypatch.setattr(engine, 'label_confusion', lambda *a, **kw: (calls.append('label_confusion'), orig(*a, **kw))[1])
    with TS2D(models=models) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device == 0
        dev = res.confusion(vol)
        dev_files = res.save_confusion(str(tmp_path / 'dev'), 'case', vol)
        assert calls == ['label_confusion'] * 2
        res.device = None
        host = res.confusion(vol)
        host_files = res.save_confusion(str(tmp_path / 'host'), 'case', vol)
        assert len(calls) == 2 and dev == host and len(dev['labels']) == 7 and sum(dev['matrix'][i][i] for i in range(1, 8)) > 0
        assert [os.path.basename(f) for f in dev_files] == [os.path.basename(f) for f in host_files] == ['case.confusion.json']
        with open(dev_files[0], 'rb') as fa, open(host_files[0], 'rb') as fb:
            assert fa.read() == fb.read()
