"""The label morphology without a GPU: the statement (morphology.label_morphology_statement, the scan form) against scipy with the disc built
explicitly, against the Euclidean distance transform, the hand cases and the algebra; the label rules of planes and label maps; csrc/morph.h's host
walk as plain C++ under the sanitizers; and label_morphology / Result.morphology / the command line on the host route."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from tests import morphology_util as U
from tests.batch_util import synthetic_batch_model
from tests.conftest import GOLDEN, ROOT
from totalsegmentator2d_amd import image, main, nrrd
from totalsegmentator2d_amd import morphology as M
from totalsegmentator2d_amd.main import ts2d_run
from totalsegmentator2d_amd.tool import TS2D

A = os.path.join(GOLDEN, 'assets')
HIPCC = '/opt/rocm/bin/hipcc'


# ------------------------------------------------------------------------------------------------ 1. the statement against scipy
@pytest.fixture(scope='module')
def masks():
    return U.random_masks(240, 39)


def test_scan_form_equals_the_disc_form_of_scipy_on_random_masks(masks):
    assert len(masks) >= 200
    for m, r, sy, sx in masks:
        B = U.explicit_disc(r, sy, sx, *m.shape)
        assert np.array_equal(B, M.disc(r, sy, sx, *m.shape))
        for op in U.OPS:
            got = M.binary_morphology(m, op, r, (sy, sx))
            assert got.dtype == bool and np.array_equal(got, U.scipy_op(m, op, B)), (op, m.shape, r, sy, sx)


def test_dilation_agrees_with_the_distance_transform_away_from_the_circle(masks):
    checked = 0
    for m, r, sy, sx in masks:
        if not m.any():
            continue
        d = ndimage.distance_transform_edt(~m, sampling=(sy, sx))
        clear = np.abs(d - r) > 1e-9                    # a distance within 1e-9 of r is the rounding's to decide, not this check's
        got = M.binary_morphology(m, 'dilate', r, (sy, sx))
        assert np.array_equal(got[clear], (d <= r)[clear])
        checked += int(clear.sum())
    assert checked > 10000


def test_algebra_on_every_random_mask(masks):
    for m, r, sy, sx in masks:
        op = {o: M.binary_morphology(m, o, r, (sy, sx)) for o in U.OPS}
        assert not (op['open'] & ~m).any() and not (m & ~op['close']).any()                  # open <= M <= close
        assert not (op['erode'] & ~m).any() and not (m & ~op['dilate']).any()
        assert np.array_equal(M.binary_morphology(op['open'], 'open', r, (sy, sx)), op['open'])          # idempotent
        assert np.array_equal(M.binary_morphology(op['close'], 'close', r, (sy, sx)), op['close'])
        assert np.array_equal(op['erode'], ~M.binary_morphology(~m, 'dilate', r, (sy, sx)))      # the dual inside the image


def test_cover_table():
    assert M.cover_table(0.0, 1.0, 1.0, 7, 9).tolist() == [0]
    assert M.cover_table(5.0, 1.0, 1.0, 9, 9).tolist() == [5, 4, 4, 4, 3, 0]                   # 3-4-5 and 5-0 on the circle
    assert M.cover_table(5.0, 1.0, 1.0, 4, 3).tolist() == [2, 2, 2, 2]                         # ends at H, clipped to W - 1
    assert M.cover_table(2.5, 0.5, 0.5, 9, 9).tolist() == [5, 4, 4, 4, 3, 0]
    assert M.cover_table(1.0, 2.5, 0.8, 9, 9).tolist() == [1]
    assert M.cover_table(1e200, 1.0, 1.0, 3, 4).tolist() == [3, 3, 3]                          # r r = inf: everything
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            M.cover_table(bad, 1.0, 1.0, 3, 3)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            M.cover_table(1.0, bad, 1.0, 3, 3)


def test_hand_cases():
    one = np.zeros((21, 21), bool)
    one[10, 10] = True
    for r, s in ((5.0, 1.0), (2.5, 0.5)):              # the 3-4-5 offset is exactly on the circle: inside
        d = M.binary_morphology(one, 'dilate', r, (s, s))
        for dy, dx in ((3, 4), (4, 3), (5, 0), (0, 5), (-3, -4), (-4, 3)):
            assert d[10 + dy, 10 + dx]
        assert not d[14, 14] and not d[15, 11] and not d[10, 16] and int(d.sum()) == 81
    rng = np.random.default_rng(1)
    m = rng.random((12, 17)) < 0.3
    for op in U.OPS:
        assert np.array_equal(M.binary_morphology(m, op, 0.0, (0.8, 2.5)), m)                    # r = 0
        assert np.array_equal(M.binary_morphology(m, op, 0.7999, (0.8, 2.5)), m)                 # r just below one spacing
    d = M.binary_morphology(one, 'dilate', 1.0, (2.5, 0.8))                                      # r between sx and sy: along x only
    assert sorted(zip(*np.nonzero(d))) == [(10, 9), (10, 10), (10, 11)]
    d = M.binary_morphology(one, 'dilate', 1.0, (0.8, 2.5))
    assert sorted(zip(*np.nonzero(d))) == [(9, 10), (10, 10), (11, 10)]
    # r beyond the image
    assert M.binary_morphology(one, 'dilate', 1e6).all() and not M.binary_morphology(~one, 'erode', 1e6).any()
    assert M.binary_morphology(np.ones((4, 5), bool), 'erode', 1e6).all() and not M.binary_morphology(np.zeros((4, 5), bool), 'dilate', 1e6).any()
    assert M.binary_morphology(one, 'close', 1e6).all() and not M.binary_morphology(one, 'open', 1e6).any()
    # H = 1 and W = 1
    line = np.array([[0, 0, 1, 0, 0, 0, 1, 1, 0]], bool)
    assert M.binary_morphology(line, 'dilate', 1.0).astype(int).tolist() == [[0, 1, 1, 1, 0, 1, 1, 1, 1]]
    assert M.binary_morphology(line, 'erode', 1.0).astype(int).tolist() == [[0, 0, 0, 0, 0, 0, 0, 0, 0]]
    assert M.binary_morphology(line.T, 'dilate', 1.0).astype(int).T.tolist() == [[0, 1, 1, 1, 0, 1, 1, 1, 1]]
    assert M.binary_morphology(line.T, 'close', 1.0).astype(int).T.tolist() == [[0, 0, 1, 0, 0, 0, 1, 1, 1]]
    for v in (False, True):
        assert M.binary_morphology(np.array([[v]]), 'dilate', 3.0).tolist() == [[v]] and M.binary_morphology(np.array([[v]]), 'erode', 3.0).tolist() == [[v]]
    # empty and full
    for op in U.OPS:
        assert not M.binary_morphology(np.zeros((5, 6), bool), op, 2.0).any() and M.binary_morphology(np.ones((5, 6), bool), op, 2.0).all()
    # a mask on an edge is not eroded from that edge
    for k in range(4):
        band = np.zeros((9, 9), bool)
        band[:3] = True
        band = np.rot90(band, k)
        want = np.zeros((9, 9), bool)
        want[:2] = True
        assert np.array_equal(M.binary_morphology(band, 'erode', 1.0), np.rot90(want, k))
        assert not np.array_equal(ndimage.binary_erosion(band, structure=M.disc(1.0, 1.0, 1.0, 9, 9)), np.rot90(want, k))     # (scipy's default is not this)
    with pytest.raises(ValueError):
        M.binary_morphology(one, 'grow', 1.0)


# ------------------------------------------------------------------------------------------------ 2. labels
def test_planes_and_label_maps_equal_the_restatement_on_random_inputs():
    rng = np.random.default_rng(40)
    for trial in range(24):
        H, W, K = int(rng.integers(1, 20)), int(rng.integers(1, 40)), int(rng.integers(1, 5))
        sp = tuple(float(v) for v in rng.choice(U.SPACINGS, 2))
        r = float(rng.choice([0.0, 0.8, 1.0, 2.0, 3.3, 1000.0]))
        select = None if trial % 3 else [bool(v) for v in rng.integers(0, 2, K)]
        planes = U.speckle_planes(rng, K, H, W, (0.03, 0.3, 0.8)[trial % 3])
        values = [int(v) for v in rng.choice(np.arange(1, 256), K, replace=False)]
        lmap = U.speckle_map(rng, values, H, W, (0.2, 0.6, 0.95)[trial % 3], others=[v for v in (7, 200) if v not in values])
        for op in U.OPS:
            for seg, vals in ((planes, None), (lmap, values)):
                got = M.label_morphology_statement(seg, vals, op, r, sp, select)
                assert got[0].dtype == seg.dtype and got[1].dtype == np.int64 and got[1].shape == (K, 4)
                assert U.same(got, U.restatement(seg, vals, op, r, sp, select)), (trial, op, vals)
                assert np.array_equal(got[1][:, 1], got[1][:, 0] + got[1][:, 2] - got[1][:, 3])
                if r == 0.0:
                    assert got[0].tobytes() == seg.tobytes()


def test_label_rules_by_hand():
    # planes: a pixel that stays keeps its byte, a new one is 1, a cleared one 0
    p = np.zeros((1, 1, 7), np.uint8)
    p[0, 0, 2:5] = (9, 200, 1)
    out, ctr = M.label_morphology_statement(p, None, 'dilate', 1.0, (1.0, 1.0))
    assert out[0, 0].tolist() == [0, 1, 9, 200, 1, 1, 0] and ctr.tolist() == [[3, 5, 2, 0]]
    out, ctr = M.label_morphology_statement(p, None, 'erode', 1.0, (1.0, 1.0))
    assert out[0, 0].tolist() == [0, 0, 0, 200, 0, 0, 0] and ctr.tolist() == [[3, 1, 0, 2]]
    # a label map: two labels compete for one background pixel, the first in `values` wins
    m = np.array([[5, 0, 3]], np.uint8)
    out, ctr = M.label_morphology_statement(m, [3, 5], 'dilate', 1.0, (1.0, 1.0))
    assert out.tolist() == [[5, 3, 3]] and ctr.tolist() == [[1, 2, 1, 0], [1, 1, 0, 0]]
    out, ctr = M.label_morphology_statement(m, [5, 3], 'dilate', 1.0, (1.0, 1.0))
    assert out.tolist() == [[5, 5, 3]] and ctr.tolist() == [[1, 2, 1, 0], [1, 1, 0, 0]]
    # an unnamed non-zero value is never overwritten, and neither is a named one
    m = np.array([[5, 9, 0, 3, 0]], np.uint8)
    out, _ = M.label_morphology_statement(m, [5, 3], 'dilate', 10.0, (1.0, 1.0))
    assert out.tolist() == [[5, 9, 5, 3, 5]]
    # an unselected label stays untouched and is an obstacle
    out, ctr = M.label_morphology_statement(m, [5, 3], 'dilate', 10.0, (1.0, 1.0), select=[False, True])
    assert out.tolist() == [[5, 9, 3, 3, 3]] and ctr.tolist() == [[1, 1, 0, 0], [1, 3, 2, 0]]
    out, ctr = M.label_morphology_statement(m, [5, 3], 'erode', 10.0, (1.0, 1.0), select=[False, True])
    assert out.tolist() == [[5, 9, 0, 0, 0]] and ctr.tolist() == [[1, 1, 0, 0], [1, 0, 0, 1]]
    # a shrink leaves zeros, also next to another label (everything that is not the label is outside its mask)
    m = np.array([[4, 4, 4, 4, 6, 6, 6, 6, 6]], np.uint8)
    out, ctr = M.label_morphology_statement(m, [4, 6], 'erode', 1.0, (1.0, 1.0))
    assert out.tolist() == [[4, 4, 4, 0, 0, 6, 6, 6, 6]] and ctr.tolist() == [[4, 3, 0, 1], [5, 4, 0, 1]]
    out, _ = M.label_morphology_statement(m, [4, 6], 'open', 2.0, (1.0, 1.0))
    assert out.tolist() == [[4, 4, 4, 4, 6, 6, 6, 6, 6]]
    # refusals by name
    with pytest.raises(ValueError, match='volume'):
        M.label_morphology_statement(np.zeros((3, 4, 5), np.uint8), [1], 'dilate', 1.0, (1.0, 1.0))
    with pytest.raises(ValueError, match='volume'):
        M.label_morphology_statement(np.zeros((2, 3, 4, 5), np.uint8), None, 'dilate', 1.0, (1.0, 1.0))
    with pytest.raises(ValueError, match='select'):
        M.label_morphology_statement(m, [4, 6], 'dilate', 1.0, (1.0, 1.0), select=[True])
    with pytest.raises(ValueError, match='distinct'):
        M.label_morphology_statement(m, [4, 4], 'dilate', 1.0, (1.0, 1.0))


# ------------------------------------------------------------------------------------------------ 3. csrc/morph.h on the host, under the sanitizers
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    """tests/morph_driver.cpp - csrc/morph.h behind a main of its own - under the address and undefined-behaviour sanitizers where the toolchain
    links them (nothing loaded into Python runs under a sanitizer)."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = tmp_path_factory.mktemp('morph_driver') / 'morph_driver'
    base = [cxx, '-x', 'c++', '-O1', '-g', '-std=c++17', '-Wno-unknown-pragmas', '-o', str(exe), os.path.join(ROOT, 'tests', 'morph_driver.cpp')]
    if subprocess.call(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    return str(exe)


def driver_cases():
    """(seg [H, W] uint8, kind, value, r, sy, sx): the hand cases, W = 1, 63, 64, 65, 130, a table of length 1 and one of length H."""
    rng = np.random.default_rng(41)
    out = []
    one = np.zeros((21, 21), np.uint8)
    one[10, 10] = 3
    out += [(one, 0, 0, 5.0, 1.0, 1.0), (one, 1, 3, 2.5, 0.5, 0.5), (one, 1, 4, 2.5, 0.5, 0.5), (one, 0, 0, 1.0, 2.5, 0.8), (one, 0, 0, 1e6, 1.0, 1.0)]
    for W in (1, 63, 64, 65, 130):
        for H in (1, 5):
            for density in (0.03, 0.5, 0.97):
                seg = ((rng.random((H, W)) < density) * rng.integers(1, 4, (H, W))).astype(np.uint8)
                for r, sy, sx in ((0.0, 1.0, 1.0), (0.9, 1.0, 2.5), (2.0, 0.8, 2.5), (2.0, 2.5, 0.8), (3.3, 1.0, 1.0), (70.0, 1.0, 1.0), (1e4, 0.7, 1.3)):
                    out.append((seg, int(rng.integers(0, 2)), 2, r, sy, sx))
        ends = np.zeros((3, W), np.uint8)                # a pixel at each end of the row: the carries cross every chunk, both ways
        ends[1, 0] = ends[1, -1] = 1
        out += [(ends, 0, 0, float(W) / 2 - 0.25, 1.0, 1.0), (ends, 0, 0, float(W), 1.0, 1.0), (ends[:, :1].copy(), 0, 0, 1.0, 1.0, 1.0)]
    for k in range(4):
        band = np.zeros((9, 9), np.uint8)
        band[:3] = 1
        out.append((np.ascontiguousarray(np.rot90(band, k)), 0, 0, 1.0, 1.0, 1.0))
    out += [(np.zeros((6, 7), np.uint8), 0, 0, 2.0, 1.0, 1.0), (np.full((6, 7), 9, np.uint8), 0, 0, 2.0, 1.0, 1.0)]
    return out


def test_host_walk_of_morph_h_gives_the_statements_bytes(driver, tmp_path):
    runs = [(c, op) for c in driver_cases() for op in range(4)]
    with open(tmp_path / 'in.bin', 'wb') as f:
        for (seg, kind, value, r, sy, sx), op in runs:
            f.write(struct.pack('<5i3d', seg.shape[0], seg.shape[1], kind, value, op, r, sy, sx))
            f.write(seg.tobytes())
    subprocess.run([driver, str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')], check=True)
    got = (tmp_path / 'out.bin').read_bytes()
    at = 0
    lengths = set()
    for (seg, kind, value, r, sy, sx), op in runs:
        H, W = seg.shape
        T = struct.unpack_from('<i', got, at)[0]
        cover = np.frombuffer(got, np.int32, T, at + 4)
        res = np.frombuffer(got, np.uint8, H * W, at + 4 + 4 * T).reshape(H, W)
        at += 4 + 4 * T + H * W
        assert cover.tolist() == M.cover_table(r, sy, sx, H, W).tolist()
        mask = seg == value if kind else seg > 0
        assert np.array_equal(res, M.binary_morphology(mask, U.OPS[op], r, (sy, sx)).astype(np.uint8)), (seg.shape, kind, value, r, sy, sx, op)
        lengths.add((T == 1, T == H and H > 1))
    assert at == len(got) and (True, False) in lengths and (False, True) in lengths


# ------------------------------------------------------------------------------------------------ 4. images, results, the command line (host route)
def _ts2d_shaped(multilabel: bool):
    """What TS2D.predict returns: 3-D with a unit axis, spacings (0.8, 7.0, 2.5) - array axis 0 has 2.5, axis 2 has 0.8."""
    spatial, sp = (9, 1, 11), (0.8, 7.0, 2.5)
    eye = tuple(float(v) for v in np.eye(3).reshape(-1))
    if multilabel:
        arr = np.zeros(spatial + (3,), np.uint8)
        arr[4, 0, 5, 0] = 200
        arr[2:7, 0, 3:9, 2] = 77
        seg = nrrd.Image(arr, sp, (0.0,) * 3, eye, 3, {}, None)
        image.set_annotation_meta(seg, {1: 'a', 2: 'b', 3: 'c'}, {'a': (255, 0, 0)})
    else:
        arr = np.zeros(spatial, np.uint8)
        arr[4, 0, 5] = 2
        arr[0:2, 0, 0:4] = 6
        seg = nrrd.Image(arr, sp, (0.0,) * 3, eye, 1, {}, None)
        image.set_annotation_meta(seg, {2: 'two', 6: 'six'}, {})
    return seg


def test_label_morphology_of_a_ts2d_shaped_image_uses_the_in_plane_spacings():
    for multilabel in (True, False):
        seg = _ts2d_shaped(multilabel)
        before = seg.array.tobytes()
        got, ctr = M.label_morphology(seg, 'dilate', 1.0)
        assert seg.array.tobytes() == before and got is not seg and got.array.shape == seg.array.shape and got.meta == seg.meta
        assert (got.spacing, got.origin, got.direction, got.components) == (seg.spacing, seg.origin, seg.direction, seg.components)
        first = got.array[..., 0] if multilabel else (got.array == 2)
        assert sorted(zip(*np.nonzero(first))) == [(4, 0, 4), (4, 0, 5), (4, 0, 6)]             # r = 1 reaches along the 0.8 axis only
        planes = np.moveaxis(seg.array, -1, 0).reshape(3, 9, 11) if multilabel else seg.array.reshape(9, 11)
        values = None if multilabel else [2, 6]
        want = M.label_morphology_statement(planes, values, 'dilate', 1.0, (2.5, 0.8))
        flat = np.moveaxis(got.array, -1, 0).reshape(3, 9, 11) if multilabel else got.array.reshape(9, 11)
        assert np.array_equal(flat, want[0])
        names = list(image.get_annotation_labels(seg))
        assert list(ctr) == names and sorted(ctr[names[0]]) == sorted(M.COUNTER_NAMES)
        assert [ctr[n]['pixels_after'] for n in names] == (want[1][:, 1].tolist())
        wide = M.label_morphology(seg, 'dilate', 2.6)[0].array                                 # one step along the 2.5 axis, three along the 0.8 axis
        flat = np.moveaxis(wide, -1, 0).reshape(3, 9, 11) if multilabel else wide.reshape(9, 11)
        assert np.array_equal(flat, M.label_morphology_statement(planes, values, 'dilate', 2.6, (2.5, 0.8))[0])
        assert sorted(zip(*np.nonzero(flat[0] if multilabel else flat == 2))) == [(3, 5)] + [(4, x) for x in range(2, 9)] + [(5, 5)]
        for wrong in ((0.8, 2.5), (7.0, 0.8), (2.5, 7.0), (0.8, 7.0)):                          # a swapped or wrong spacing shows
            assert not np.array_equal(M.label_morphology_statement(planes, values, 'dilate', 2.6, wrong)[0], flat)
        # labels: a subset; the rest stays
        only, c1 = M.label_morphology(seg, 'erode', 1.0, labels=[names[-1]])
        sel = [False] * (3 if multilabel else 2)
        sel[-1] = True
        w1 = M.label_morphology_statement(planes, values, 'erode', 1.0, (2.5, 0.8), sel)
        flat = np.moveaxis(only.array, -1, 0).reshape(3, 9, 11) if multilabel else only.array.reshape(9, 11)
        assert np.array_equal(flat, w1[0]) and c1[names[0]]['removed'] == 0 and c1[names[-1]]['removed'] > 0
        zero, _ = M.label_morphology(seg, 'open', 0.0)
        assert zero.array.tobytes() == before
        with pytest.raises(ValueError, match='nobody'):
            M.label_morphology(seg, 'dilate', 1.0, labels=['nobody'])
    vol = nrrd.Image(np.zeros((3, 4, 5), np.uint8), (1.0, 1.0, 1.0), (0.0,) * 3, tuple(float(v) for v in np.eye(3).reshape(-1)), 1, {}, None)
    image.set_annotation_meta(vol, {1: 'x'}, {})
    with pytest.raises(ValueError, match='volume'):
        M.label_morphology(vol, 'dilate', 1.0)


@pytest.fixture(scope='module')
def two_models():
    m1, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_cardiac', 3, 31, mirror=False, feats=(32, 32))
    m2, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_ribs', 4, 32, mirror=False, feats=(32, 32))
    return {'ts2d-v2-ep4000b2_cardiac': m1, 'ts2d-v2-ep4000b2_ribs': m2}


def test_result_morphology_on_the_host_route(two_models):
    with TS2D(models=dict(two_models)) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device is None
        seg = res.get_segmentation()
        before = seg.array.tobytes()
        parts = {m: res.get_segmentation(m).array.tobytes() for m in res.models}
        same = res.morphology('close', 0.0)
        assert same is not res and same.get_segmentation() is not seg and same.get_segmentation().array.tobytes() == before
        assert all(same.get_segmentation(m).array.tobytes() == parts[m] for m in res.models) and same.models == res.models
        assert same.get_input() is res.get_input() and all(same.get_projection(c) is p for c, p in res.get_projection().items())
        assert same.get_segmentation().meta == seg.meta and same.device is res.device
        grown = res.morphology('dilate', 3.0)
        assert seg.array.tobytes() == before and all(res.get_segmentation(m).array.tobytes() == parts[m] for m in res.models)
        assert grown.get_segmentation().array.tobytes() == M.label_morphology(seg, 'dilate', 3.0)[0].array.tobytes() != before
        for m in res.models:
            assert grown.get_segmentation(m).array.tobytes() == M.label_morphology(res.get_segmentation(m), 'dilate', 3.0)[0].array.tobytes()
        only = res.morphology('dilate', 3.0, labels=['ribs_2'], models=['ts2d-v2-ep4000b2_ribs'])
        assert only.get_segmentation('ts2d-v2-ep4000b2_cardiac').array.tobytes() == parts['ts2d-v2-ep4000b2_cardiac']
        assert only.get_segmentation().array.tobytes() == M.label_morphology(seg, 'dilate', 3.0, labels=['ribs_2'])[0].array.tobytes()
        with pytest.raises(ValueError, match='nobody'):
            res.morphology('dilate', 3.0, labels=['nobody'])
        with pytest.raises(ValueError):
            res.morphology('grow', 3.0)


def test_cli_flags_order_and_argument_errors(tmp_path, two_models, monkeypatch, capsys):
    src = tmp_path / 'in'
    os.makedirs(src)
    shutil.copy(os.path.join(A, 'sample_s0521.nrrd'), src / 'one.nrrd')
    run = dict(models=dict(two_models), visualize=False, silent=True)
    ts2d_run(str(src), str(tmp_path / 'plain'), **run)
    ts2d_run(str(src), str(tmp_path / 'zero'), morphology=('open', 0.0), **run)
    ts2d_run(str(src), str(tmp_path / 'open'), morphology=('open', 2.0), keep_largest=True, **run)
    assert sorted(os.listdir(tmp_path / 'zero')) == sorted(os.listdir(tmp_path / 'plain'))
    for f in os.listdir(tmp_path / 'plain'):
        assert (tmp_path / 'zero' / f).read_bytes() == (tmp_path / 'plain' / f).read_bytes()
    with TS2D(models=dict(two_models)) as ts:          # the step runs BEFORE the clean-up
        res = ts.predict(str(src / 'one.nrrd'))
        want = res.morphology('open', 2.0).cleaned(keep_largest=True).get_segmentation().array
        other = res.cleaned(keep_largest=True).morphology('open', 2.0).get_segmentation().array
    saved = nrrd.read(str(tmp_path / 'open' / 'one.seg.nrrd')).array
    assert saved.tobytes() == want.tobytes() and want.tobytes() != res.get_segmentation().array.tobytes()
    assert want.tobytes() != other.tobytes()            # (else the case does not show the order)
    # the parser
    seen = {}
    monkeypatch.setattr(main, 'ts2d_run', lambda **kw: (seen.clear(), seen.update(kw)))
    base = ['-i', str(src), '-o', str(tmp_path / 'e')]
    main.ts2d_entry_point(base)
    assert not {'morphology', 'morphology_labels'} & set(seen)                                  # the call of before
    for flag, op in (('--grow', 'dilate'), ('--shrink', 'erode'), ('--open', 'open'), ('--close', 'close')):
        main.ts2d_entry_point(base + [flag, '2.5'])
        assert seen['morphology'] == (op, 2.5) and 'morphology_labels' not in seen
    main.ts2d_entry_point(base + ['--grow', '0', '--morphology-labels', 'ribs_1, ribs_2', '--keep-largest'])
    assert seen['morphology'] == ('dilate', 0.0) and seen['morphology_labels'] == ['ribs_1', 'ribs_2'] and seen['keep_largest'] is True
    for bad in (['--grow', '1', '--shrink', '1'], ['--open', '1', '--close', '2'], ['--morphology-labels', 'ribs_1'], ['--grow', '-1'],
                ['--close', 'nan'], ['--grow', '1', '--morphology-labels', ' , ']):
        with pytest.raises(SystemExit) as ei:
            main.ts2d_entry_point(base + bad)
        assert ei.value.code == 2
    assert '--morphology-labels' in capsys.readouterr().err


def test_the_symbol_is_optional_and_the_abi_version_stays():
    from totalsegmentator2d_amd import _lib
    with open(os.path.join(ROOT, 'include', 'ts2d_engine.h')) as f:
        hdr = f.read()
    assert 'ts2d_label_morphology' in _lib.SIGNATURES and 'ts2d_label_morphology' in _lib.OPTIONAL and _lib.ABI_VERSION == 9
    for name, value in (('DILATE', _lib.MORPH_DILATE), ('ERODE', _lib.MORPH_ERODE), ('OPEN', _lib.MORPH_OPEN), ('CLOSE', _lib.MORPH_CLOSE),
                        ('COUNTERS', _lib.MORPH_COUNTERS)):
        assert f'#define TS2D_MORPH_{name} {value}\n' in hdr
    assert [_lib.MORPH_DILATE, _lib.MORPH_ERODE, _lib.MORPH_OPEN, _lib.MORPH_CLOSE] == [M.OPS.index(o) for o in M.OPS]
    lib = _lib.load()
    assert hasattr(lib, 'ts2d_label_morphology') and lib.ts2d_abi_version() == 9
