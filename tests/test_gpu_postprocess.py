"""nnU-Net's largest-component postprocessing on the MI355X: the entry ts2d_keep_largest_components (csrc/kernels_post_cc.h) against the
numpy/scipy statement ``postprocess.keep_largest_components_statement`` - bytes and the four counters of every step - on crafted and random
maps, its refusals, and a synthetic label-map model with a plan through ``HIPModel.apply`` / ``apply_batch`` against its own host route
(``device_postprocessing = False``)."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

from tests import prob_util
from tests.surface_util import synthetic_model
from tests.test_postprocess_cpu import serpentine
from totalsegmentator2d_amd import _lib, nrrd, prng
from totalsegmentator2d_amd.engine import has_keep_largest_components, keep_largest_components
from totalsegmentator2d_amd.model import HIPModel
from totalsegmentator2d_amd.postprocess import PostprocessingPlan, apply_postprocessing, keep_largest_components_statement

pytestmark = pytest.mark.gpu
FULL = np.ones((3, 3, 3), bool)
EACH = [([1, 2, 3], 0), ([1], 0), ([2], 0), ([3], 0)]          # "all foreground, then every label"


def _check(seg, plan, must_remove=False):
    """The entry on `seg` under `plan`: the statement's bytes and counters; the input is left alone.  Returns the counters."""
    seg = np.ascontiguousarray(seg, np.uint8)
    before = seg.copy()
    want, want_stats = keep_largest_components_statement(seg, plan)
    tables, bgs = PostprocessingPlan(plan).compiled
    got, stats, status = keep_largest_components(seg, tables, bgs, device=0)
    assert status == 0
    print(f'{seg.shape} steps={len(tables)} stats={stats.tolist()}')
    assert np.array_equal(stats, want_stats), (stats.tolist(), want_stats.tolist())
    assert got.dtype == np.uint8 and got.shape == seg.shape and np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(seg, before)
    if must_remove:
        assert stats[:, 3].sum() > 0
    return stats


def _random(seed, shape, density, labels=3):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) < density) * rng.integers(1, labels + 1, shape)).astype(np.uint8)


def spiral(n):
    """A one-voxel square spiral in an n x n plane, its arms one empty line apart: ONE 8-connected component whose voxels lie n^2 / 2 steps apart."""
    v = np.zeros((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    v[0, 0] = 1
    while True:
        moved = 0
        while True:
            ny, nx = y + dy, x + dx
            ahead = (ny + dy, nx + dx)
            if not (0 <= ny < n and 0 <= nx < n) or v[ny, nx] or (0 <= ahead[0] < n and 0 <= ahead[1] < n and v[ahead]):
                break
            y, x = ny, nx
            v[y, x] = 1
            moved += 1
        if moved < 2:
            return v
        dy, dx = dx, -dy


def test_the_entry_is_there():
    assert has_keep_largest_components() and 'ts2d_keep_largest_components' in _lib.OPTIONAL


@pytest.mark.parametrize('W', [1, 63, 64, 65, 130])
def test_planes_of_every_width_around_the_word(W):
    for k, density in enumerate((0.3, 0.5, 0.8)):
        _check(_random(10 * W + k, (1, 37, W), density), EACH, must_remove=W > 1)
        _check(_random(10 * W + k, (37, W), density)[:, :W], [([1, 2, 3], 5)])       # a 2-D array, another background


@pytest.mark.parametrize('shape', [(3, 5, 7), (5, 70, 130)])
@pytest.mark.parametrize('density', [0.15, 0.3, 0.5, 0.8])
def test_random_volumes_equal_the_statement(shape, density):
    stats = _check(_random(int(density * 100) + shape[0], shape, density), EACH, must_remove=True)
    if shape == (5, 70, 130) and density == 0.3:
        assert stats[0, 1] > 10 and stats[0, 2] > stats[0, 0] // 2                   # small components beside a giant one
        assert (stats[1:, 1] > 500).all()                                           # ... and a thousand per label


def test_components_across_word_row_and_block_ends():
    v = np.zeros((3, 9, 130), np.uint8)
    v[0, 0, 60:70] = 1              # a run across the first word end
    v[0, 0, 120:130] = 1            # ... one that ends with its row: (0, 0, 129) and (0, 1, 0) are index neighbours, not voxel neighbours
    v[0, 1, 0:3] = 1
    v[0, 3, 63] = v[0, 4, 64] = 1   # a diagonal step across a word end
    v[0, 6, 127:130] = 1
    v[1, 7, 129] = 1                # ... and a corner contact across slices at the last column
    v[1:3, :, 100] = 1              # a wall through every row of two slices: a block of four words holds 1 1/3 rows
    v[2, 8, 0:101] = 1
    stats = _check(v, [([1], 0)], must_remove=True)
    assert stats[0, 1] == ndimage.label(v, structure=FULL)[1] == 6
    _check(v * 7, [([7], 3)], must_remove=True)


def test_deep_chains_serpentine_and_spiral():
    s = serpentine(4, 64, 64)
    stats = _check(s, [([1], 0)])
    assert stats.tolist() == [[int(s.sum()), 1, int(s.sum()), 0]]
    lone = np.concatenate([s, np.zeros((2, 64, 64), np.uint8)])                      # an empty slice, then one voxel of its own
    lone[5, 63, 63] = 1
    assert _check(lone, [([1], 0)]).tolist() == [[int(s.sum()) + 1, 2, int(s.sum()), 1]]
    sp = spiral(129)
    assert ndimage.label(sp, structure=np.ones((3, 3)))[1] == 1 and sp.sum() > 129 * 129 // 3
    assert _check(sp[None], [([1], 0)]).tolist() == [[int(sp.sum()), 1, int(sp.sum()), 0]]
    assert _check(np.stack([sp, 0 * sp, sp.T * 2]), [([1, 2], 0)]).tolist() == [[2 * int(sp.sum()), 2, int(sp.sum()), 0]]       # a tie: both stay


def test_tie_empty_and_all_mask():
    c = np.zeros((1, 5, 9), np.uint8)
    c[0, 0, 0:3] = c[0, 4, 6:9] = 1
    c[0, 2, 4] = 1
    assert _check(c, [([1], 0)]).tolist() == [[7, 3, 3, 1]]
    assert _check(c, [([5], 0), ([1], 0)]).tolist() == [[0, 0, 0, 0], [7, 3, 3, 1]]
    assert _check(np.zeros((2, 3, 70), np.uint8), [([1], 0)]).tolist() == [[0, 0, 0, 0]]
    assert _check(np.full((2, 3, 70), 255, np.uint8), [([255], 0)]).tolist() == [[420, 1, 420, 0]]
    out, stats, status = keep_largest_components(c, np.zeros((0, 256), np.uint8), np.zeros(0, np.uint8))    # no steps: nothing to do
    assert status == 0 and np.array_equal(out, c) and stats.shape == (0, 4)


def test_a_plan_of_nineteen_steps_over_eighteen_labels():
    seg = _random(19, (4, 40, 70), 0.6, labels=18)
    plan = [(list(range(1, 19)), 0)] + [([k], 0) for k in range(1, 19)]
    stats = _check(seg, plan, must_remove=True)
    assert stats.shape == (19, 4) and (stats[1:, 3] > 0).all()
    out, _, route = apply_postprocessing(seg, plan, device=0)
    assert route == 'device' and np.array_equal(out, keep_largest_components_statement(seg, plan)[0])


def test_a_random_label_map_across_many_blocks():
    stats = _check(_random(64, (64, 256, 256), 0.3), EACH, must_remove=True)
    assert stats[0, 0] > 1_000_000 and stats[0, 1] > 100 and (stats[1:, 1] > 10_000).all()       # (a giant with a few hundred islands; per label tens of thousands)


def test_refusals_by_name_leave_the_buffer_alone():
    lib = _lib.load()
    seg = _random(5, (2, 6, 70), 0.5)
    before = seg.copy()
    steps = (_lib.CcStep * 1)()
    steps[0].member[1] = 1
    stats = np.full((1, 4), -1, np.int64)
    status = ctypes.c_int(77)
    call = lambda s, z, h, w, st, n, sp: lib.ts2d_keep_largest_components(0, s, z, h, w, ctypes.cast(st, ctypes.c_void_p) if st is not None else None, n,   # noqa: E731
                                                                        stats.ctypes.data, sp)
    for args, word in [((None, 2, 6, 70, steps, 1, ctypes.byref(status)), 'null argument'),
                       ((seg.ctypes.data, 2, 6, 70, None, 1, ctypes.byref(status)), 'null argument'),
                       ((seg.ctypes.data, 2, 6, 70, steps, 1, None), 'null argument'),
                       ((seg.ctypes.data, 0, 6, 70, steps, 1, ctypes.byref(status)), 'extents 0 x 6 x 70 must be positive'),
                       ((seg.ctypes.data, 2, -6, 70, steps, 1, ctypes.byref(status)), 'must be positive'),
                       ((seg.ctypes.data, 1 << 16, 1 << 15, 1, steps, 1, ctypes.byref(status)), 'more voxels than one call takes'),
                       ((seg.ctypes.data, 1 << 16, 1 << 16, 1 << 16, steps, 1, ctypes.byref(status)), 'more voxels than one call takes'),
                       ((seg.ctypes.data, 2, 6, 70, steps, -1, ctypes.byref(status)), '-1 steps')]:
        assert call(*args) == -1, word
        assert _lib.last_error().startswith('ts2d_keep_largest_components: ') and word in _lib.last_error(), _lib.last_error()
        assert np.array_equal(seg, before) and (stats == -1).all()
    assert call(seg.ctypes.data, 2, 6, 70, steps, 1, ctypes.byref(status)) == 0 and status.value == 0                # (the same buffers are fine)
    assert np.array_equal(seg, keep_largest_components_statement(before, [([1], 0)])[0]) and stats[0, 0] == (before == 1).sum()
    with pytest.raises(RuntimeError, match='uint8'):
        keep_largest_components(before.astype(np.int16), np.zeros((1, 256), np.uint8), [0])


# ------------------------------------------------------------------------------------------------ end to end
PLAN = [([1, 2], 0), ([1], 0), ([2], 0)]


def labelmap_model(seed=47):
    """A synthetic label-map model (two labels): tests/surface_util.py's, with the dataset of a label-map model."""
    m0, _, _ = synthetic_model('ts2d-v2-ep4000b2_labelmap', 3, seed, feats=(32, 32))
    cfg = dict(m0._config)
    cfg['synthetic'] = dict(cfg['synthetic'], dataset_json=dict(prob_util.DATASETS['labelmap']))
    cfg['param'] = dict(cfg['param'], **{'nnu.result.colors': None})
    return cfg


def case_2d(seed=1):
    a = np.zeros((64, 64, 2), np.float32)
    a[3:61, 2:62] = prng.normal_f32(seed, 0, (58, 60, 2)) * 300
    return nrrd.Image(a, (1.5, 1.5), (3.0, -7.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


def case_stack(seed=2):
    a = np.zeros((6, 64, 64, 2), np.float32)
    a[:, 3:61, 2:62] = prng.normal_f32(seed, 0, (6, 58, 60, 2)) * 40 + 10
    return nrrd.Image(a, (1.5, 1.5, 3.0), (1.0, 2.0, 3.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), 2, {}, 'left-posterior-superior')


def components_per_label(seg, labels):
    return {k: int(ndimage.label(seg.reshape(((1,) + seg.shape)[-3:]) == k, structure=FULL)[1]) for k in labels}


def test_a_label_map_model_with_a_plan_through_apply_and_apply_batch():
    cases = {'flat': case_2d(), 'stack': case_stack()}
    m = HIPModel(labelmap_model())
    assert m.device_postprocessing is True and m.postprocessing is None
    m.start()
    try:
        plain = {k: m.apply(v) for k, v in cases.items()}
        plain_batch = m.apply_batch(dict(cases))
        assert not any(hasattr(im, 'postprocessing') for im in plain.values())
        m.set_postprocessing(PLAN)
        dev = {k: m.apply(v) for k, v in cases.items()}
        assert 'postprocessed' in m.timestamps
        dev_batch = m.apply_batch(dict(cases))
        m.device_postprocessing = False
        host = {k: m.apply(v) for k, v in cases.items()}
        host_batch = m.apply_batch(dict(cases))
    finally:
        m.stop()
    for k in cases:
        base = plain[k].array
        assert base.shape == cases[k].array.shape[:-1] and base.dtype == np.uint8
        # the condition: without the plan some label holds at least two components - else the plan has nothing to do and the test shows nothing
        counts = components_per_label(base, (1, 2))
        print(f'{k}: components per label without the plan: {counts}')
        if max(counts.values()) < 2:
            pytest.fail(f'{k}: no label of the unprocessed map has two components ({counts}): choose another seed')
        want, stats = keep_largest_components_statement(base, PLAN)
        assert stats[:, 3].sum() > 0
        for got, route in ((dev[k], 'device'), (host[k], 'host')):
            assert got.postprocessing['route'] == route and np.array_equal(got.postprocessing['stats'], stats)
            assert np.array_equal(got.array, want) and got.meta == plain[k].meta and got.spacing == plain[k].spacing
        # with the plan every named label has exactly its largest-size components left
        for label in (1, 2):
            lab, n = ndimage.label(want.reshape(((1,) + want.shape)[-3:]) == label, structure=FULL)
            assert n == 0 or len(set(np.bincount(lab.ravel())[1:].tolist())) == 1
        # apply_batch: the two routes agree byte for byte, each is the statement of its own unprocessed map, and it equals apply
        want_batch = keep_largest_components_statement(plain_batch[k].array, PLAN)[0]
        assert dev_batch[k].postprocessing['route'] == 'device' and host_batch[k].postprocessing['route'] == 'host'
        assert np.array_equal(dev_batch[k].array, want_batch) and np.array_equal(host_batch[k].array, want_batch)
        assert np.array_equal(dev_batch[k].array, dev[k].array)
