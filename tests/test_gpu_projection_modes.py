"""ts2d_project_coronal_modes on the MI355X against its host statement, ``image.project`` behind ``image.reorient_image``: every mode and sample
type over extents at the lane, tile and wave edges, permuted and flipped views, the three median variants, the status word, the refusals, and
``TS2D.predict`` of sub-models whose channel names go beyond max / mean, device route against host route."""
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import _lib, image, nrrd
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu
A = os.path.join(GOLDEN, 'assets')
EYE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
PERMUTED = (0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0)       # x <- -j, y <- i, z <- -k
FLIPPED = (-1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0)        # two axes flipped: negative strides
DTYPES = ('int16', 'uint8', 'uint16', 'int32', 'float32')
MODES = ('max', 'min', 'mean', 'median', 'std', 'first', 'slice:middle', 'slice:first', 'depth', 'mip')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _samples(dtype, shape, rng):
    """Random samples with zeros in front of many rays, ties, and the extreme values of the type."""
    n = int(np.prod(shape))
    if dtype == 'float32':
        fi = np.finfo(np.float32)
        a = rng.normal(0, 300, n).astype(np.float32)
        ex = np.array([fi.max, fi.min, fi.tiny, -fi.tiny, 1e-45, -1e-45, -0.0, 0.0], np.float32)
    else:
        ii = np.iinfo(dtype)
        a = rng.integers(max(ii.min, -1100), min(ii.max, 3000) + 1, n).astype(dtype)
        ex = np.array([ii.min, ii.max, ii.min + 1, ii.max - 1, 0, 1], dtype)
    a[rng.random(n) < 0.3] = 0
    a[rng.random(n) < 0.2] = 7                                   # ties
    where = rng.random(n) < 0.05
    a[where] = rng.choice(ex, int(where.sum()))
    return a.reshape(shape)


def _volume(dtype, nz, ny, nx, direction, rng):
    """A volume whose RAI view has the extents (nz, ny, nx)."""
    shape = {EYE: (nz, ny, nx), FLIPPED: (nz, ny, nx), PERMUTED: (nz, nx, ny)}[direction]
    vol = nrrd.Image(_samples(dtype, shape, rng), (1.0, 2.0, 3.0), (5.0, -7.0, 11.0), direction, 1, {}, None)
    return vol


def _statement(vol, modes):
    r = image.reorient_image(vol)
    with np.errstate(over='ignore'):
        return r, {m: image.cast(image.project(r, m, 'coronal'), np.float32).array[:, 0, :] for m in modes}


def _check_planes(vol, got, modes, what):
    r, want = _statement(vol, modes)
    integer = np.issubdtype(vol.array.dtype, np.integer)
    for m in modes:
        g = got[m]
        assert g.size == (r.size[0], 1, r.size[2]) and g.spacing == r.spacing and np.allclose(g.origin, r.origin) and np.allclose(g.direction, r.direction)
        p = g.array[:, 0, :]
        assert p.dtype == np.float32 and p.shape == want[m].shape
        if integer or m == 'std':
            assert np.array_equal(_bits(p), _bits(want[m])), (what, m)          # bit for bit
        else:
            assert np.array_equal(p, want[m]), (what, m)                        # by value: the sign of a zero is unspecified
    return want


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_mode_against_the_statement(dtype):
    """ny over {2, 3, 64, 65, 257}, nx over {1, 63, 64, 65, 130}, nz over {1, 3}; the three directions in turn."""
    rng = np.random.default_rng(DTYPES.index(dtype))
    dirs = (EYE, PERMUTED, FLIPPED)
    k = 0
    for ny in (2, 3, 64, 65, 257):
        for nx in (1, 63, 64, 65, 130):
            for nz in (1, 3):
                vol = _volume(dtype, nz, ny, nx, dirs[k % 3], rng)
                k += 1
                assert image.reorient_image(vol).array.shape == (nz, ny, nx)
                got = image.project_coronal_gpu(vol, modes=list(MODES))
                _check_planes(vol, got, MODES, (ny, nx, nz))
                assert np.array_equal(_bits(got['mip'].array), _bits(got['max'].array)) and np.array_equal(_bits(got['depth'].array), _bits(got['first'].array))


@pytest.mark.parametrize('dtype', DTYPES)
def test_max_and_mean_equal_the_old_entry_and_the_zscore_outputs(dtype):
    """The max and mean planes are those of ts2d_project_coronal bit for bit; out_norm / out_stats / out_box against numpy float64 on the
    STATEMENT's planes (as tests/test_gpu_surface.py::test_device_zscore_behind_the_projection does it), the box per plane."""
    from oracle import input_oracle as IO
    rng = np.random.default_rng(40 + DTYPES.index(dtype))
    modes = ('median', 'max', 'std', 'mean', 'min', 'first', 'slice:0.25')
    for direction, (nz, ny, nx) in ((EYE, (40, 33, 50)), (PERMUTED, (3, 65, 130)), (FLIPPED, (30, 20, 40))):
        vol = _volume(dtype, nz, ny, nx, direction, rng)
        if direction == FLIPPED:                                 # a frame of zero rays: the non-zero boxes are smaller than the plane
            a = vol.array
            a[:5], a[25:], a[:, :, :8], a[:, :, 30:] = 0, 0, 0, 0
        old = image.project_coronal_gpu(vol)
        got = image.project_coronal_gpu(vol, zscore=True, modes=list(modes))
        for m in ('max', 'mean'):
            assert np.array_equal(_bits(got[m].array), _bits(old[m].array)), m
        want = _check_planes(vol, got, modes, direction)
        for m in modes:
            zs = got['zscore'][m]
            assert zs['shape'] == (nz, nx) and zs['norm'].shape == (nz, nx) and zs['norm'].dtype == np.float32
            plane = want[m]
            if not np.isfinite(plane).all() or float(np.abs(plane).max()) > 1e30:
                continue                                          # (float32 extremes: the float32 reference of the z-score overflows)
            ref = IO.zscore(plane)
            assert np.abs(zs['norm'] - ref).max() <= 4e-6 * max(1.0, float(np.abs(ref).max())), m
            mean64, std64 = IO.zscore_stats64(plane)
            assert abs(zs['stats'][0] - mean64) <= 1e-9 * max(1.0, abs(mean64)), m
            assert abs(zs['stats'][1] - std64) <= 1e-9 * max(1.0, std64), m
            rows, cols = np.where((plane != 0).any(1))[0], np.where((plane != 0).any(0))[0]
            assert zs['box'] == ((rows[0], rows[-1], cols[0], cols[-1]) if len(rows) else (nz, -1, nx, -1)), m


MEDIAN_EDGES = {'uint8': (1248, 1249, 4992, 4993), 'int16': (624, 625, 1248, 1249, 2496, 2497), 'uint16': (624, 625, 2496, 2497),
                'int32': (312, 313, 624, 625, 1248, 1249), 'float32': (312, 313, 624, 625, 1248, 1249)}


@pytest.mark.parametrize('dtype', DTYPES)
def test_median_at_the_ray_lengths_where_the_variant_changes(dtype):
    """The longest ray of each tile width (64, 32, 16 columns of keys in LDS) and one sample more; one more than the last - 1249 samples of the
    4-byte types, the documented LDS limit of the widest element - runs the variant that re-reads global memory per key bit."""
    rng = np.random.default_rng(70 + DTYPES.index(dtype))
    for i, ny in enumerate(MEDIAN_EDGES[dtype]):
        vol = _volume(dtype, 2, ny, 70, (EYE, FLIPPED, PERMUTED)[i % 3], rng)
        got = image.project_coronal_gpu(vol, modes=['median', 'std'])
        _check_planes(vol, got, ('median', 'std'), ny)


def _raw(lib, a, nz, ny, nx, strides, base, modes, sidx, planes, norm=None, stats=None, box=None, status=None, n_modes=None, n_elems=None, dtype=0):
    p = lambda x: None if x is None else x.ctypes.data
    return lib.ts2d_project_coronal_modes(0, p(a), a.size if n_elems is None else n_elems, dtype, nz, ny, nx, strides[0], strides[1], strides[2], base,
                                          p(modes), p(sidx), len(modes) if n_modes is None else n_modes, p(planes), p(norm), p(stats), p(box), p(status))


def test_a_ray_above_the_cap_sets_the_status_bit_and_nothing_is_used():
    lib = _lib.load()
    ny = _lib.PROJECT_RAY_CAP + 1
    a = np.ones((1, ny, 2), np.int16)
    modes, sidx = np.array([3, 0], np.int32), np.zeros(2, np.int32)
    planes = np.full((2, 1, 2), -77.0, np.float32); norm = planes.copy(); status = np.full(1, -1, np.int32)
    assert _raw(lib, a, 1, ny, 2, (2 * ny, 2, 1), 0, modes, sidx, planes, norm, None, None, status) == 0
    assert status[0] == _lib.PROJECT_RAY_TOO_LONG and (planes == -77.0).all() and (norm == -77.0).all()
    with pytest.raises(image.ProjectionDeviceRefused) as ei:
        image.project_coronal_gpu(nrrd.Image(a, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), EYE, 1, {}, None), modes=['median'])
    assert ei.value.status == _lib.PROJECT_RAY_TOO_LONG
    ok = np.ones((1, _lib.PROJECT_RAY_CAP, 2), np.int16)         # the cap itself is served
    got = image.project_coronal_gpu(nrrd.Image(ok, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), EYE, 1, {}, None), modes=['median'])
    assert (got['median'].array == 1.0).all()


def test_every_refusal_names_its_argument_and_writes_nothing():
    lib = _lib.load()
    nz, ny, nx = 2, 5, 3
    a = np.arange(nz * ny * nx, dtype=np.int16).reshape(nz, ny, nx)
    st = (ny * nx, nx, 1)
    modes, sidx = np.array([0, 6, 3], np.int32), np.array([0, 2, 0], np.int32)

    def refused(name, **kw):
        planes = np.full((3, nz, nx), -77.0, np.float32); norm = planes.copy()
        stats = np.full((3, 2), -77.0); box = np.full((3, 4), -77, np.int32); status = np.full(1, -77, np.int32)
        args = dict(a=a, nz=nz, ny=ny, nx=nx, strides=st, base=0, modes=modes, sidx=sidx, planes=planes, norm=norm, stats=stats, box=box, status=status)
        args.update(kw)
        rc = _raw(lib, **args)
        assert rc == -1, name                                     # TS2D_ERR_INVALID
        msg = _lib.last_error()
        assert 'ts2d_project_coronal_modes' in msg and name in msg, (name, msg)
        assert (planes == -77.0).all() and (norm == -77.0).all() and (stats == -77.0).all() and (box == -77).all() and status[0] == -77, name

    refused('volume', a=None, n_elems=a.size)
    refused('modes', modes=None, n_modes=3)
    refused('slice_index', sidx=None)
    refused('out_planes', planes=None)
    refused('status', status=None)
    refused('out_norm', norm=None)                                # statistics or boxes without the normalised planes
    refused('modes[1]', modes=np.array([0, 7, 3], np.int32))
    refused('modes[2]', modes=np.array([0, 6, -1], np.int32))
    refused('slice_index[1]', sidx=np.array([0, ny, 0], np.int32))
    refused('slice_index[1]', sidx=np.array([0, -1, 0], np.int32))
    refused('n_modes', n_modes=0)
    refused('n_modes', n_modes=17)
    refused('nz', nz=0)
    refused('ny', ny=0)
    refused('nx', nx=-1)
    refused('dtype', dtype=5)
    refused('leaves the buffer', n_elems=a.size - 1)
    refused('leaves the buffer', base=1)
    refused('leaves the buffer', strides=(ny * nx, -nx, 1))
    refused('std', ny=1, modes=np.array([0, 4, 3], np.int32), sidx=np.zeros(3, np.int32))
    # ... and the same call without a fault is served
    planes = np.empty((3, nz, nx), np.float32); status = np.zeros(1, np.int32)
    assert _raw(lib, a, nz, ny, nx, st, 0, modes, sidx, planes, status=status) == 0 and status[0] == 0
    assert np.array_equal(planes[0], a.max(1)) and np.array_equal(planes[1], a[:, 2]) and np.array_equal(planes[2], np.sort(a, 1)[:, ny // 2])


# ------------------------------------------------------------------------------------------------ TS2D.predict
SIBLING = ('mean', 'max')


def _predict(models, asset, host=False):
    with TS2D(models=models) as ts:
        assert ts._gpu_projection                                # HIP engines behind every model: the device route is the default
        if host:
            ts._gpu_projection = False
        r = ts.predict(asset)
        return ({m: r.get_segmentation(m).array.copy() for m in r.models}, r.get_segmentation().array.copy(),
                {k: v.array.copy() for k, v in r.get_projection().items()})


@pytest.fixture
def device_calls(monkeypatch):
    """The ``modes`` argument of every ``image.project_coronal_gpu`` call, in order (None: the (max, mean) entry)."""
    calls, real = [], image.project_coronal_gpu

    def spy(img, device=0, zscore=False, modes=None):
        calls.append(None if modes is None else tuple(modes))
        return real(img, device, zscore=zscore, modes=modes)
    monkeypatch.setattr(image, 'project_coronal_gpu', spy)
    return calls


def _models(spec):
    return {mid: synthetic_model(mid, K, seed, channels=ch, patch=(64, 64), mirror=False)[0] for mid, (K, seed, ch) in spec.items()}


@pytest.fixture(scope='module')
def sibling_alone():
    """The bytes of the ordinary (mean, max) sub-model when it is the only one of its TS2D, per model id: computed once, never changed."""
    done = {}

    def get(mid):
        if mid not in done:
            seg, _, _ = _predict(_models({mid: (3, 61, SIBLING)}), os.path.join(A, 'sample_s0521.nrrd'))
            seg[mid].setflags(write=False)
            done[mid] = seg[mid]
        return done[mid]
    return get


@pytest.mark.parametrize('channels,new_first', [(('median', 'std'), False), (('min', 'first'), True), (('slice:middle', 'max'), False)])
def test_predict_with_mode_channels_device_route_equals_host_route(channels, new_first, sibling_alone, device_calls):
    """A sub-model whose channel names are projection modes beyond max / mean beside an ordinary (mean, max) sibling, on the 3-D sample: the device
    route (ts2d_project_coronal_modes, z-score on the device) against the host route (``_gpu_projection`` off): byte-identical segmentations, equal
    projections; the sibling's bytes are those of a TS2D that holds it alone.  (On the parent commit: ``Unsupported filter mode: median``.)"""
    asset = os.path.join(A, 'sample_s0521.nrrd')
    ids = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_ribs')
    new_id, sib_id = ids if new_first else ids[::-1]
    spec = {new_id: (4, 62, channels), sib_id: (3, 61, SIBLING)}
    sibling_bytes = sibling_alone(sib_id)
    del device_calls[:]
    dev_seg, dev_merged, dev_proj = _predict(_models(spec), asset)
    # the sibling makes exactly the call it makes alone, the other sub-model one call of the new entry for its own names
    new_call = tuple(dict.fromkeys(channels))
    assert device_calls == ([new_call, None] if new_first else [None, new_call])
    host_seg, host_merged, host_proj = _predict(_models(spec), asset, host=True)
    assert len(device_calls) == 2                                # the host route makes none
    assert sorted(dev_seg) == sorted(ids)
    for m in ids:
        assert dev_seg[m].dtype == np.uint8 and np.array_equal(dev_seg[m], host_seg[m]), m
    assert np.array_equal(dev_merged, host_merged) and dev_merged.any()
    assert sorted(dev_proj) == sorted(host_proj) == sorted(set(channels) | set(SIBLING))
    for name in dev_proj:
        assert dev_proj[name].dtype == np.float32 and np.array_equal(dev_proj[name], host_proj[name]), name
    assert np.array_equal(dev_seg[sib_id], sibling_bytes)


def test_a_float_volume_with_a_nan_takes_the_host_route(device_calls):
    v = nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))
    a = v.array.astype(np.float32)
    a[a.shape[0] // 2, a.shape[1] // 2, a.shape[2] // 2] = np.nan          # deep inside: every ray has non-zero samples before it
    vol = nrrd.Image(a, v.spacing, v.origin, v.direction, 1, dict(v.meta), v.space)
    with pytest.raises(image.ProjectionDeviceRefused) as ei:
        image.project_coronal_gpu(vol, zscore=True, modes=['median', 'first'])
    assert ei.value.status == _lib.PROJECT_NONFINITE
    finite = nrrd.Image(np.nan_to_num(a), v.spacing, v.origin, v.direction, 1, dict(v.meta), v.space)
    assert 'median' in image.project_coronal_gpu(finite, zscore=True, modes=['median', 'first'])      # the same volume without it is served
    spec = {'ts2d-v2-ep4000b2_ribs': (4, 62, ('median', 'first'))}
    del device_calls[:]
    dev_seg, _, dev_proj = _predict(_models(spec), vol)
    assert device_calls == [('median', 'first')]                  # asked once, refused, answered on the host
    host_seg, _, host_proj = _predict(_models(spec), vol, host=True)
    for m in dev_seg:
        assert np.array_equal(dev_seg[m], host_seg[m])
    for name in ('median', 'first'):
        assert np.isfinite(dev_proj[name]).all() and np.array_equal(dev_proj[name], host_proj[name])
