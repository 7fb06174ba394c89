"""The synthetic radiograph without a GPU: the statements of totalsegmentator2d_amd/xray.py against an independent scalar loop per ray
(tests/xray_util.py) bit for bit, closed forms, the geometry and the refusals, TS2D / Result / the command line on the host route, and the
planner of csrc/prep_plan.cpp as plain C++ under the sanitizers (tests/xr_driver.cpp) against xr_tables bit for bit."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.batch_util import synthetic_batch_model
from tests.conftest import GOLDEN, ROOT
from tests.xray_util import EXTENTS, SPACING, as_image, ct_volume, detector, label_volume, per_ray
from totalsegmentator2d_amd import evaluate as E, image, main, nrrd, xray as X
from totalsegmentator2d_amd.main import ts2d_run
from totalsegmentator2d_amd.tool import TS2D

HIPCC = '/opt/rocm/bin/hipcc'
A = os.path.join(GOLDEN, 'assets')
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
BEAMS = [dict(view=v, parallel=p) for v in ('ap', 'pa') for p in (False, True)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _render(vol, geometry=None, spacing=SPACING):
    tb = X.xr_tables(vol.shape, spacing, geometry)
    s = X.synthetic_xr_statement(vol, tb)
    return s, (s * tb['step']).astype(np.float32), tb


# ------------------------------------------------------------------------------------------------ 1. the statement
@pytest.mark.parametrize('shape', EXTENTS)
def test_statement_against_the_per_ray_loop(shape):
    for n, beam in enumerate(BEAMS):
        for dtype in ('int16', 'float32') if n % 2 else ('uint8', 'int32'):
            vol = ct_volume(shape, dtype, 380 + n)
            s, xr, _ = _render(vol, X.XRGeometry(**beam))
            rs, rx = per_ray(vol, SPACING, **beam)
            assert s.dtype == np.float64 and s.shape == rs.shape and (_bits(s) == _bits(rs)).all(), (shape, beam, dtype)
            assert (_bits(xr) == _bits(rx)).all()
    vol = ct_volume(shape, 'int16', 390)                                         # ... and with every option set
    opt = dict(sdd=70.0, sod=40.0, view='pa', du=0.7, dv=2.6, size=(31, 5), air=-900.0, water=100.0, density_max=1.75)
    g = X.XRGeometry(source_detector_mm=70.0, source_center_mm=40.0, view='pa', detector_spacing=(0.7, 2.6), detector_size=(31, 5), air=-900.0,
                     water=100.0, density_max=1.75)
    s, xr, _ = _render(vol, g)
    rs, rx = per_ray(vol, SPACING, **opt)
    assert (_bits(s) == _bits(rs)).all() and (_bits(xr) == _bits(rx)).all()


def test_parallel_render_of_multiples_of_125_is_the_closed_form():
    rng = np.random.default_rng(381)
    vol = (rng.integers(-10, 21, (6, 150, 17)) * 125).astype(np.int16)            # (v + 1000) / 1000 is a multiple of 1 / 8: every sum is exact
    for view in ('ap', 'pa'):
        s, xr, tb = _render(vol, X.XRGeometry(parallel=True, view=view))
        closed = np.maximum(vol.astype(np.int64) + 1000, 0).sum(axis=1) / 1000
        assert s.shape == (6, 17) and (s == closed).all() and (tb['step'] == SPACING[1]).all()
        assert (xr == (closed * SPACING[1]).astype(np.float32)).all()


def test_uniform_water_under_a_cone_beam():
    ny = 37
    vol = np.zeros((21, ny, 66), np.int16)                                        # water: density 1 everywhere
    s, _, tb = _render(vol)
    g = tb['geometry']
    # a ray is interior when all its samples lie in [0, nx - 1] x [0, nz - 1]: the largest |t| is t[ny - 1], the smallest t[0]
    x_far, z_far = tb['cx'] + tb['t'][-1] * tb['a'], tb['cz'] + tb['t'][-1] * tb['b']
    x_near, z_near = tb['cx'] + tb['t'][0] * tb['a'], tb['cz'] + tb['t'][0] * tb['b']
    ix = (np.minimum(x_far, x_near) >= 0) & (np.maximum(x_far, x_near) <= 65)
    kz = (np.minimum(z_far, z_near) >= 0) & (np.maximum(z_far, z_near) <= 20)
    interior = s[np.ix_(kz, ix)]
    assert interior.size > 500
    # each sample is a few rounded operations on weights that sum to 1 within an ulp
    assert (np.abs(interior - ny) <= ny * ny * 8 * 2.0 ** -53).all()
    big = X.XRGeometry(detector_size=(g['nu'] + 40, g['nv'] + 40))
    s2, xr2, tb2 = _render(vol, big)
    x_out = (tb2['cx'] + tb2['t'][0] * tb2['a'] <= -1) | (tb2['cx'] + tb2['t'][0] * tb2['a'] >= 66)      # outside at the NEAREST plane: outside at all
    assert x_out.sum() >= 10 and (_bits(s2[:, x_out]) == 0).all() and (_bits(xr2[:, x_out]) == 0).all()      # exactly +0.0
    assert (s2[20:-20, 20:-20] == s).all()                                        # the same rays, the same sums


def test_density_hand_cases():
    vol = np.array([[[-2000, -1000, -500, 0, 1000, 3000]]], np.int16)            # one row, one plane: a parallel ray per sample
    par = dict(parallel=True)
    assert _render(vol, X.XRGeometry(**par))[0].tolist() == [[0.0, 0.0, 0.5, 1.0, 2.0, 4.0]]
    assert _render(vol, X.XRGeometry(density_max=1.5, **par))[0].tolist() == [[0.0, 0.0, 0.5, 1.0, 1.5, 1.5]]
    assert _render(vol, X.XRGeometry(air=0.0, water=1000.0, **par))[0].tolist() == [[0.0, 0.0, 0.0, 0.0, 1.0, 3.0]]
    assert _render(vol, X.XRGeometry(air=0.0, water=-1000.0, **par))[0].tolist() == [[2.0, 1.0, 0.5, 0.0, 0.0, 0.0]]      # a falling scale
    assert _render(vol, X.XRGeometry(**par), spacing=(1.0, 2.5, 1.0))[1].tolist() == [[0.0, 0.0, 1.25, 2.5, 5.0, 10.0]]  # millimetres of water
    assert (_bits(_render(vol, X.XRGeometry(**par))[0][0, :2]) == 0).all()                                                  # +0.0, not -0.0
    half = np.array([[[0, 1000]]], np.int16)                                     # densities 1 and 2, one pixel between them: the bilinear mean
    s = _render(half, X.XRGeometry(parallel=False, detector_size=(1, 1), source_detector_mm=10.0, source_center_mm=5.0), spacing=(1.0, 1.0, 1.0))[0]
    assert s.tolist() == [[1.5]]


def test_a_detector_much_larger_than_the_volume_and_one_of_a_single_pixel():
    vol = ct_volume((3, 2, 63), 'int16', 382)
    for size in ((400, 90), (1, 1), (1, 7), (9, 1)):
        g = X.XRGeometry(detector_size=size, view='pa')
        s, xr, _ = _render(vol, g)
        rs, rx = per_ray(vol, SPACING, view='pa', size=size)
        assert s.shape == (size[1], size[0]) and (_bits(s) == _bits(rs)).all() and (_bits(xr) == _bits(rx)).all()
    assert (_render(vol, X.XRGeometry(detector_size=(400, 90)))[0][:, :100] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. geometry, labels, refusals
def test_default_detector_size_and_tables():
    for shape, spacing, sdd, sod in (((5, 37, 66), SPACING, 1800.0, 1500.0), ((53, 120, 133), (1.5, 1.5, 1.5), 1800.0, 1500.0),
                                     ((4, 3, 10), (0.7, 1.0, 3.0), 1000.0, 300.0), ((1, 1, 1), (1.0, 1.0, 1.0), 2.0, 1.0)):
        g = X.XRGeometry(source_detector_mm=sdd, source_center_mm=sod).resolve(shape, spacing)
        nz, ny, nx = shape
        assert (g['nu'], g['nv']) == (math.ceil(nx * spacing[0] * (sdd / sod) / spacing[0]), math.ceil(nz * spacing[2] * (sdd / sod) / spacing[2]))
        assert (g['du'], g['dv'], g['nu'], g['nv']) == detector(shape, spacing, sdd, sod)
    assert X.XRGeometry().resolve((5, 37, 66), SPACING)['nu'] == 80 and X.XRGeometry(detector_spacing=(3.0, 1.0)).resolve((5, 37, 66), SPACING)['nu'] == 40
    g = X.XRGeometry(parallel=True).resolve((5, 37, 66), SPACING)
    assert (g['du'], g['dv'], g['nu'], g['nv']) == (1.5, 2.0, 66, 5)
    tb = X.xr_tables((5, 37, 66), SPACING)
    assert tb['t'].shape == (37,) and (tb['t'] > 0).all() and (tb['t'] <= 1).all() and (np.diff(tb['t']) > 0).all()
    assert tb['a'].shape == tb['cx'].shape == (80,) and tb['b'].shape == tb['cz'].shape == (6,) and tb['step'].shape == (6, 80)
    assert (tb['cx'] == 32.5).all() and (tb['cz'] == 2.0).all() and (tb['a'] == -tb['a'][::-1]).all() and (tb['step'] >= SPACING[1]).all()
    # the detector plane may lie on the last plane centre (t = 1 there), not inside the slab
    edge = X.xr_tables((5, 37, 66), SPACING, X.XRGeometry(source_center_mm=100.0, source_detector_mm=113.5))
    assert edge['t'][-1] == 1.0
    pt = X.xr_tables((5, 37, 66), SPACING, X.XRGeometry(parallel=True))
    assert (pt['t'] == 0).all() and (pt['cx'] == np.arange(66)).all() and (pt['cz'] == np.arange(5)).all() and (pt['step'] == 0.75).all()


def test_geometry_of_the_returned_image():
    vol = ct_volume((5, 37, 66), 'int16', 383)
    for order, flip in (((0, 1, 2), (False, False, False)), ((2, 0, 1), (True, False, True)), ((1, 2, 0), (False, True, False))):
        img = as_image(vol, flip=flip, order=order)
        out = X.synthetic_xr(img)
        assert out.size == (80, 1, 6) and out.array.dtype == np.float32 and out.array.shape == (6, 1, 80) and out.components == 1
        assert out.spacing == (1.5, 0.75, 2.0) and out.meta == img.meta and out.meta is not img.meta
        re = image.reorient_image(img)
        assert out.direction == re.direction and np.allclose(re.direction, np.eye(3).reshape(-1))
        tb = X.xr_tables(vol.shape, SPACING)
        u0, v0 = 32.5 * 1.5 - 39.5 * 1.5, 2.0 * 2.0 - 2.5 * 2.0                  # U_0 = Cx - (nu - 1) / 2 du, V_0 likewise
        assert (tb['u0'], tb['v0']) == (u0, v0)
        assert np.allclose(out.origin, np.asarray(re.origin) + np.array([u0, 0.0, v0]), rtol=0, atol=1e-12)
        assert (_bits(out.array.reshape(6, 80)) == _bits(_render(vol)[1])).all()
        big = X.synthetic_xr(img, X.XRGeometry(detector_spacing=(3.0, 4.0), detector_size=(10, 4)))
        assert big.spacing == (3.0, 0.75, 4.0) and big.size == (10, 1, 4)
        lab = X.project_labels_xr(as_image(label_volume(vol.shape, 3, 384), flip=flip, order=order), 3)
        assert lab.size == out.size and lab.spacing == out.spacing and lab.origin == out.origin and lab.direction == out.direction
        assert lab.components == 3 and lab.array.shape == (6, 1, 80, 3) and lab.array.dtype == np.uint8
    with pytest.raises(ValueError, match='scalar 3-D volume'):
        X.synthetic_xr(nrrd.Image(np.zeros((4, 5), np.int16), (1.0, 1.0), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 1, {}, None))
    with pytest.raises(TypeError, match='XRGeometry'):
        X.synthetic_xr(as_image(vol), geometry={'view': 'ap'})


@pytest.mark.parametrize('shape', EXTENTS)
def test_label_statement_against_the_per_ray_loop(shape):
    for n, beam in enumerate(BEAMS):
        num = (1, 3, 70, 255)[n]
        vol = label_volume(shape, num, 385 + n, ('uint8', 'int16', 'uint16', 'int32')[n])
        tb = X.xr_tables(shape, SPACING, X.XRGeometry(**beam))
        got = X.project_labels_xr_statement(vol, num, tb)
        assert got.dtype == np.uint8 and got.shape == (num, tb['geometry']['nv'], tb['geometry']['nu'])
        assert (got == per_ray(vol, SPACING, num=num, **beam)).all(), (shape, beam)
    vol = label_volume(shape, 5, 389, 'uint8')
    g = X.XRGeometry(source_detector_mm=70.0, source_center_mm=40.0, detector_spacing=(0.7, 2.6), detector_size=(200, 5))
    assert (X.project_labels_xr_statement(vol, 5, X.xr_tables(shape, SPACING, g)) == per_ray(vol, SPACING, num=5, sdd=70.0, sod=40.0, du=0.7, dv=2.6,
                                                                                              size=(200, 5))).all()


def test_parallel_label_projection_is_project_labels():
    for order, flip in (((0, 1, 2), (False, False, False)), ((2, 1, 0), (True, True, False))):
        for num in (1, 4, 40):
            img = as_image(label_volume((7, 9, 130), num, 386, 'int16'), flip=flip, order=order)
            want = E.project_labels(image.reorient_image(img), num, 'coronal')
            for view in ('ap', 'pa'):
                got = X.project_labels_xr(img, num, X.XRGeometry(parallel=True, view=view))
                assert got.array.shape == want.array.shape and got.array.tobytes() == want.array.tobytes() and got.components == want.components
                assert got.spacing == want.spacing and got.size == want.size and np.allclose(got.origin, want.origin) and got.direction == want.direction


def test_every_refusal_by_name():
    shape = (5, 9, 66)                                                           # half depth 8 * 0.75 / 2 = 3 mm
    nan, inf = float('nan'), float('inf')
    for kw, text in [(dict(source_detector_mm=0.0), 'source_detector_mm = 0.0 is not finite and positive'), (dict(source_detector_mm=inf), 'source_detector_mm'),
                     (dict(source_center_mm=-1.0), 'source_center_mm'), (dict(source_center_mm=nan), 'source_center_mm'),
                     (dict(detector_spacing=(0.0, 1.0)), 'detector_spacing du'), (dict(detector_spacing=(1.0, inf)), 'detector_spacing dv'),
                     (dict(source_center_mm=3.0), 'source inside the slab'), (dict(source_center_mm=1.0), 'source inside the slab'),
                     (dict(source_center_mm=1500.0, source_detector_mm=1502.5), 'detector inside the slab'),
                     (dict(source_center_mm=1500.0, source_detector_mm=1000.0), 'detector inside the slab'),
                     (dict(detector_size=(65536, 32768)), 'more than 2^31 - 1 pixels'), (dict(detector_size=(0, 4)), 'below 1'),
                     (dict(water=-1000.0), 'water == air'), (dict(air=5.0, water=5.0), 'water == air'), (dict(air=nan), 'not finite'),
                     (dict(density_max=nan), 'density_max'), (dict(density_max=-1.0), 'density_max'), (dict(view='lateral'), "neither 'ap' nor 'pa'"),
                     (dict(parallel=True, detector_size=(10, 10)), 'parallel rays fix detector_size'),
                     (dict(parallel=True, detector_spacing=(1.0, 1.0)), 'parallel rays fix detector_spacing')]:
        with pytest.raises(ValueError, match='synthetic_xr: .*' + text.replace('^', r'\^').replace('(', r'\(').replace(')', r'\)')):
            X.xr_tables(shape, SPACING, X.XRGeometry(**kw))
    for spacing, text in (((0.0, 1.0, 1.0), 'spacing sx'), ((1.0, -2.0, 1.0), 'spacing sy'), ((1.0, 1.0, nan), 'spacing sz'), ((inf, 1.0, 1.0), 'spacing sx')):
        with pytest.raises(ValueError, match=text):
            X.xr_tables(shape, spacing)
    with pytest.raises(ValueError, match='extents'):
        X.xr_tables((0, 9, 66), SPACING)
    X.xr_tables(shape, SPACING, X.XRGeometry(source_center_mm=3.0 + 2.0 ** -40, source_detector_mm=6.0 + 2.0 ** -40))      # the limits are served
    X.xr_tables(shape, SPACING, X.XRGeometry(parallel=True, detector_size=(66, 5), detector_spacing=(1.5, 2.0)))
    tb = X.xr_tables(shape, SPACING)
    with pytest.raises(ValueError, match='shape'):
        X.synthetic_xr_statement(np.zeros((5, 9, 65), np.int16), tb)
    with pytest.raises(ValueError, match='shape'):
        X.project_labels_xr_statement(np.zeros((5, 9, 65), np.uint8), 3, tb)


@pytest.mark.parametrize('bad', (np.nan, np.inf, -np.inf))
def test_a_non_finite_sample_is_refused(bad):
    vol = ct_volume((5, 9, 66), 'float32', 387)
    vol[4, 8, 65] = bad
    with pytest.raises(ValueError, match='non-finite'):
        X.synthetic_xr_statement(vol, X.xr_tables(vol.shape, SPACING))
    with pytest.raises(ValueError, match='non-finite'):
        X.synthetic_xr(as_image(vol))


def test_label_range_num_and_type():
    tb = X.xr_tables((5, 9, 66), SPACING)
    for dtype, bad in (('uint8', 4), ('int16', -1), ('int32', 70000)):
        vol = label_volume((5, 9, 66), 3, 388, dtype)
        vol[0, 0, 0] = bad
        with pytest.raises(ValueError, match=r'project_labels: the volume holds samples outside 0 \.\.\. 3'):
            X.project_labels_xr_statement(vol, 3, tb)
        with pytest.raises(ValueError, match=r'outside 0 \.\.\. 3'):
            X.project_labels_xr(as_image(vol), 3)
    good = label_volume((5, 9, 66), 3, 388)
    for num in (0, 256, -1):
        with pytest.raises(ValueError, match='outside 1 ... 255'):
            X.project_labels_xr_statement(good, num, tb)
    with pytest.raises(ValueError, match='integer type'):
        X.project_labels_xr_statement(good.astype(np.float32), 3, tb)


def test_the_device_probes_ask_for_the_symbols(monkeypatch):
    from totalsegmentator2d_amd import engine
    img, lab = as_image(ct_volume((2, 3, 4), 'float32', 1)), as_image(label_volume((2, 3, 4), 3, 1))
    asked = []
    monkeypatch.setattr(engine, 'has_entry', lambda *names: asked.append(names) or False)
    assert not X.device_renders(img) and not X.device_projects_labels(lab) and asked == [('ts2d_project_xr',), ('ts2d_project_labels_xr',)]
    monkeypatch.setattr(engine, 'has_entry', lambda *names: True)
    assert X.device_renders(img) and X.device_projects_labels(lab) and not X.device_projects_labels(img)
    assert not X.device_renders(as_image(np.zeros((2, 3, 4), np.float64)))
    monkeypatch.setattr(engine, 'has_entry', lambda *names: False)               # a library without the entries: the host route, the same bytes
    assert X.synthetic_xr(img, device=0).array.tobytes() == X.synthetic_xr(img).array.tobytes()
    assert X.project_labels_xr(lab, 3, device=0).array.tobytes() == X.project_labels_xr(lab, 3).array.tobytes()


def test_the_size_gate_keeps_a_few_planes_on_the_host(monkeypatch):
    from totalsegmentator2d_amd import engine
    calls = []
    monkeypatch.setattr(engine, 'has_entry', lambda *names: True)
    monkeypatch.setattr(engine, 'project_xr', lambda *a, **kw: calls.append('xr') or (None, np.zeros((a[4]['nv'], a[4]['nu']), np.float32), 0))
    monkeypatch.setattr(engine, 'project_labels_xr', lambda *a, **kw: calls.append('labels') or (np.zeros((a[4], a[5]['nv'], a[5]['nu']), np.uint8), 0))
    for ny, want in ((1, []), (4, []), (6, ['xr']), (8, ['xr']), (12, ['xr', 'labels']), (37, ['xr', 'labels'])):      # a detector of 80 x 6 pixels
        calls.clear()
        X.synthetic_xr(as_image(ct_volume((5, ny, 66), 'int16', 392)), device=0)
        X.project_labels_xr(as_image(label_volume((5, ny, 66), 3, 393)), 3, device=0)
        assert calls == want, (ny, calls)
    for ny, want in ((1, ['xr']), (2, ['xr', 'labels'])):                        # 240 x 120 pixels: one plane is enough for the radiograph
        calls.clear()
        X.synthetic_xr(as_image(ct_volume((100, ny, 200), 'int16', 392)), device=0)
        X.project_labels_xr(as_image(label_volume((100, ny, 200), 3, 393)), 3, device=0)
        assert calls == want, (ny, calls)
    g = X.XRGeometry().resolve((5, 4, 66), SPACING)
    assert X.host_is_faster('xr', g) and X.host_is_faster('labels', g) and not X.host_is_faster('xr', dict(g, shape=(5, 6, 66)))


# ------------------------------------------------------------------------------------------------ 3. TS2D, Result, the command line (host route)
MID = 'ts2d-v2-ep4000b2_cardiac'


@pytest.fixture(scope='module')
def xr_model():
    m, _, _ = synthetic_batch_model(MID, 3, 31, channels=('xray',), mirror=False, feats=(32, 32))
    return {MID: m}


@pytest.fixture(scope='module')
def projected_model():
    m, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_ribs', 4, 32, mirror=False, feats=(32, 32))     # channels (mean, max)
    return {'ts2d-v2-ep4000b2_ribs': m}


def reference_volume(seed=61):
    case = nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))
    rng = np.random.default_rng(seed)
    lab = np.zeros(case.array.shape, np.int16)
    for v in range(1, 4):
        lo = [int(rng.integers(0, s // 2)) for s in lab.shape]
        lab[tuple(slice(o, o + int(rng.integers(3, s // 2))) for o, s in zip(lo, lab.shape))] = v
    return nrrd.Image(lab, case.spacing, case.origin, case.direction, 1, {}, case.space)


def test_predict_evaluate_and_save_on_a_synthetic_radiograph(tmp_path, xr_model):
    case = nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))
    vol = reference_volume()
    with TS2D(models=dict(xr_model), synthetic_xr=True) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device is None and list(res.get_projection()) == ['xray']
        xr = res.get_projection('xray')
        want = X.synthetic_xr(case)
        assert xr.array.tobytes() == want.array.tobytes() and xr.size == want.size == (64, 1, 160) and xr.spacing == (1.5, 1.5, 1.5)
        seg = res.get_segmentation()
        assert seg.size == xr.size and seg.components == 3 and seg.spacing == xr.spacing and seg.origin == xr.origin
        assert res.data['models'][MID]['xr_geometry'] == X.XRGeometry() and res.get_input(MID).array.tobytes() == xr.array.tobytes()
        ref2d = X.project_labels_xr(vol, 3)                                      # a 3-D label volume goes through the radiograph's rays
        ev = res.evaluate(vol)
        assert ev == E.evaluate(seg, ref2d) == res.evaluate(ref2d) == res.evaluate(vol, model=MID)
        assert sum(e['count_ref'] for e in ev.values()) == int(ref2d.array.sum()) > 0
        assert res.confusion(vol) == E.confusion(seg, ref2d)
        coronal = E.project_labels(image.reorient_image(vol), 3, 'coronal')      # ... not through the coronal projection: another grid
        assert coronal.size != ref2d.size
        files = res.save(str(tmp_path / 'out'), name='case', content='file', targets=['segmentation', 'projection'])
        assert sorted(os.path.basename(f) for f in files) == ['case.seg.nrrd', 'case_xray.nrrd']
        assert nrrd.read(str(tmp_path / 'out' / 'case_xray.nrrd')).array.tobytes() == xr.array.tobytes()
        both = res.save(str(tmp_path / 'vis'), name='case', targets=['projection'])
        assert sorted(os.path.basename(f) for f in both) == ['case_xray.nrrd', 'case_xray.png']
        assert res.cleaned(keep_largest=True).evaluate(vol).keys() == ev.keys()    # the geometry travels with a cleaned result
        many = ts.predict_many([case, case], max_cases=2)
        assert all(r.get_projection('xray').array.tobytes() == xr.array.tobytes() and r.evaluate(vol) == many[0].evaluate(vol) for r in many)
    pa = X.XRGeometry(view='pa', source_center_mm=1000.0)
    with TS2D(models=dict(xr_model), synthetic_xr=pa, synthetic_xr_channels=('XRAY ',)) as ts:      # a geometry of the caller's; names are matched lower-case
        res = ts.predict(case)
        assert res.get_projection('xray').array.tobytes() == X.synthetic_xr(case, pa).array.tobytes() != xr.array.tobytes()
        assert res.evaluate(vol) == E.evaluate(res.get_segmentation(), X.project_labels_xr(vol, 3, pa))
    with TS2D(models=dict(xr_model), synthetic_xr=True, synthetic_xr_channels=('xr',)) as ts:       # 'xray' is no radiograph channel here
        with pytest.raises(RuntimeError, match='Unsupported filter mode'):
            ts.predict(case)


def test_without_the_option_nothing_changes(xr_model, projected_model):
    case = os.path.join(A, 'sample_s0521.nrrd')
    for kw in ({}, {'synthetic_xr': None}, {'synthetic_xr': False}):
        with TS2D(models=dict(xr_model), **kw) as ts:
            with pytest.raises(RuntimeError, match='Unsupported filter mode: xray'):
                ts.predict(case)
    with TS2D(models=dict(projected_model)) as ts:
        plain = ts.predict(case)
    with TS2D(models=dict(projected_model), synthetic_xr=True) as ts:            # a (max, mean) model with the option: equal bytes
        same = ts.predict(case)
    assert list(plain.get_projection()) == list(same.get_projection()) and 'xr_geometry' not in same.data['models']['ts2d-v2-ep4000b2_ribs']
    for n in plain.get_projection():
        assert plain.get_projection(n).array.tobytes() == same.get_projection(n).array.tobytes()
    assert plain.get_segmentation().array.tobytes() == same.get_segmentation().array.tobytes()
    vol = reference_volume()
    assert plain.evaluate(vol) == same.evaluate(vol)


def test_mixed_sub_models_and_mixed_channels(xr_model, projected_model):
    case = nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))
    vol = reference_volume()
    both = dict(xr_model, **projected_model)
    with TS2D(models=both, synthetic_xr=True) as ts:
        with pytest.raises(RuntimeError, match='different grids: there is no merged segmentation'):
            ts.predict(case)
        res = ts.predict(case, merge=False)
        assert sorted(res.get_projection()) == ['max', 'mean', 'xray']
        ribs = 'ts2d-v2-ep4000b2_ribs'
        assert res.evaluate(vol, model=MID) == E.evaluate(res.get_segmentation(MID), X.project_labels_xr(vol, 3))
        assert res.evaluate(vol, model=ribs) == E.evaluate(res.get_segmentation(ribs), E.project_labels(image.reorient_image(vol), 4, 'coronal'))
    with TS2D(models=both, synthetic_xr=X.XRGeometry(parallel=True)) as ts:      # parallel rays: one grid, a merged segmentation - but no one projection
        res = ts.predict(case)
        assert res.get_segmentation().components == 7
        with pytest.raises(ValueError, match='mixes sub-models on synthetic radiographs'):
            res.evaluate(vol)
        assert res.evaluate(vol, model=MID) == E.evaluate(res.get_segmentation(MID), E.project_labels(image.reorient_image(vol), 3, 'coronal'))
    m, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_spine', 2, 33, channels=('xray', 'max'), mirror=False, feats=(32, 32))
    with TS2D(models={'ts2d-v2-ep4000b2_spine': m}, synthetic_xr=True) as ts:    # one sub-model, two grids
        with pytest.raises(RuntimeError, match='ts2d-v2-ep4000b2_spine mixes synthetic radiographs and projections on different grids'):
            ts.predict(case)
    m, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_spine', 2, 33, channels=('xray', 'max'), mirror=False, feats=(32, 32))
    with TS2D(models={'ts2d-v2-ep4000b2_spine': m}, synthetic_xr=X.XRGeometry(parallel=True)) as ts:
        res = ts.predict(case)
        assert res.get_input('ts2d-v2-ep4000b2_spine').components == 2 and sorted(res.get_projection()) == ['max', 'xray']


def test_cli_synthetic_xr(tmp_path, xr_model, monkeypatch, capsys):
    src = tmp_path / 'one.nrrd'
    shutil.copy(os.path.join(A, 'sample_s0521.nrrd'), src)
    ref = tmp_path / 'ref.nrrd'
    nrrd.write(reference_volume(), str(ref), True)
    ts2d_run(str(src), str(tmp_path / 'a'), models=dict(xr_model), visualize=False, silent=True, reference=str(ref), synthetic_xr=True)
    assert sorted(os.listdir(tmp_path / 'a')) == ['one.evaluation.json', 'one.seg.nrrd', 'one_xray.nrrd']
    with open(tmp_path / 'a' / 'one.evaluation.json') as f:
        ev = json.load(f)
    with TS2D(models=dict(xr_model), synthetic_xr=True) as ts:
        assert ev == json.loads(json.dumps(ts.predict(str(src)).evaluate(str(ref))))
    with pytest.raises(RuntimeError, match='Unsupported filter mode'):
        ts2d_run(str(src), str(tmp_path / 'b'), models=dict(xr_model), visualize=False, silent=True)
    for argv in (['--xr-view', 'pa'], ['--xr-parallel'], ['--xr-source-detector', '1000'], ['--xr-source-center', '900']):
        with pytest.raises(SystemExit):                                          # an --xr-* flag alone is an argument error
            main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e')] + argv)
        assert '--synthetic-xr' in capsys.readouterr().err and not os.path.exists(tmp_path / 'e')
    with pytest.raises(SystemExit):
        main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--synthetic-xr', '--xr-view', 'lateral'])
    capsys.readouterr()
    seen = {}
    monkeypatch.setattr(main, 'ts2d_run', lambda **kw: seen.update(kw))
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--synthetic-xr'])
    assert seen['synthetic_xr'] == X.XRGeometry()
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--synthetic-xr', '--xr-source-detector', '1000', '--xr-source-center', '900',
                           '--xr-view', 'pa', '--xr-parallel'])
    assert seen['synthetic_xr'] == X.XRGeometry(source_detector_mm=1000.0, source_center_mm=900.0, view='pa', parallel=True)
    seen.clear()
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e')])
    assert 'synthetic_xr' not in seen                                            # without the flag: the call of before


# ------------------------------------------------------------------------------------------------ 4. the planner as plain C++ under the sanitizers
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    """tests/xr_driver.cpp with csrc/prep_plan.cpp behind a main of its own, under the address and undefined-behaviour sanitizers (nothing loaded
    into Python runs under a sanitizer)."""
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc: the planner includes the HIP runtime API header')
    exe = tmp_path_factory.mktemp('xr_driver') / 'xr_driver'
    inc = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), 'include')
    subprocess.check_call([HIPCC, '-x', 'c++', '-D__HIP_PLATFORM_AMD__', '-I' + inc, '-I' + CSRC, '-O1', '-g', '-std=c++17', '-Wall', '-Wno-unused-function',
                           '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', str(exe), os.path.join(ROOT, 'tests', 'xr_driver.cpp'),
                           os.path.join(CSRC, 'prep_plan.cpp')])
    return str(exe)


def test_the_planner_forms_the_tables_of_the_statement(driver, tmp_path):
    rng = np.random.default_rng(391)
    cases, refused = [], []
    for n in range(120):
        shape = tuple(int(v) for v in rng.integers(1, (9, 40, 70)))
        spacing = tuple(float(v) for v in rng.choice([0.5, 0.7, 0.9765625, 1.0, 1.5, 2.3, 3.0, 5.0], 3))
        half = (shape[1] - 1) * spacing[1] / 2
        near = float(rng.choice([2.0 ** -20, 0.3, 17.0, 400.0, 1500.0]))           # the source's distance to the first plane
        sod = float(half + near)
        sdd = float(sod + half + rng.choice([2.0 ** -10, 0.1, 33.3, 300.0]))
        kw = dict(source_detector_mm=sdd, source_center_mm=sod, view=('ap', 'pa')[n % 2], parallel=bool(n // 2 % 2))
        if not kw['parallel'] and (n % 3 == 0 or near < 1):                      # (a source that near magnifies the default detector beyond any use)
            kw.update(detector_spacing=(float(rng.choice([0.3, 1.0, 2.7])), float(rng.choice([0.4, 1.1, 7.0]))), detector_size=(int(rng.integers(1, 90)), int(rng.integers(1, 12))))
        cases.append((shape, spacing, X.XRGeometry(**kw)))
    lines = []
    for shape, spacing, g in cases:
        r = g.resolve(shape, spacing)
        lines.append((shape, spacing, r['sdd'], r['sod'], r['pa'], r['parallel'], r['du'], r['dv'], r['nu'], r['nv']))
    # what the planner refuses, in the module's words: each line of `bad` is one good line with one number changed
    base = ((5, 9, 66), SPACING, 1800.0, 1500.0, 0, 0, 1.5, 2.0, 80, 6)
    for at, value, text in ((0, (0, 9, 66), 'below 1'), (1, (0.0, 0.75, 2.0), 'spacing_x'), (1, (1.5, float('nan'), 2.0), 'spacing_y'),
                            (1, (1.5, 0.75, float('inf')), 'spacing_z'), (2, -1.0, 'source_detector_mm'), (3, 0.0, 'source_center_mm'),
                            (3, 3.0, 'source inside the slab'), (2, 1502.5, 'detector inside the slab'), (4, 2, 'view 2'), (5, 3, 'parallel 3'),
                            (6, 0.0, 'du'), (7, float('inf'), 'dv'), (8, 0, 'below 1'), (9, -2, 'below 1'), (8, 2 ** 30, 'more than 2^31 - 1 pixels'),
                            (5, 1, 'parallel rays fix')):
        bad = list(base)
        bad[at] = value
        lines.append(tuple(bad))
        refused.append((len(lines) - 1, text))
    with open(tmp_path / 'cases.txt', 'w') as f:
        for shape, spacing, sdd, sod, pa, par, du, dv, nu, nv in lines:
            f.write(' '.join([str(v) for v in shape] + [float(v).hex() for v in (*spacing, sdd, sod)] + [str(pa), str(par), float(du).hex(), float(dv).hex(),
                                                                                                       str(nu), str(nv)]) + '\n')
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([driver, str(tmp_path / 'cases.txt'), str(tmp_path / 'out.bin')], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and not run.stderr.strip(), run.stderr[-4000:]
    got = np.fromfile(tmp_path / 'out.bin', np.float64)
    at = 0
    seen = set()
    for shape, spacing, g in cases:
        tb = X.xr_tables(shape, spacing, g)
        r = tb['geometry']
        assert got[at] == 0.0, (shape, spacing, g)
        at += 1
        n = r['nu'] * r['nv']
        sums = 0.375 * (np.arange(n, dtype=np.float64) + 1).reshape(r['nv'], r['nu'])
        for name, want in (('t', tb['t']), ('a', tb['a']), ('cx', tb['cx']), ('b', tb['b']), ('cz', tb['cz']), ('step', tb['step']),
                           ('xr', (sums * tb['step']).astype(np.float32).astype(np.float64))):
            assert (_bits(got[at:at + want.size]) == _bits(want.reshape(-1))).all(), (name, shape, spacing, g)
            at += want.size
        seen.add((r['pa'], r['parallel'], g.detector_size is None))
    assert len(seen) == 6                                                         # both views, both beam forms, default and given detectors
    messages = dict(line.split(': ', 1) for line in run.stdout.splitlines() if line.startswith('refused '))
    for line, text in refused:
        assert got[at] == -1.0 and text in messages[f'refused {line}'] and messages[f'refused {line}'].startswith('xr_driver: '), (line, text, messages)
        at += 1
    assert at == got.size
