"""The components of every label at once, without a GPU: the statement (components.label_components_statement) against two independent
restatements, the hand cases of the rule, the size threshold in mm, csrc/cc_label.h's class-equality linking as plain C++ under the sanitizers,
and Result.components / Result.cleaned / save_components / the command line on the host route."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import components_util as U
from tests.batch_util import synthetic_batch_model
from tests.conftest import GOLDEN, ROOT
from totalsegmentator2d_amd import components as C
from totalsegmentator2d_amd import image, main, nrrd
from totalsegmentator2d_amd.main import ts2d_run
from totalsegmentator2d_amd.tool import TS2D

HIPCC = '/opt/rocm/bin/hipcc'
A = os.path.join(GOLDEN, 'assets')


# ------------------------------------------------------------------------------------------------ 1. the statement
def random_cases(n=200):
    """2-D and 3-D inputs of both kinds, at most 4 x 9 x 11, densities 0.1 ... 0.8, label-map values that are not 1 ... K."""
    rng = np.random.default_rng(36)
    out = []
    for j in range(n):
        spatial = (int(rng.integers(1, 10)), int(rng.integers(1, 12)))
        if j % 2:
            spatial = (int(rng.integers(1, 5)),) + spatial
        K = int(rng.integers(1, 5))
        seg, values = U.random_case(rng, ('planes', 'labelmap')[j // 2 % 2], spatial, K, (0.1, 0.2, 0.3, 0.5, 0.65, 0.8)[j % 6])
        rule = (dict(), dict(keep_largest=True), dict(min_voxels=[int(v) for v in rng.integers(0, 6, K)]),
                dict(keep_largest=True, min_voxels=[int(v) for v in rng.integers(0, 6, K)]))[j // 4 % 4]
        out.append((seg, values, ('full', 'faces')[j // 16 % 2], rule))
    return out


def test_statement_equals_both_restatements_on_random_inputs():
    cases = random_cases()
    assert len(cases) >= 200
    seen = set()
    for seg, values, conn, rule in cases:
        got = C.label_components_statement(seg, values, conn, **rule)
        assert got[0].dtype == seg.dtype and got[0].shape == seg.shape and got[1].dtype == np.int64 and got[2].dtype == np.int64
        assert U.same(got, U.scipy_restatement(seg, values, conn, **rule))
        assert U.same(got, U.flood_restatement(seg, values, conn, **rule))
        seen.add((values is None, seg.ndim - (values is None), conn, tuple(sorted(rule))))
        assert int(got[1][:, 3].sum()) == int(np.count_nonzero(seg) - np.count_nonzero(got[0])) and len(got[2]) == int(got[1][:, 1].sum())
    assert len(seen) == 2 * 2 * 2 * 4          # both kinds, 2-D and 3-D, both connectivities, every rule


def S(seg, values=None, conn='full', **rule):
    return C.label_components_statement(np.asarray(seg, np.uint8), values, conn, **rule)


def test_hand_cases():
    # two labels adjacent in a label map do not join; the same label touching only diagonally joins under full, not under faces
    m = [[5, 9, 0], [0, 5, 9], [0, 0, 0]]
    out, ctr, rows = S(m, [5, 9])
    assert ctr.tolist() == [[2, 1, 2, 0, 0], [2, 1, 2, 0, 0]] and rows.tolist() == [[0, 0, 2], [1, 1, 2]]
    out, ctr, rows = S(m, [5, 9], 'faces')
    assert ctr.tolist() == [[2, 2, 1, 0, 0], [2, 2, 1, 0, 0]] and rows.tolist() == [[0, 0, 1], [0, 4, 1], [1, 1, 1], [1, 5, 1]]
    # a mask that ends plane k and starts plane k + 1 stays two components
    p = np.zeros((2, 2, 3), np.uint8)
    p[0, 1, 2] = p[1, 0, 0] = 1
    assert S(p)[2].tolist() == [[0, 5, 1], [1, 0, 1]]
    # a tie for the largest: both stay under keep_largest, the smaller one goes
    t = [[1, 1, 0, 1, 1, 0, 1]]
    out, ctr, rows = S(t, [1], keep_largest=True)
    assert out.tolist() == [[1, 1, 0, 1, 1, 0, 0]] and ctr.tolist() == [[5, 3, 2, 1, 1]] and rows.tolist() == [[0, 0, 2], [0, 3, 2], [0, 6, 1]]
    # s == min_voxels stays, s == min_voxels - 1 goes
    assert S(t, [1], min_voxels=[2])[0].tolist() == [[1, 1, 0, 1, 1, 0, 0]]
    assert S(t, [1], min_voxels=[3])[0].tolist() == [[0] * 7] and S(t, [1], min_voxels=[3])[1].tolist() == [[5, 3, 2, 5, 3]]
    assert S(t, [1], min_voxels=[1])[0].tolist() == t
    # both rules together: keep_largest takes the 2, the threshold takes the 1 - and, in another label, the largest itself
    b = [[1, 1, 1, 0, 1, 1, 0, 1, 0, 7, 7]]
    out, ctr, _ = S(b, [1, 7], keep_largest=True, min_voxels=[0, 3])
    assert out.tolist() == [[1, 1, 1] + [0] * 8] and ctr.tolist() == [[6, 3, 3, 3, 2], [2, 1, 2, 2, 1]]
    # an absent label: zeros and no rows; an all-foreground map; K = 1
    out, ctr, rows = S(np.full((2, 3, 4), 3), [8, 3])
    assert ctr.tolist() == [[0] * 5, [24, 1, 24, 0, 0]] and rows.tolist() == [[1, 0, 24]] and out.tolist() == np.full((2, 3, 4), 3).tolist()
    out, ctr, rows = S(np.zeros((1, 2, 2)), None)
    assert ctr.tolist() == [[0] * 5] and rows.shape == (0, 3)
    with pytest.raises(ValueError):
        S(t, [1], 'edges')
    with pytest.raises(ValueError):
        S(t, [1], min_voxels=[-1])
    with pytest.raises(ValueError):
        S([1, 1], [1])


def test_min_size_mm_to_voxels():
    for spacing in ((0.8, 2.5), (1.5, 0.8, 0.8), (0.1, 0.3), (1.0, 1.0), (0.7, 0.7, 3.0)):
        mm = float(np.prod(np.asarray(spacing, np.float64)))
        for n in (1, 2, 3, 7, 10, 1000, 12345, 2 ** 31 - 1):
            for size in (np.float64(n) * mm, np.nextafter(np.float64(n) * mm, np.inf), np.nextafter(np.float64(n) * mm, 0.0), n * 0.37):
                got = C.min_voxels_of(float(size), mm)
                assert np.float64(got) * np.float64(mm) >= size and (got == 0 or np.float64(got - 1) * np.float64(mm) < size)
        assert C.min_voxels_of(0.0, mm) == 0 and C.min_voxels_of(mm, mm) == 1 and C.min_voxels_of(1e-300, mm) == 1
    assert C.min_voxels_of(5.0, 2.0) == 3 and C.min_voxels_of(6.0, 2.0) == 3 and C.min_voxels_of(6.000001, 2.0) == 4
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            C.min_voxels_of(bad, 1.0)
    with pytest.raises(ValueError):
        C.min_voxels_of(1.0, 0.0)


# ------------------------------------------------------------------------------------------------ 2. cc_label.h on the host, under the sanitizers
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    """tests/components_driver.cpp - csrc/cc_label.h behind a main of its own - under the address and undefined-behaviour sanitizers where the
    toolchain links them (nothing loaded into Python runs under a sanitizer)."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = tmp_path_factory.mktemp('components_driver') / 'components_driver'
    base = [cxx, '-x', 'c++', '-O1', '-g', '-std=c++17', '-Wno-unknown-pragmas', '-o', str(exe), os.path.join(ROOT, 'tests', 'components_driver.cpp')]
    if subprocess.call(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    return str(exe)


def class_maps():
    """Class arrays [Z, H, W] (0: no label): the random label maps of section 1 as classes, the serpentine, and extents with W = 1, 63, 64, 65, 130."""
    rng = np.random.default_rng(37)
    out = []
    for seg, values, _, _ in random_cases():
        if values is not None:
            table = np.zeros(256, np.uint8)
            table[values] = np.arange(1, len(values) + 1)
            out.append(table[seg].reshape(((1,) + seg.shape)[-3:]))
    out.append(U.serpentine(4, 32, 32))
    for W in (1, 63, 64, 65, 130):
        for Z, H in ((1, 5), (3, 4)):
            for density in (0.3, 0.7, 1.0):
                out.append(((rng.random((Z, H, W)) < density) * rng.integers(1, 4, (Z, H, W))).astype(np.uint8))
            out.append(np.full((Z, H, W), 2, np.uint8))
    return out


def test_host_build_of_the_class_linking_gives_the_statements_partition(driver, tmp_path):
    maps = class_maps()
    runs = [(cls, faces, rev) for cls in maps for faces in (0, 1) for rev in (0, 1)]
    with open(tmp_path / 'in.bin', 'wb') as f:
        for cls, faces, rev in runs:
            f.write(struct.pack('<5i', *cls.shape, faces, rev))
            f.write(cls.tobytes())
    subprocess.run([driver, str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')], check=True)
    got = np.fromfile(tmp_path / 'out.bin', np.int32)
    at = 0
    for cls, faces, rev in runs:
        n = cls.size
        gave_up, parent, count = int(got[at]), got[at + 1:at + 1 + n], got[at + 1 + n:at + 1 + 2 * n]
        at += 1 + 2 * n
        assert gave_up == 0
        K = int(cls.max())
        want_parent, want_count = np.full(n, -1, np.int64), np.zeros(n, np.int64)
        if K:
            _, _, rows = C.label_components_statement(cls, list(range(1, K + 1)), ('full', 'faces')[faces])
            lab_of = {}
            for k in range(K):          # every voxel's root is the first voxel of its component, whose count is the component's size
                lab, _ = U.ndimage.label(cls == k + 1, structure=U.STRUCTURES[('full', 'faces')[faces], 3])
                flat = lab.reshape(-1)
                first = {int(flat[r[1]]): int(r[1]) for r in rows if r[0] == k}
                for c, root in first.items():
                    want_parent[flat == c] = root
            want_count[rows[:, 1]] = rows[:, 2]
        assert np.array_equal(parent, want_parent) and np.array_equal(count, want_count)
    assert at == got.size


# ------------------------------------------------------------------------------------------------ 3. images, results, the command line (host route)
def _annotated(multilabel: bool, dim3: bool):
    rng = np.random.default_rng(6)
    spatial = (5, 1, 9) if dim3 else (5, 9)
    sp = (0.8, 2.0, 1.5) if dim3 else (0.8, 2.5)
    eye = tuple(float(v) for v in np.eye(len(spatial)).reshape(-1))
    if multilabel:
        arr = (rng.random(spatial + (3,)) < 0.4).astype(np.uint8) * 200
        arr[..., 1] = 0
        seg = nrrd.Image(arr, sp, (0.0,) * len(spatial), eye, 3, {}, None)
        image.set_annotation_meta(seg, {1: 'a', 2: 'b', 3: 'c'}, {'a': (255, 0, 0)})
    else:
        arr = rng.integers(0, 4, spatial).astype(np.uint8) * 2          # values 0, 2, 4, 6: the meta names every value the map holds
        seg = nrrd.Image(arr, sp, (0.0,) * len(spatial), eye, 1, {}, None)
        image.set_annotation_meta(seg, {2: 'two', 4: 'four'}, {'four': '#00FF00'})
    return seg


def test_label_components_and_clean_components_of_images():
    for multilabel in (True, False):
        for dim3 in (False, True):
            seg = _annotated(multilabel, dim3)
            before = seg.array.tobytes()
            mm = float(np.prod(seg.spacing))
            for conn in C.CONNECTIVITIES:
                got = C.label_components(seg, connectivity=conn)
                assert list(got) == list(image.get_annotation_labels(seg))
                for name, info in image.get_annotation_labels(seg).items():
                    mask = seg.array[..., info['value'] - 1] > 0 if multilabel else seg.array == info['value']
                    lab, n = U.ndimage.label(mask, structure=U.STRUCTURES[conn, mask.ndim])
                    sizes = sorted(np.bincount(lab.ravel())[1:].tolist(), reverse=True)
                    e = got[name]
                    assert sorted(e) == ['components', 'count', 'first_index', 'largest', 'largest_mm', 'mm', 'sizes', 'sizes_mm']
                    assert e['count'] == int(mask.sum()) and e['mm'] == e['count'] * mm and e['components'] == n and e['sizes'] == sizes
                    assert e['largest'] == (sizes[0] if sizes else 0) and e['largest_mm'] == e['largest'] * mm
                    assert e['sizes_mm'] == [s * mm for s in sizes] and len(e['first_index']) == n
                    for at, s in zip(e['first_index'], e['sizes']):
                        assert len(at) == mask.ndim and mask[tuple(at)] and int((lab == lab[tuple(at)]).sum()) == s
                        assert int(np.flatnonzero(lab.ravel() == lab[tuple(at)])[0]) == int(np.ravel_multi_index(at, mask.shape))
                assert json.loads(json.dumps(got)) == got
                same, ctr = C.clean_components(seg, connectivity=conn)
                assert same is not seg and same.array.tobytes() == before and same.array.shape == seg.array.shape and same.meta == seg.meta
                assert (same.spacing, same.origin, same.direction, same.components) == (seg.spacing, seg.origin, seg.direction, seg.components)
                assert all(c['voxels_removed'] == 0 and c['components_removed'] == 0 and c['voxels'] == got[n]['count'] for n, c in ctr.items())
                clean, ctr = C.clean_components(seg, connectivity=conn, keep_largest=True, min_size_mm=2 * mm)
                assert seg.array.tobytes() == before
                after = C.label_components(clean, connectivity=conn)
                for name, e in got.items():
                    keep = [s for s in e['sizes'] if s == e['largest'] and s >= 2]
                    assert after[name]['sizes'] == keep and ctr[name]['components_removed'] == e['components'] - len(keep)
                    assert ctr[name]['voxels_removed'] == e['count'] - sum(keep) and sorted(ctr[name]) == sorted(C.COUNTER_NAMES)
    empty = C.label_components(_annotated(True, True))['b']
    assert empty == {'count': 0, 'mm': 0.0, 'components': 0, 'largest': 0, 'largest_mm': 0.0, 'sizes': [], 'sizes_mm': [], 'first_index': []}
    with pytest.raises(ValueError):
        C.label_components(_annotated(True, True), connectivity='corners')


@pytest.fixture(scope='module')
def two_models():
    m1, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_cardiac', 3, 31, mirror=False, feats=(32, 32))
    m2, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_ribs', 4, 32, mirror=False, feats=(32, 32))
    return {'ts2d-v2-ep4000b2_cardiac': m1, 'ts2d-v2-ep4000b2_ribs': m2}


def test_result_components_cleaned_and_save_components_on_the_host_route(tmp_path, two_models):
    with TS2D(models=dict(two_models)) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device is None
        seg = res.get_segmentation()
        before = seg.array.tobytes()
        parts = {m: res.get_segmentation(m).array.tobytes() for m in res.models}
        got = res.components()
        assert got == C.label_components(seg) and list(got) == list(image.get_annotation_labels(seg)) and len(got) == 7
        assert res.components(connectivity='faces') == C.label_components(seg, connectivity='faces')
        part = res.components('ts2d-v2-ep4000b2_ribs')
        assert list(part) == [f'ribs_{i}' for i in range(1, 5)] and all(part[n] == got[n] for n in part)
        # the defaults: a new result of equal bytes that shares input and projections
        same = res.cleaned()
        assert same is not res and same.get_segmentation() is not seg and same.get_segmentation().array.tobytes() == before
        assert all(same.get_segmentation(m).array.tobytes() == parts[m] for m in res.models) and same.models == res.models
        assert same.get_input() is res.get_input() and all(same.get_projection(c) is p for c, p in res.get_projection().items())
        assert same.get_segmentation().meta == seg.meta and same.device is res.device
        # the rule, on the merged segmentation and on every sub-model's; the original stays
        clean = res.cleaned(keep_largest=True)
        assert seg.array.tobytes() == before and all(res.get_segmentation(m).array.tobytes() == parts[m] for m in res.models)
        after = clean.components()
        assert any(e['components'] > 1 for e in got.values())          # (else the case shows nothing)
        for name, e in got.items():
            keep = [s for s in e['sizes'] if s == e['largest']]
            assert after[name]['sizes'] == keep and after[name]['count'] == sum(keep)
        assert clean.components('ts2d-v2-ep4000b2_ribs') == {n: after[n] for n in part}
        only = res.cleaned(keep_largest=True, models=['ts2d-v2-ep4000b2_ribs'])
        assert only.get_segmentation('ts2d-v2-ep4000b2_cardiac').array.tobytes() == parts['ts2d-v2-ep4000b2_cardiac']
        assert only.components('ts2d-v2-ep4000b2_ribs') == clean.components('ts2d-v2-ep4000b2_ribs')
        mm = float(np.prod(seg.spacing))
        small = res.cleaned(min_size_mm=3 * mm).components()
        assert all(small[n]['sizes'] == [s for s in e['sizes'] if s >= 3] for n, e in got.items())
        # the files
        files = res.save_components(str(tmp_path), 'case')
        assert [os.path.basename(f) for f in files] == ['case.components.json']
        files = res.save_components(str(tmp_path), 'case', models='all')
        assert [os.path.basename(f) for f in files] == ['case.components.json', 'case-cardiac.components.json', 'case-ribs.components.json']
        assert [os.path.basename(f) for f in res.save_components(str(tmp_path), 'case', models='all', naming='model')][1:] == \
            ['case-ts2d-v2-ep4000b2_cardiac.components.json', 'case-ts2d-v2-ep4000b2_ribs.components.json']
        with open(tmp_path / 'case.components.json') as f:
            assert json.load(f) == got
        with open(tmp_path / 'case-ribs.components.json') as f:
            assert json.load(f) == part


def test_cli_flags_files_and_the_lone_connectivity(tmp_path, two_models, monkeypatch, capsys):
    src = tmp_path / 'in'
    os.makedirs(src)
    shutil.copy(os.path.join(A, 'sample_s0521.nrrd'), src / 'one.nrrd')
    run = dict(models=dict(two_models), visualize=False, silent=True)
    ts2d_run(str(src), str(tmp_path / 'plain'), **run)
    ts2d_run(str(src), str(tmp_path / 'comp'), components=True, statistics=True, save_all=True, **run)
    ts2d_run(str(src), str(tmp_path / 'clean'), keep_largest=True, min_component_mm=0.5, components=True, statistics=True, **run)
    ts2d_run(str(src), str(tmp_path / 'batch'), keep_largest=True, min_component_mm=0.5, components=True, statistics=True, batch_cases=2, **run)
    assert sorted(os.listdir(tmp_path / 'plain')) == ['one.seg.nrrd', 'one_max.nrrd', 'one_mean.nrrd']          # without a flag: the files of before
    extra = sorted(f for f in os.listdir(tmp_path / 'comp') if 'components' in f)
    assert extra == ['one-cardiac.components.json', 'one-ribs.components.json', 'one.components.json']
    assert (tmp_path / 'comp' / 'one.seg.nrrd').read_bytes() == (tmp_path / 'plain' / 'one.seg.nrrd').read_bytes()          # --components alone cleans nothing
    assert sorted(os.listdir(tmp_path / 'clean')) == sorted(os.listdir(tmp_path / 'plain') + ['one.components.json', 'one.statistics.json'])
    for f in os.listdir(tmp_path / 'clean'):
        assert (tmp_path / 'clean' / f).read_bytes() == (tmp_path / 'batch' / f).read_bytes()
    with open(tmp_path / 'comp' / 'one.components.json') as f:
        raw = json.load(f)
    with open(tmp_path / 'clean' / 'one.components.json') as f:
        clean = json.load(f)
    with open(tmp_path / 'clean' / 'one.statistics.json') as f:
        stats = json.load(f)
    assert any(e['components'] > 1 for e in raw.values())
    for name, e in raw.items():          # saved, measured: everything sees the cleaned result
        assert clean[name]['sizes'] == [s for s in e['sizes'] if s == e['largest']] and stats[name]['count'] == clean[name]['count']
    assert nrrd.read(str(tmp_path / 'clean' / 'one.seg.nrrd')).array.tobytes() != nrrd.read(str(tmp_path / 'plain' / 'one.seg.nrrd')).array.tobytes()
    # the parser
    seen = {}
    monkeypatch.setattr(main, 'ts2d_run', lambda **kw: (seen.clear(), seen.update(kw)))
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e')])
    assert not {'keep_largest', 'min_component_mm', 'components', 'component_connectivity'} & set(seen)          # the call of before
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--keep-largest', '--min-component-mm', '12.5', '--components',
                           '--component-connectivity', 'faces'])
    assert (seen['keep_largest'], seen['min_component_mm'], seen['components'], seen['component_connectivity']) == (True, 12.5, True, 'faces')
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--components'])
    assert (seen['keep_largest'], seen['min_component_mm'], seen['components'], seen['component_connectivity']) == (False, 0.0, True, 'full')
    for bad in (['--component-connectivity', 'faces'], ['--min-component-mm', '-1'], ['--components', '--component-connectivity', 'corners']):
        with pytest.raises(SystemExit) as ei:
            main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e')] + bad)
        assert ei.value.code == 2
    assert '--component-connectivity' in capsys.readouterr().err


def test_the_symbol_is_optional_and_the_abi_version_stays():
    from totalsegmentator2d_amd import _lib
    with open(os.path.join(ROOT, 'include', 'ts2d_engine.h')) as f:
        hdr = f.read()
    assert 'ts2d_label_components' in _lib.SIGNATURES and 'ts2d_label_components' in _lib.OPTIONAL and _lib.ABI_VERSION == 9
    for name, value in (('FULL', _lib.COMP_FULL), ('FACES', _lib.COMP_FACES), ('GIVE_UP', _lib.COMP_GIVE_UP), ('LIST_FULL', _lib.COMP_LIST_FULL),
                        ('COUNTERS', _lib.COMP_COUNTERS)):
        assert f'#define TS2D_COMP_{name} {value}\n' in hdr
    lib = _lib.load()
    assert hasattr(lib, 'ts2d_label_components') and lib.ts2d_abi_version() == 9
