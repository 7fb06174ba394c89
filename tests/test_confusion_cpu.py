"""The confusion matrix without a GPU: evaluate.confusion_statement against a plain per-pair loop and against overlap_statement, the hand cases
of evaluate.confusion (orientation, the top lists, accuracy and kappa), the JSON round trip, Result.confusion / save_confusion and the command
line on the host route, and csrc/confusion.h's operand forms as plain C++ under the sanitizers (tests/confusion_driver.cpp)."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests.batch_util import synthetic_batch_model
from tests.confusion_util import PAIRINGS, plain_loop, random_side
from tests.conftest import GOLDEN, ROOT
from totalsegmentator2d_amd import evaluate as E, image, main, nrrd
from totalsegmentator2d_amd.main import ts2d_run
from totalsegmentator2d_amd.tool import TS2D

HIPCC = '/opt/rocm/bin/hipcc'
A = os.path.join(GOLDEN, 'assets')


# ------------------------------------------------------------------------------------------------ 1. the statement
def random_cases(n=104):
    rng = np.random.default_rng(37)
    out = []
    for j in range(n):
        kind_a, kind_b = PAIRINGS[j % 4]
        spatial = (int(rng.integers(1, 9)), int(rng.integers(1, 12)))
        if j // 4 % 2:
            spatial = (int(rng.integers(1, 4)),) + spatial
        K = int(rng.integers(1, 7))
        values = sorted(int(v) for v in rng.choice(np.arange(1, 256), K, replace=False)) if j // 8 % 2 else list(range(1, K + 1))
        absent_a = (0,) if j // 16 % 3 else ()
        absent_b = (0,) if j // 16 % 3 == 2 else ((K - 1,) if j // 16 % 3 == 1 else ())
        out.append((random_side(rng, kind_a, K, spatial, values, absent_a), kind_a, random_side(rng, kind_b, K, spatial, values, absent_b), kind_b,
                    values, K))
    return out


def test_statement_against_the_plain_loop_and_the_overlap_statement():
    cases = random_cases()
    assert len(cases) >= 100
    seen = set()
    for a, kind_a, b, kind_b, values, K in cases:
        M = E.confusion_statement(a, kind_a, b, kind_b, values)
        assert M.dtype == np.int64 and M.shape == (K + 2, K + 2)
        assert (M == plain_loop(a, kind_a, b, kind_b, values, K)).all()
        N = int(np.prod(a.shape[1:] if kind_a == E.PLANES else a.shape))
        ov = E.overlap_statement(a, kind_a, b, kind_b, values)
        d = np.arange(1, K + 1)
        assert (M[d, d] == ov['n_both']).all() and (M[d, K + 1] == ov['n_a']).all() and (M[K + 1, d] == ov['n_b']).all() and M[K + 1, K + 1] == N
        if kind_a == kind_b == E.LABELMAP:
            inner = M[:K + 1, :K + 1]
            assert inner.sum() == N and (inner.sum(axis=1) == M[:K + 1, K + 1]).all() and (inner.sum(axis=0) == M[K + 1, :K + 1]).all()
        seen.add((kind_a, kind_b, a.ndim - (kind_a == E.PLANES), values == list(range(1, K + 1))))
    assert len(seen) == 4 * 2 * 2                  # every pairing, 2-D and 3-D, values 1 ... K and others
    # planes overlap: somewhere the inner block sums to more than N
    assert any(E.confusion_statement(a, ka, b, kb, v)[:K + 1, :K + 1].sum() > np.prod(b.shape[1:] if kb == E.PLANES else b.shape)
               for a, ka, b, kb, v, K in cases if E.PLANES in (ka, kb))


def test_statement_refusals_are_those_of_the_overlap_statement():
    with pytest.raises(ValueError, match='values'):
        E.confusion_statement(np.zeros((2, 3), np.uint8), E.LABELMAP, np.zeros((2, 3), np.uint8), E.LABELMAP)
    with pytest.raises(ValueError, match='shape'):
        E.confusion_statement(np.zeros((2, 3, 3), np.uint8), E.PLANES, np.zeros((2, 3, 4), np.uint8), E.PLANES)


# ------------------------------------------------------------------------------------------------ 2. confusion(): the hand cases
def label_image(arr, names=None, spacing=None):
    arr = np.asarray(arr, np.uint8)
    nd = arr.ndim
    img = nrrd.Image(arr, spacing or (1.0,) * nd, (0.0,) * nd, tuple(np.eye(nd).reshape(-1)), 1, {}, None)
    if names:
        img.meta = {k: v for i, (value, name) in enumerate(names.items())
                    for k, v in ((f'Segment{i}_ID', str(i)), (f'Segment{i}_Name', name), (f'Segment{i}_LabelValue', str(value)), (f'Segment{i}_Layer', '0'))}
    return img


def planes_image(planes, names):
    planes = np.asarray(planes, np.uint8)
    nd = planes.ndim - 1
    img = nrrd.Image(np.ascontiguousarray(np.moveaxis(planes, 0, -1)), (1.0,) * nd, (0.0,) * nd, tuple(np.eye(nd).reshape(-1)), planes.shape[0], {}, None)
    image.set_annotation_meta(img, names)
    return img


def test_orientation_rows_are_the_reference():
    #  reference: 4 x bg, 3 x A (5), 3 x B (9);  prediction: the A's become A, B, B; one B becomes bg; one bg becomes A
    ref = label_image([[0, 0, 0, 0, 5, 5, 5, 9, 9, 9]])
    pred = label_image([[0, 0, 0, 5, 5, 9, 9, 9, 9, 0]], {5: 'A', 9: 'B'})
    c = E.confusion(pred, ref)
    assert c['classes'] == ['background', 'A', 'B'] and c['values'] == [0, 5, 9] and c['samples'] == 10
    assert (c['rows'], c['columns']) == ('reference', 'prediction')
    assert c['matrix'] == [[3, 1, 0], [0, 1, 2], [1, 0, 2]]                 # matrix[r][p]: asymmetric, written out by hand
    assert c['count_ref'] == [4, 3, 3] and c['count_pred'] == [4, 2, 4] and c['exclusive'] is True
    assert c['labels']['A'] == {'value': 5, 'predicted_as': [{'class': 'B', 'value': 9, 'count': 2, 'fraction': 2 / 3}],
                                'predicted_from': [{'class': 'background', 'value': 0, 'count': 1, 'fraction': 1 / 2}]}
    assert c['labels']['B']['predicted_as'] == [{'class': 'background', 'value': 0, 'count': 1, 'fraction': 1 / 3}]
    assert c['labels']['B']['predicted_from'] == [{'class': 'A', 'value': 5, 'count': 2, 'fraction': 2 / 4}]
    assert all(type(v) is int for row in c['matrix'] for v in row)
    # accuracy and kappa by hand: trace 6 of 10; pe = (4*4 + 3*2 + 3*4) / 100 = 0.34
    assert c['accuracy'] == 6 / 10 and c['kappa'] == (6 * 10 - 34) / (100 - 34)
    assert abs(c['kappa'] - (0.6 - 0.34) / (1 - 0.34)) < 1e-15
    with pytest.raises(ValueError, match='extent'):
        E.confusion(pred, label_image([[0, 0, 5]]))
    with pytest.raises(ValueError, match='top'):
        E.confusion(pred, ref, top=-1)


def test_top_ordering_with_a_tie_and_top_zero():
    names = {1: 'a', 2: 'b', 3: 'c', 4: 'd'}
    #  the reference's 'a' (8 samples) goes: 1 to bg, 2 to b, 2 to c, 3 to d  -> d (3), then the tie b, c (2) by class index, then bg
    ref = label_image([[1] * 8 + [0, 0]])
    pred = label_image([[0, 2, 2, 3, 3, 4, 4, 4, 1, 1]], names)
    c = E.confusion(pred, ref)
    assert [(e['class'], e['count']) for e in c['labels']['a']['predicted_as']] == [('d', 3), ('b', 2), ('c', 2)]
    assert [(e['class'], e['count']) for e in E.confusion(pred, ref, top=10)['labels']['a']['predicted_as']] == [('d', 3), ('b', 2), ('c', 2), ('background', 1)]
    assert [e['class'] for e in E.confusion(pred, ref, top=1)['labels']['a']['predicted_as']] == ['d']
    assert c['labels']['a']['predicted_from'] == [{'class': 'background', 'value': 0, 'count': 2, 'fraction': 1.0}]
    assert c['labels']['b']['predicted_as'] == [] and c['labels']['b']['predicted_from'] == [{'class': 'a', 'value': 1, 'count': 2, 'fraction': 1.0}]
    z = E.confusion(pred, ref, top=0)
    assert all(l['predicted_as'] == [] and l['predicted_from'] == [] for l in z['labels'].values()) and z['matrix'] == c['matrix']


def test_kappa_is_none_with_one_class_and_both_are_none_with_planes():
    full = label_image(np.full((3, 4), 7), {7: 'x'})
    c = E.confusion(full, full)
    assert c['matrix'] == [[0, 0], [0, 12]] and c['accuracy'] == 1.0 and c['kappa'] is None
    p = planes_image(np.ones((2, 3, 4)), {1: 'u', 2: 'v'})
    c = E.confusion(p, label_image(np.ones((3, 4))))
    assert c['exclusive'] is False and c['accuracy'] is None and c['kappa'] is None
    assert c['matrix'] == [[0, 0, 0], [0, 12, 12], [0, 0, 0]] and sum(map(sum, c['matrix'])) > c['samples']
    c = E.confusion(label_image(np.ones((3, 4)), {1: 'u', 2: 'v'}), p)
    assert c['exclusive'] is False and c['accuracy'] is None and c['matrix'] == [[0, 0, 0], [0, 12, 0], [0, 12, 0]]


def test_confusion_of_a_result_with_itself_is_the_label_cooccurrence():
    rng = np.random.default_rng(5)
    planes = (rng.random((3, 6, 7)) < 0.4).astype(np.uint8)
    seg = planes_image(planes, {1: 'p', 2: 'q', 3: 'r'})
    c = E.confusion(seg, seg)
    m = np.array(c['matrix'])
    assert (m == m.T).all() and [m[i, i] for i in (1, 2, 3)] == [int(planes[k].sum()) for k in range(3)]
    assert m[1, 2] == int((planes[0] & planes[1]).sum()) > 0 and m[0, 0] == int((planes.sum(axis=0) == 0).sum())
    assert c['count_ref'] == c['count_pred'] and c['exclusive'] is False


def test_json_round_trip(tmp_path):
    rng = np.random.default_rng(6)
    pred = label_image(rng.integers(0, 4, (2, 5, 6)), {1: 'a', 2: 'b', 3: 'c'}, (1.0, 2.0, 0.5))
    ref = label_image(rng.integers(0, 4, (2, 5, 6)))
    c = E.confusion(pred, ref)
    assert c['samples'] == 60 and np.array(c['matrix']).sum() == 60
    with open(E.dump_evaluation(c, str(tmp_path / 'c.json'))) as f:
        assert json.load(f) == c


def test_device_confuses_asks_for_the_symbol(monkeypatch):
    from totalsegmentator2d_amd import engine
    a = np.zeros((4, 5), np.uint8)
    asked = []
    monkeypatch.setattr(engine, 'has_entry', lambda *names: asked.append(names) or all(n != 'ts2d_label_confusion' for n in names))
    assert E.device_confuses(a, E.LABELMAP, a, E.LABELMAP, [1, 2], (4, 5), 2) is False and ('ts2d_label_confusion',) in asked
    monkeypatch.setattr(engine, 'has_entry', lambda *names: True)
    assert E.device_confuses(a, E.LABELMAP, a, E.LABELMAP, [1, 2], (4, 5), 2) is True
    assert E.device_confuses(a.astype(np.int16), E.LABELMAP, a, E.LABELMAP, [1, 2], (4, 5), 2) is False


# ------------------------------------------------------------------------------------------------ 3. Result.confusion, save_confusion, the CLI
@pytest.fixture(scope='module')
def two_models():
    m1, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_cardiac', 3, 31, mirror=False, feats=(32, 32))
    m2, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_ribs', 4, 32, mirror=False, feats=(32, 32))
    return {'ts2d-v2-ep4000b2_cardiac': m1, 'ts2d-v2-ep4000b2_ribs': m2}


def reference_volume(seed=61):
    case = nrrd.read(os.path.join(A, 'sample_s0521.nrrd'))
    rng = np.random.default_rng(seed)
    lab = np.zeros(case.array.shape, np.int16)
    for v in range(1, 7):
        lo = [int(rng.integers(0, s // 2)) for s in lab.shape]
        lab[tuple(slice(o, o + int(rng.integers(3, s // 2))) for o, s in zip(lo, lab.shape))] = v
    return nrrd.Image(lab, case.spacing, case.origin, case.direction, 1, {}, case.space)


def test_result_confusion_and_save_confusion_on_the_host_route(tmp_path, two_models):
    vol = reference_volume()
    with TS2D(models=dict(two_models)) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        assert res.device is None
        seg = res.get_segmentation()
        ref2d = E.project_labels(image.reorient_image(vol), 7, 'coronal')
        c = res.confusion(vol)                                               # a 3-D label volume is projected
        assert c == E.confusion(seg, ref2d) and c['classes'][1:] == list(image.get_annotation_labels(seg)) and len(c['matrix']) == 8
        ev = res.evaluate(vol)
        for i, e in enumerate(ev.values(), 1):
            assert (c['matrix'][i][i], c['count_ref'][i], c['count_pred'][i]) == (e['count_both'], e['count_ref'], e['count_pred'])
        assert res.confusion(ref2d) == c                                     # an already-2-D segmentation is taken as it is
        assert res.confusion(vol, top=1) == E.confusion(seg, ref2d, top=1) != c
        with pytest.raises(ValueError, match=r'extent .* against extent'):   # the shared preparation keeps the grid check, for both methods
            res.confusion(nrrd.Image(ref2d.array[:-1], ref2d.spacing, ref2d.origin, ref2d.direction, 7, {}, None))
        with pytest.raises(ValueError, match=r'extent .* against extent'):
            res.evaluate(nrrd.Image(ref2d.array[:-1], ref2d.spacing, ref2d.origin, ref2d.direction, 7, {}, None))
        with pytest.raises(ValueError, match='spacing'):
            res.evaluate(nrrd.Image(ref2d.array, (9.0, 9.0, 9.0), ref2d.origin, ref2d.direction, 7, {}, None))
        with pytest.raises(ValueError, match='no segmentation'):
            res.confusion(vol, model='nope')
        files = res.save_confusion(str(tmp_path), 'case', vol)
        assert [os.path.basename(f) for f in files] == ['case.confusion.json']
        with open(files[0]) as f:
            assert json.load(f) == c
        files = res.save_confusion(str(tmp_path / 'all'), 'case', ref2d, models='all')
        assert sorted(os.path.basename(f) for f in files) == ['case-cardiac.confusion.json', 'case-ribs.confusion.json', 'case.confusion.json']


def test_cli_confusion(tmp_path, two_models, monkeypatch, capsys):
    src = tmp_path / 'one.nrrd'
    shutil.copy(os.path.join(A, 'sample_s0521.nrrd'), src)
    ref = tmp_path / 'ref.nrrd'
    nrrd.write(reference_volume(61), str(ref), True)
    kw = dict(models=dict(two_models), visualize=False, silent=True, reference=str(ref))
    ts2d_run(str(src), str(tmp_path / 'a'), **kw)
    ts2d_run(str(src), str(tmp_path / 'b'), confusion=True, **kw)
    assert sorted(os.listdir(tmp_path / 'b')) == sorted(os.listdir(tmp_path / 'a') + ['one.confusion.json'])
    for f in os.listdir(tmp_path / 'a'):                                     # without the flag: the files and bytes of before
        assert (tmp_path / 'a' / f).read_bytes() == (tmp_path / 'b' / f).read_bytes()
    with open(tmp_path / 'b' / 'one.confusion.json') as f, open(tmp_path / 'b' / 'one.evaluation.json') as g:
        c, ev = json.load(f), json.load(g)
    assert [c['matrix'][i][i] for i in range(1, 8)] == [e['count_both'] for e in (ev[n] for n in c['classes'][1:])]
    with pytest.raises(SystemExit):                                          # --confusion alone is an argument error
        main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--confusion'])
    assert '--reference' in capsys.readouterr().err and not os.path.exists(tmp_path / 'e')
    seen = {}
    monkeypatch.setattr(main, 'ts2d_run', lambda **kw: seen.update(kw))
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--reference', str(ref), '--confusion'])
    assert seen['confusion'] is True and seen['reference'] == str(ref)
    seen.clear()
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--reference', str(ref)])
    assert 'confusion' not in seen                                           # without the flag: the call of before


# ------------------------------------------------------------------------------------------------ 4. csrc/confusion.h on the host, under the sanitizers
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    """tests/confusion_driver.cpp - csrc/confusion.h behind a main of its own - under the address and undefined-behaviour sanitizers where the
    toolchain links them (nothing loaded into Python runs under a sanitizer)."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = tmp_path_factory.mktemp('confusion_driver') / 'confusion_driver'
    base = [cxx, '-x', 'c++', '-O1', '-g', '-std=c++17', '-Wno-unknown-pragmas', '-o', str(exe), os.path.join(ROOT, 'tests', 'confusion_driver.cpp')]
    if subprocess.call(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    return str(exe)


def test_the_shared_header_forms_the_statement(driver, tmp_path):
    rng = np.random.default_rng(38)
    runs = []
    for N in (1, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 100):
        for K in (1, 2, 5, 30, 31, 33):
            kind_a, kind_b = PAIRINGS[len(runs) % 4]
            values = sorted(int(v) for v in rng.choice(np.arange(1, 256), K, replace=False))
            runs.append((random_side(rng, kind_a, K, (N,), values, (0,) if K > 2 else ()), kind_a, random_side(rng, kind_b, K, (N,), values), kind_b, values, K))
    with open(tmp_path / 'in.bin', 'wb') as f:
        for a, kind_a, b, kind_b, values, K in runs:
            f.write(struct.pack('<4i', a.shape[-1], K, kind_a, kind_b))
            f.write(bytes(values) + a.tobytes() + b.tobytes())
    subprocess.run([driver, str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')], check=True)
    got = np.fromfile(tmp_path / 'out.bin', np.int64)
    at = 0
    for a, kind_a, b, kind_b, values, K in runs:
        M = E.confusion_statement(a, kind_a, b, kind_b, values)
        assert (got[at:at + M.size].reshape(M.shape) == M).all(), (a.shape, K, kind_a, kind_b)
        at += M.size
    assert at == got.size
