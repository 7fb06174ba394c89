"""Percentiles of the intensities under a label on the host (totalsegmentator2d_amd/statistics.py): label_percentiles_statement against the fully
sorted brute force and against np.percentile, hand cases, label_statistics with and without percentiles, Result.statistics / save_statistics /
``ts2d --statistics-percentile`` on the host route, and csrc/label_select.h with the chunk planner of csrc/stats_plan.cpp compiled into a
stand-alone program (tests/label_select_driver.cpp)."""
import json
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.batch_util import synthetic_batch_model
from totalsegmentator2d_amd import evaluate as E, image, main, nrrd, statistics as S
from totalsegmentator2d_amd.tool import TS2D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'totalsegmentator2d_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
A = os.path.join(GOLDEN, 'assets')
QS = (0.0, 25.0, 37.5, 50.0, 95.0, 100.0)


def b32(v):
    return np.asarray(v, np.float32).view(np.uint32)


def b64(v):
    return np.asarray(v, np.float64).view(np.uint64)


def _case(kind, spatial, C, seed):
    """(seg, values, x): planes with overlaps, an empty plane and a one-sample plane, or a label map whose values are not 1 ... K with one
    value absent; intensities of mixed magnitude with ties, both zeros and subnormals."""
    rng = np.random.default_rng(seed)
    if kind == 'planes':
        seg = ((rng.random((4,) + spatial) < 0.5) * rng.integers(1, 256, (4,) + spatial)).astype(np.uint8)
        seg[2] = 0
        seg[3] = 0
        seg[3][tuple(rng.integers(0, s) for s in spatial)] = 9
        values = None
    else:
        values = [7, 200, 3, 41]                                                       # 41 stays absent
        seg = np.array([0, 7, 200, 3], np.uint8)[rng.integers(0, 4, spatial)]
    x = (rng.normal(size=(C,) + spatial) * rng.choice([1e-3, 1.0, 1e4], size=(C,) + spatial)).astype(np.float32)
    x[0] = np.round(x[0])                                                              # many ties, and zeros of both signs
    x.reshape(C, -1)[:, ::7] = rng.choice(np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39], np.float32), x.reshape(C, -1)[:, ::7].shape)
    return seg, values, x


CASES = [(kind, spatial, C, seed) for kind in ('planes', 'labelmap') for spatial in ((131,), (7, 70), (3, 5, 67), (1, 1)) for C, seed in ((1, 0), (3, 1))]


@pytest.mark.parametrize('kind,spatial,C,seed', CASES)
def test_the_ranks_are_those_of_the_sorted_keys_and_the_percentile_is_numpys(kind, spatial, C, seed):
    seg, values, x = _case(kind, spatial, C, 3500 + 100 * len(spatial) + 10 * C + seed)
    st = S.label_percentiles_statement(seg, x, QS, values)
    K = seg.shape[0] if values is None else len(values)
    assert st['count'].dtype == np.int64 and st['count'].shape == (K,)
    assert st['rank_value'].dtype == np.float32 and st['rank_value'].shape == (K, C, len(QS), 2)
    assert st['rank_weight'].dtype == np.float64 and st['rank_weight'].shape == (K, len(QS))
    assert st['percentile'].dtype == np.float64 and st['percentile'].shape == (K, C, len(QS))
    seen_empty = False
    for k in range(K):
        mask = seg[k] > 0 if values is None else seg == values[k]
        n = int(mask.sum())
        assert st['count'][k] == n
        if n == 0:
            seen_empty = True
            assert not b32(st['rank_value'][k]).any() and not b64(st['rank_weight'][k]).any() and not b64(st['percentile'][k]).any()
            continue
        for c in range(C):
            samples = x[c][mask]
            order = S.float_unkeys(np.sort(S.float_keys(samples)))                     # the brute force: every key sorted
            for p, q in enumerate(QS):
                i, j, t = E.percentile_ranks(n, q)
                assert b32(st['rank_value'][k, c, p, 0]) == b32(order[i]) and b32(st['rank_value'][k, c, p, 1]) == b32(order[j])
                assert b64(st['rank_weight'][k, p]) == b64(t)
                want = np.percentile(samples.astype(np.float64), q)
                assert abs(st['percentile'][k, c, p] - want) <= 1e-12 * abs(want)
    assert seen_empty


def _one(samples, qs):
    """The statement over ONE label that covers a row of samples."""
    x = np.asarray(samples, np.float32).reshape(1, 1, -1)
    return S.label_percentiles_statement(np.ones((1, 1, x.shape[-1]), np.uint8), x, qs)


def test_hand_cases():
    st = _one([3.5], (0, 50, 100))                                                     # n = 1
    assert st['count'][0] == 1 and (st['rank_value'] == 3.5).all() and not st['rank_weight'].any() and (st['percentile'] == 3.5).all()
    st = _one([4.0, 1.0], (50,))                                                       # n = 2 at q = 50
    assert st['rank_value'][0, 0, 0].tolist() == [1.0, 4.0] and st['rank_weight'][0, 0] == 0.5 and st['percentile'][0, 0, 0] == 2.5
    st = _one([5.0, -2.0, 9.0, 0.5], (0, 100))                                         # q = 0 and q = 100
    assert st['percentile'][0, 0].tolist() == [-2.0, 9.0] and st['rank_value'][0, 0, 1].tolist() == [9.0, 9.0]
    st = _one([10.0, 30.0, 20.0, 50.0, 40.0], (25, 50))                                # integral ranks: h = 1 and 2
    assert st['rank_weight'][0].tolist() == [0.0, 0.0] and st['percentile'][0, 0].tolist() == [20.0, 30.0]
    assert st['rank_value'][0, 0, 0].tolist() == [20.0, 30.0]
    st = _one([2.0, 2.0, 2.0, 7.0], (50, 37.5))                                        # ties: equal values are repeated
    assert st['rank_value'][0, 0, 0].tolist() == [2.0, 2.0] and st['percentile'][0, 0].tolist() == [2.0, 2.0]
    st = _one([0.0, -0.0, 0.0, -0.0], (0, 50, 100))                                    # -0.0 right below +0.0
    signs = np.signbit(st['rank_value'][0, 0])
    assert signs.tolist() == [[True, True], [True, False], [False, False]]
    assert np.signbit(st['percentile'][0, 0, 0]) and not np.signbit(st['percentile'][0, 0, 2])
    with np.errstate(all='ignore'):
        st = _one([1.0, np.nan, 3.0], (0, 50))                                         # a NaN under the label
        assert np.isnan(st['percentile'][0, 0]).all()
        st = _one([1.0, np.inf, -np.inf], (0, 50, 100, 25))                            # infinities are ordinary keys
    assert st['percentile'][0, 0, :3].tolist() == [-np.inf, 1.0, np.inf] and st['percentile'][0, 0, 3] == -np.inf
    x = np.ones((2, 1, 3), np.float32); x[1, 0, 1] = np.nan                            # the NaN of one channel leaves the other alone
    st = S.label_percentiles_statement(np.ones((1, 1, 3), np.uint8), x, (50,))
    assert st['percentile'][0, 0, 0] == 1.0 and np.isnan(st['percentile'][0, 1, 0])
    x[1, 0, 1] = 1.0
    seg = np.array([[1, 1, 0]], np.uint8); x[0, 0, 2] = np.nan                         # a NaN under no label is of no consequence
    assert S.label_percentiles_statement(seg[None], x, (50,))['percentile'][0, 0, 0] == 1.0


def test_percentile_of_values_is_numpys_linear_method_spelled_out():
    rng = np.random.default_rng(35)
    for _ in range(200):
        lo, hi = np.sort((rng.normal(size=2) * 10.0 ** rng.integers(-3, 5)).astype(np.float32))
        t = np.float64(rng.random())
        lo64, hi64 = np.float64(lo), np.float64(hi)
        want = lo64 + (hi64 - lo64) * t if t < 0.5 else hi64 - (hi64 - lo64) * (np.float64(1) - t)
        assert b64(S.percentile_of_values(lo, hi, t)) == b64(want)
    assert b64(S.percentile_of_values(np.float32(-0.0), np.float32(5.0), 0.0)) == b64(-0.0)
    assert S.percentile_of_values(np.float32(2.0), np.float32(2.0), 0.7) == 2.0
    # evaluate.percentile_of_ranks is this on the roots
    assert b64(E.percentile_of_ranks(4.0, 9.0, 0.3)) == b64(S.percentile_of_values(2.0, 3.0, 0.3))


def test_the_percentiles_are_checked_as_evaluate_checks_its_own():
    seg, x = np.ones((1, 2, 2), np.uint8), np.ones((1, 2, 2), np.float32)
    for bad in ((-1.0,), (100.5,), (float('nan'),), (float('inf'),), tuple(range(9))):
        with pytest.raises(ValueError, match='percentiles'):
            S.label_percentiles_statement(seg, x, bad)
        with pytest.raises(ValueError, match='percentiles'):
            E._percentiles(bad, 'evaluate')
    with pytest.raises(ValueError, match='intensities'):
        S.label_percentiles_statement(seg, np.ones((1, 2, 3), np.float32), (50,))
    with pytest.raises(ValueError, match='intensities'):
        S.label_percentiles_statement(seg, np.ones((0, 2, 2), np.float32), (50,))


# ------------------------------------------------------------------------------------------------ label_statistics
def _annotated():
    arr = np.array([[2, 2, 0, 4], [2, 0, 0, 4], [2, 2, 2, 0]], np.uint8)
    seg = nrrd.Image(arr, (0.5, 2.0), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 1, {}, None)
    image.set_annotation_meta(seg, {2: 'two', 4: 'four'})
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    return seg, x


def test_label_statistics_with_defaults_is_the_dict_of_before():
    seg, x = _annotated()
    st = S.label_statistics(seg, {'grey': x})
    want_two = {'value': 2, 'exists': True, 'count': 6, 'mm': 6.0, 'bbox': [[0, 0], [2, 2]], 'centroid_index': [7 / 6, 4 / 6],
                'centroid_physical': [0.5 * 4 / 6, 2.0 * 7 / 6], 'intensity': {'grey': {'min': 0.0, 'max': 10.0, 'mean': 32 / 6, 'std': st['two']['intensity']['grey']['std']}}}
    assert list(st) == ['two', 'four']
    for key in want_two:
        assert st['two'][key] == want_two[key], key
    assert sorted(st['two']) == sorted(want_two)
    assert st['two']['intensity']['grey']['std'] == pytest.approx(float(np.std(np.array([0, 1, 4, 8, 9, 10], np.float64))), rel=1e-14)
    assert S.label_statistics(seg, {'grey': x}, percentiles=()) == st
    # with percentiles: the same dict, and 'percentile' beside min, max, mean, std
    got = S.label_statistics(seg, {'grey': x}, percentiles=(50, 25.0))
    for name in st:
        for key in st[name]:
            if key != 'intensity':
                assert got[name][key] == st[name][key]
        assert sorted(got[name]) == sorted(st[name])
        assert {k: v for k, v in got[name]['intensity']['grey'].items() if k != 'percentile'} == st[name]['intensity']['grey']
    assert got['two']['intensity']['grey']['percentile'] == {'50.0': 6.0, '25.0': 1.75}
    assert got['four']['intensity']['grey']['percentile'] == {'50.0': 5.0, '25.0': 4.0}
    assert S.label_statistics(seg, None, percentiles=(50,)) == S.label_statistics(seg)             # no channel: nothing to take a percentile of
    with pytest.raises(ValueError, match='percentiles'):
        S.label_statistics(seg, {'grey': x}, percentiles=(101,))
    with np.errstate(all='ignore'):
        x[0, 0] = np.nan
        e = S.label_statistics(seg, {'grey': x}, percentiles=(50,))
    assert math.isnan(e['two']['intensity']['grey']['percentile']['50.0']) and e['four']['intensity']['grey']['percentile']['50.0'] == 5.0
    # a multi-component segmentation: component v - 1 > 0; its third component is empty
    planes = np.stack([seg.array == 2, seg.array == 4, seg.array == 6]).astype(np.uint8) * 3
    multi = nrrd.Image(np.ascontiguousarray(np.moveaxis(planes, 0, -1)), seg.spacing, seg.origin, seg.direction, 3, {}, None)
    image.set_annotation_meta(multi, {1: 'two', 2: 'four', 3: 'six'})
    x[0, 0] = 0.0
    plain = S.label_statistics(multi, {'grey': x})
    assert plain['six'] == {'value': 3, 'exists': False, 'count': 0, 'mm': 0.0, 'bbox': None, 'centroid_index': None, 'centroid_physical': None,
                            'intensity': {'grey': {'min': None, 'max': None, 'mean': None, 'std': None}}}
    both = S.label_statistics(multi, {'grey': x}, percentiles=(50, 25))
    assert {n: both[n]['intensity'] for n in ('two', 'four')} == {n: got[n]['intensity'] for n in ('two', 'four')}
    assert both['six'] == dict(plain['six'], intensity={'grey': {'min': None, 'max': None, 'mean': None, 'std': None,
                                                                  'percentile': {'50.0': None, '25.0': None}}})          # an empty label


# ------------------------------------------------------------------------------------------------ Result.statistics, save_statistics, the CLI
@pytest.fixture(scope='module')
def one_model():
    m, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_cardiac', 3, 31, mirror=False, feats=(32, 32))
    return {'ts2d-v2-ep4000b2_cardiac': m}


def test_result_statistics_and_the_json_round_trip(tmp_path, one_model):
    with TS2D(models=dict(one_model)) as ts:
        res = ts.predict(os.path.join(A, 'sample_s0521.nrrd'))
        seg, pr = res.get_segmentation(), res.get_projection()
        plain = res.statistics()
        st = res.statistics(percentiles=(5, 50, 95))
        assert all('percentile' not in i for e in plain.values() for i in e['intensity'].values())
        for i, (name, e) in enumerate(st.items()):
            mask = seg.array[..., i] > 0
            for c, got in e['intensity'].items():
                assert {k: v for k, v in got.items() if k != 'percentile'} == plain[name]['intensity'][c]
                assert list(got['percentile']) == ['5.0', '50.0', '95.0']
                for q in (5, 50, 95):
                    if e['count']:
                        want = np.percentile(pr[c].array.reshape(mask.shape)[mask].astype(np.float64), q)
                        assert got['percentile'][repr(float(q))] == pytest.approx(want, rel=1e-12, abs=0)
                    else:
                        assert got['percentile'][repr(float(q))] is None
        assert res.statistics(channels='max', percentiles=(50,))['cardiac_1']['intensity']['max']['percentile'] == \
            {'50.0': st['cardiac_1']['intensity']['max']['percentile']['50.0']}
        files = res.save_statistics(str(tmp_path), 'case', percentiles=(5, 50, 95))
        assert [os.path.basename(f) for f in files] == ['case.statistics.json']
        with open(files[0]) as f:
            assert json.load(f) == st
        with open(res.save_statistics(str(tmp_path / 'plain'), 'case')[0]) as f:
            assert json.load(f) == plain


def test_the_command_line(tmp_path, one_model, monkeypatch, capsys):
    src = tmp_path / 'in'
    os.makedirs(src)
    shutil.copy(os.path.join(A, 'sample_s0521.nrrd'), src / 'one.nrrd')
    main.ts2d_run(str(src), str(tmp_path / 'a'), models=dict(one_model), visualize=False, silent=True, statistics=True, statistics_percentiles=(50.0,))
    main.ts2d_run(str(src), str(tmp_path / 'b'), models=dict(one_model), visualize=False, silent=True, statistics=True)
    with open(tmp_path / 'a' / 'one.statistics.json') as f:
        with_q = json.load(f)
    with open(tmp_path / 'b' / 'one.statistics.json') as f:
        without = json.load(f)
    assert all(list(i['percentile']) == ['50.0'] for e in with_q.values() for i in e['intensity'].values())
    for e in with_q.values():
        for i in e['intensity'].values():
            del i['percentile']
    assert with_q == without
    seen = {}
    monkeypatch.setattr(main, 'ts2d_run', lambda **kw: seen.update(kw))
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--statistics', '--statistics-percentile', '50', '--statistics-percentile', '95'])
    assert seen['statistics'] is True and seen['statistics_percentiles'] == (50.0, 95.0)
    seen.clear()
    main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e'), '--statistics'])
    assert seen['statistics'] is True and 'statistics_percentiles' not in seen      # without the flag: the call of before
    for argv in (['--statistics-percentile', '50'], ['--statistics', '--statistics-percentile', '101'],
                 ['--statistics'] + ['--statistics-percentile', '50'] * 9):
        seen.clear()
        with pytest.raises(SystemExit) as ex:
            main.ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'e')] + argv)
        assert ex.value.code == 2 and not seen and '--statistics-percentile' in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ the shared header and the planner, stand-alone
@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    """tests/label_select_driver.cpp with csrc/stats_plan.cpp as plain C++ behind a main of its own, under the address and undefined-behaviour
    sanitizers where the toolchain links them (nothing loaded into Python runs under a sanitizer)."""
    cxx = HIPCC if os.path.exists(HIPCC) else shutil.which('c++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = tmp_path_factory.mktemp('label_select') / 'label_select_driver'
    base = [cxx, '-x', 'c++', '-O1', '-g', '-std=c++17', '-Wno-unknown-pragmas', '-o', str(exe), os.path.join(ROOT, 'tests', 'label_select_driver.cpp'),
            os.path.join(CSRC, 'stats_plan.cpp')]
    if subprocess.call(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    return str(exe)


def test_the_host_walk_equals_the_statement_bit_for_bit(driver, tmp_path):
    cases = []
    for kind, spatial, C, seed in CASES:
        seg, values, x = _case(kind, spatial, C, 3500 + 100 * len(spatial) + 10 * C + seed)
        K = seg.shape[0] if values is None else len(values)
        for k in range(K):
            for c in range(C):
                cases.append((0, 0, seg[k], x[c], QS, None) if values is None else (1, values[k], seg, x[c], QS, k))
    const = np.full(200, 7.25, np.float32)                                             # one bin in every round; the lowest key byte alone; the top one alone
    low = (np.float32(1.0).view(np.uint32) + np.arange(200, dtype=np.uint32) % 251).view(np.float32)
    top = np.array([1e-30, 1e-10, 1.0, 1e10, 1e30, -1e-30, -1e-10, -1.0, -1e10, -1e30] * 20, np.float32)
    for x in (const, low, top):
        cases.append((0, 0, np.ones(200, np.uint8), x, (0, 5, 50, 95, 100, 37.5, 25, 75), None))
    bad = const.copy(); bad[17] = np.inf
    cases.append((0, 0, np.ones(200, np.uint8), bad, (50,), None))
    path = tmp_path / 'cases.bin'
    with open(path, 'wb') as f:
        for kind, value, m, x, qs, _ in cases:
            f.write(struct.pack('<4i', kind, value, m.size, len(qs))); f.write(np.asarray(qs, np.float64).tobytes())
            f.write(np.ascontiguousarray(m).tobytes()); f.write(np.ascontiguousarray(x, np.float32).tobytes())
    lines = subprocess.run([driver, 'walk', str(path)], check=True, capture_output=True, text=True).stdout.split('\n')[:-1]
    assert len(lines) == len(cases)
    for line, (kind, value, m, x, qs, k) in zip(lines, cases):
        got = [int(v) for v in line.split()]
        if kind == 0:
            st = S.label_percentiles_statement(m[None], x.reshape((1,) + m.shape), qs)
        else:
            st = S.label_percentiles_statement(m, x.reshape((1,) + m.shape), qs, [value])
        want = [int(st['count'][0]), int(not np.isfinite(x.reshape(m.shape)[(m > 0) if kind == 0 else (m == value)]).all())]
        for p in range(len(qs)):
            want += [int(b32(st['rank_value'][0, 0, p, 0])), int(b32(st['rank_value'][0, 0, p, 1])), int(b64(st['rank_weight'][0, p]))]
        assert got == want
    assert lines[-1].split()[1] == '1'                                                 # the infinite sample under the label is reported


def test_the_planner(driver, tmp_path):
    queries = []
    for K in (1, 2, 3, 117, 255):
        for C in (1, 2, 64):
            for P in (1, 3, 8):
                for rows in (1, 337, 32768, 2 ** 31 - 1, 2 ** 24):
                    per = C * 2 * P * (8 + 8 + 1024) + rows * 20                       # the state of one label, as the header of the entry says it
                    for bound in (0, per - 1, per, per + 1, 2 * per, 2 * per + per // 2, 4 * per - 1, K * per, K * per + 1, 1 << 40):
                        queries.append((K, C, P, rows, bound, per))
    path = tmp_path / 'plan.txt'
    path.write_text(''.join(f'{K} {C} {P} {rows} {bound}\n' for K, C, P, rows, bound, _ in queries))
    lines = subprocess.run([driver, 'plan', str(path)], check=True, capture_output=True, text=True).stdout.split('\n')[:-1]
    assert len(lines) == len(queries)
    refused = planned = several = 0
    for line, (K, C, P, rows, bound, per) in zip(lines, queries):
        f = line.split()
        rc, need, budget = int(f[0]), int(f[1]), int(f[2])
        chunks = [tuple(int(v) for v in c.split(':')) for c in f[3:]]
        assert need == per and budget == (bound if bound else 256 << 20)
        if budget < per:
            assert rc == -1 and not chunks                                             # below ONE label: a refusal, nothing planned
            refused += 1
            continue
        assert rc == 0 and chunks[0][0] == 0 and chunks[-1][1] == K
        for (a0, a1), (b0, _) in zip(chunks, chunks[1:]):
            assert a1 == b0                                                            # every label in exactly one chunk, in order
        for k0, k1 in chunks:
            assert k0 < k1 and (k1 - k0) * per <= budget and (k1 - k0) * rows <= 2 ** 31 - 1
        assert len(chunks) == -(-K // min(K, budget // per, (2 ** 31 - 1) // rows))    # no more chunks than the bounds ask for
        planned += 1
        several += len(chunks) > 1
    assert refused and planned and several


def test_the_symbol_is_optional_and_the_abi_version_stays():
    from totalsegmentator2d_amd import _lib
    with open(os.path.join(ROOT, 'include', 'ts2d_engine.h')) as f:
        hdr = f.read()
    assert 'ts2d_label_percentiles' in _lib.SIGNATURES and 'ts2d_label_percentiles' in _lib.OPTIONAL and _lib.ABI_VERSION == 9
    assert f'#define TS2D_STATS_MAX_PERCENTILES {_lib.STATS_MAX_PERCENTILES}\n' in hdr and _lib.STATS_MAX_PERCENTILES == E.MAX_PERCENTILES
    lib = _lib.load()
    assert hasattr(lib, 'ts2d_label_percentiles') and lib.ts2d_abi_version() == 9
