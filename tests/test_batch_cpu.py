"""The batched surface without a GPU: TS2D.predict_many / HIPModel.apply_batch / the ``--batch-cases`` CLI flag over the host restatement
(tests/batch_util.py), and the C-ABI binding of ts2d_engine_predict_tiled_batch as far as it goes without a device."""
import ctypes
import os
import re
import shutil
import threading

import numpy as np
import pytest

from tests.batch_util import synthetic_batch_model
from tests.conftest import GOLDEN
from totalsegmentator2d_amd import _lib, nrrd
from totalsegmentator2d_amd.main import ts2d_entry_point, ts2d_run
from totalsegmentator2d_amd.tool import TS2D

A = os.path.join(GOLDEN, 'assets')
CT = [os.path.join(A, n) for n in ('sample_s0521.nrrd', 'sample_s0616.nrrd', 'sample_s0332.nrrd')]


@pytest.fixture(scope='module')
def two_models():
    m1, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_cardiac', 3, 31, mirror=False, feats=(32, 32))
    m2, _, _ = synthetic_batch_model('ts2d-v2-ep4000b2_ribs', 4, 32, mirror=False, feats=(32, 32))
    return {'ts2d-v2-ep4000b2_cardiac': m1, 'ts2d-v2-ep4000b2_ribs': m2}


def _same_image(a, b):
    return (type(a) is type(b) and np.array_equal(a.array, b.array) and a.array.dtype == b.array.dtype and a.spacing == b.spacing
            and a.origin == b.origin and a.direction == b.direction and a.components == b.components and a.meta == b.meta)


def _same_result(a, b):
    assert a.models == b.models
    for m in [None] + a.models:
        sa, sb = a.get_segmentation(m), b.get_segmentation(m)
        assert (sa is None) == (sb is None) and (sa is None or _same_image(sa, sb)), m
        ia, ib = a.get_input(m), b.get_input(m)
        assert (ia is None) == (ib is None) and (ia is None or _same_image(ia, ib)), m
    assert sorted(a.get_projection()) == sorted(b.get_projection())
    for c in a.get_projection():
        assert _same_image(a.get_projection(c), b.get_projection(c))


@pytest.mark.parametrize('kw', [{}, {'merge': False}, {'collapse': True}])
def test_predict_many_equals_predict_per_case(two_models, kw):
    """3-D volume, native 2-D two-channel image, pre-projected vector image: each result equals predict() of that case exactly."""
    with TS2D(models=dict(two_models)) as ts:
        single = [ts.predict(p, **kw) for p in CT]
        for max_cases in (1, 2, 8):
            many = ts.predict_many(CT, max_cases=max_cases, **kw)
            assert len(many) == 3
            for a, b in zip(many, single):
                _same_result(a, b)
        if kw.get('merge') is False:
            assert many[0].get_segmentation() is None
        assert ts.predict_many([]) == []


def test_predict_many_names_the_case_with_the_wrong_channel_count(two_models):
    with TS2D(models=dict(two_models)) as ts:
        with pytest.raises(RuntimeError, match='number of channels'):
            ts.predict_many([CT[1], os.path.join(A, 'sample_chexpert.nrrd')])
        with pytest.raises(RuntimeError, match='input must be a string path or an image'):
            ts.predict_many([CT[1], 5])


class _StubModel:
    """The members TS2D touches, around an ``apply`` the test controls."""
    channels, multilabel, revision, colors = {0: 'mean', 1: 'max'}, True, 'r000', {}

    def __init__(self, apply):
        self.apply, self.timestamps = apply, {}

    def start(self, wait=True):
        pass

    await_startup = stop = lambda self: None


def test_predict_waits_for_every_running_sub_model_before_it_raises():
    """A sub-model fails at once while another is still at work: predict() raises that failure, but not before the other has finished
    (C-ABI: one caller thread per engine - the caller may start the next case on the same handles as soon as it has control)."""
    running, release, finished = threading.Event(), threading.Event(), threading.Event()

    def failing(img):
        running.wait(10)                      # (the other sub-model has started: it cannot be cancelled any more)
        raise ValueError('device lost')

    def slow(img):
        running.set()
        release.wait(10)
        finished.set()
        return img

    img = nrrd.Image(np.zeros((8, 8, 2), np.float32), (1.5, 1.5), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), components=2)
    outcome = []

    def call(ts):
        try:
            ts.predict(img)
        except BaseException as ex:
            outcome.append((ex, finished.is_set()))

    with TS2D(models={'a_fails': _StubModel(failing), 'b_slow': _StubModel(slow)}) as ts:
        t = threading.Thread(target=call, args=(ts,))
        t.start()
        try:
            assert running.wait(10)
            t.join(0.3)
            assert t.is_alive() and not outcome        # the failure is there, the second sub-model still runs: predict() holds on
        finally:
            release.set()
            t.join(10)
    assert not t.is_alive() and len(outcome) == 1
    ex, second_had_finished = outcome[0]
    assert isinstance(ex, ValueError) and str(ex) == 'device lost' and second_had_finished


def test_apply_batch_stage_errors_timestamps_and_override(tmp_path, two_models):
    m = two_models['ts2d-v2-ep4000b2_cardiac']
    m.start()
    try:
        good = nrrd.read(CT[1])
        bad = nrrd.Image(np.zeros((8, 8, 3), np.float32), (1.5, 1.5), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), components=3)
        with pytest.raises(RuntimeError, match=r'^(Preprocessing|Prediction) failed for second: '):
            m.apply_batch({'first': good, 'second': bad})
        with pytest.raises(RuntimeError, match=r'^Preprocessing failed for nofile: '):
            m.apply_batch({'first': good, 'nofile': str(tmp_path / 'missing.nrrd')})
        # a failing network: the stage and the input of the batch it failed for
        p = m._predictor
        net, calls = p._network, []

        def failing(batch, fold=0):
            calls.append(1)
            if len(calls) == 2:
                raise ValueError('device lost')
            return net(batch, fold)
        p._network = failing
        try:
            with pytest.raises(RuntimeError, match=r'^Prediction failed for b: input 1: device lost'):
                m.apply_batch({'a': good, 'b': good, 'c': good})
        finally:
            p._network = net
        out = m.apply_batch({'a': good, 'b': good}, result_dir=str(tmp_path / 'r'))
        assert out == {'a': str(tmp_path / 'r' / 'a.nrrd'), 'b': str(tmp_path / 'r' / 'b.nrrd')}
        assert m.timestamps == m.batch_timestamps['b']
        one = m.apply(good, result_dir=str(tmp_path / 's'))
        assert open(out['a'], 'rb').read() == open(one, 'rb').read() == open(out['b'], 'rb').read()
        for name in ('a', 'b'):
            ts = m.batch_timestamps[name]
            assert ts['start'] <= ts['preprocessed'] <= ts['predicted'] <= ts['exported'] <= ts['done']
        assert m.batch_timestamps['a']['predicted'] == m.batch_timestamps['b']['predicted']
        # override=False: existing outputs are skipped before any network call
        calls.clear()
        p._network = failing
        try:
            again = m.apply_batch({'a': good, 'b': good}, result_dir=str(tmp_path / 'r'), override=False)
        finally:
            p._network = net
        assert again == out and not calls and 'preprocessed' not in m.batch_timestamps['a']
        lst = m.apply_batch([good, good])
        assert list(lst) == ['image1', 'image2'] and np.array_equal(lst['image1'].array, m.apply(good).array)
    finally:
        m.stop()


def test_cli_batch_cases_writes_the_same_files(tmp_path, two_models, capsys):
    src = tmp_path / 'in'
    os.makedirs(src)
    for p in CT:
        shutil.copy(p, src / os.path.basename(p))
    ts2d_run(str(src), str(tmp_path / 'one'), models=dict(two_models), visualize=False, save_all=True)
    log_one = capsys.readouterr().out
    ts2d_run(str(src), str(tmp_path / 'two'), models=dict(two_models), visualize=False, save_all=True, batch_cases=2)
    log_two = capsys.readouterr().out
    assert sorted(log_one.splitlines()) == sorted(log_two.splitlines()) and '[3/3] Processing: sample_s0616' in log_two
    names = sorted(os.listdir(tmp_path / 'one'))
    assert names == sorted(os.listdir(tmp_path / 'two')) and len(names) >= 9
    for n in names:
        assert open(tmp_path / 'one' / n, 'rb').read() == open(tmp_path / 'two' / n, 'rb').read(), n
    with pytest.raises(SystemExit):
        ts2d_entry_point(['-i', str(src), '-o', str(tmp_path / 'x'), '--batch-cases', '0'])


def test_tiled_image_binding_matches_the_header_layout():
    """ctypes layout of ts2d_tiled_image against the header's field order under the C rules for an LP64 target, and the entry without a GPU."""
    src = open(_lib.HEADER_PATH).read()
    body = re.search(r'typedef struct \{([^}]*)\} ts2d_tiled_image;', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.rsplit(None, 1)[0], decl.rsplit(None, 1)[1]
        ptr = '*' in decl
        for n in [x.strip() for x in decl.replace('*', ' ').split(None, 2 if decl.startswith('const') else 1)[-1].split(',')]:
            fields.append((n, 8 if ptr else 4))
    assert [n for n, _ in fields] == ['image', 'Hp', 'Wp', 'n_tiles', 'tile_y', 'tile_x', 'logits_f16', 'seg_u8', 'inf_flag']
    off = 0
    for n, size in fields:
        off = (off + size - 1) // size * size
        assert getattr(_lib.TiledImage, n).offset == off and getattr(_lib.TiledImage, n).size == size, n
        off += size
    assert ctypes.sizeof(_lib.TiledImage) == (off + 7) // 8 * 8 == 64
    assert [f[0] for f in _lib.TiledImage._fields_] == [n for n, _ in fields]
    lib = _lib.load()
    assert 'ts2d_engine_predict_tiled_batch' in _lib.SYMBOLS and lib.ts2d_abi_version() == _lib.ABI_VERSION == 9
    desc = (_lib.TiledImage * 1)()
    assert lib.ts2d_engine_predict_tiled_batch(None, desc, 1, 64, 64, 0, None) == -1
    assert 'null engine' in _lib.last_error()
