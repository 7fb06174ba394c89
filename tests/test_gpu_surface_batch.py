"""The batched surface on the MI355X engine: HIPModel.apply_batch and TS2D.predict_many against apply / predict.  Inside a batched engine
call the network always takes the full-batch dispatch, so the oracle for bit equality is the per-case surface on engines created with
'sbk': 0; against the default per-case surface (small-batch dispatch) the results agree to fp32 summation order."""
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import nrrd
from totalsegmentator2d_amd.engine import Engine
from totalsegmentator2d_amd.tool import TS2D

pytestmark = pytest.mark.gpu
A = os.path.join(GOLDEN, 'assets')
CT = [os.path.join(A, n) for n in ('sample_s0521.nrrd', 'sample_s0616.nrrd', 'sample_s0332.nrrd')]
IDS = ('ts2d-v2-ep4000b2_cardiac', 'ts2d-v2-ep4000b2_muscles', 'ts2d-v2-ep4000b2_ribs')


def _models(sbk_off):
    """Three synthetic sub-models; sbk_off: their engines are created with the small-batch dispatch off (the bit-for-bit twin)."""
    old = dict(Engine.default_options)
    if sbk_off:
        Engine.default_options = {**old, 'sbk': 0}
    try:
        models = {m: synthetic_model(m, 3 + 2 * i, 41 + i, patch=(64, 64), mirror=True)[0] for i, m in enumerate(IDS)}
        for m in models.values():
            m.start()                          # (engines are created here, under the options above)
    finally:
        Engine.default_options = old
    return models


def test_apply_batch_equals_apply_on_an_sbk_off_model(tmp_path):
    twin = _models(True)[IDS[0]]
    model = _models(False)[IDS[0]]
    try:
        imgs = {n: nrrd.read(CT[1]) for n in ('a', 'b')}
        imgs['c'] = nrrd.Image(np.ascontiguousarray(imgs['a'].array[:300, :200]), imgs['a'].spacing, imgs['a'].origin, imgs['a'].direction,
                               imgs['a'].components, {}, None)
        got = model.apply_batch(dict(imgs))
        for n, img in imgs.items():
            want = twin.apply(img)
            assert np.array_equal(got[n].array, want.array) and got[n].meta == want.meta
            ts = model.batch_timestamps[n]
            assert ts['start'] <= ts['preprocessed'] <= ts['predicted'] <= ts['exported'] <= ts['done']
        files = model.apply_batch(dict(imgs), result_dir=str(tmp_path / 'batch'))
        for n, img in imgs.items():
            one = twin.apply({n: img}, result_dir=str(tmp_path / 'single'))[n]
            assert open(files[n], 'rb').read() == open(one, 'rb').read()
    finally:
        twin.stop()
        model.stop()


def test_predict_many_equals_predict():
    with TS2D(models=_models(False)) as ts, TS2D(models=_models(True)) as twin:
        many = ts.predict_many(CT)
        for path, a in zip(CT, many):
            b = twin.predict(path)
            assert a.models == b.models == sorted(IDS)
            for m in [None] + list(IDS):
                sa, sb = a.get_segmentation(m), b.get_segmentation(m)
                assert np.array_equal(sa.array, sb.array) and sa.meta == sb.meta and sa.size == sb.size, (path, m)
            # the default per-case path (small-batch dispatch): only pixels whose half logit sits at the threshold may differ
            c = ts.predict(path)
            assert (a.get_segmentation().array != c.get_segmentation().array).mean() < 2e-3
            assert a.get_segmentation().meta == c.get_segmentation().meta
        for max_cases in (1, 2):
            other = ts.predict_many(CT, max_cases=max_cases)
            for a, b in zip(many, other):
                for m in [None] + list(IDS):
                    assert np.array_equal(a.get_segmentation(m).array, b.get_segmentation(m).array), (max_cases, m)
