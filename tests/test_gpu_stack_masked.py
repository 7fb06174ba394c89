"""Masked normalisation of slice stacks on the MI355X: ts2d_planes_crop_normalize_stack_masked (csrc/kernels_prep_fill.h, kernels_prep_stack.h) against the
numpy statements (tests/stack_masked_util.py; tests/test_stack_masked_cpu.py pins them to scipy's binary_fill_holes and to normalize_channel) - the
box, every bit of every float32 result, the statistics, the status bits - and DefaultPreprocessor.run_case_npy under the key against the host route."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests.prep_schemes_util import CT_PROPS, bits
from tests.stack_masked_util import embed, fill_shapes, serpentine, solid, stack_masked_statement
from totalsegmentator2d_amd import preprocess as P

pytestmark = pytest.mark.gpu
FIP = {str(c): dict(CT_PROPS, mean=5.0 + c, std=20.0 - 3 * c) for c in range(2)}
Z, CT, RS, RGB, NO = P.NORM_SCHEME_IDS
SHAPES = list(fill_shapes())


def _check(data, schemes, use_mask, holes=True):
    """The entry against the statement: box, bytes, statistics; and the statement with the raw, unfilled mask differs - a route that skips the fill fails."""
    C = data.shape[0]
    box, want, status, rounds = stack_masked_statement(data, schemes, use_mask, FIP)
    assert status == 0 and 1 <= rounds <= P.FILL_MAX_ROUNDS, (status, rounds)
    raw = stack_masked_statement(data, schemes, use_mask, FIP, fill=False)[1]
    assert (not np.array_equal(bits(raw), bits(want))) == holes
    (z0, z1), (r0, r1), (c0, c1) = box
    mask = P.fill_holes_sweeps_statement((data[:, z0:z1, r0:r1, c0:c1] != 0).any(axis=0))[0]
    with P.DevicePlanes(data, 0, stack=True) as p:
        assert p.crop_normalize_stack_masked(schemes, use_mask, FIP) == box and p.status == 0 and p.shape == want.shape and p.slices == z1 - z0
        got = p.download()
        diff = bits(got) != bits(want)
        assert not diff.any(), (data.shape, box, int(diff.sum()), np.argwhere(diff)[:4])
        for c, s in enumerate(schemes):
            vol = np.ascontiguousarray(data[c, z0:z1, r0:r1, c0:c1])
            if s == Z:
                run = vol[mask] if use_mask[c] else vol.reshape(-1)
                assert np.array_equal(bits(p.stats[c]), bits(np.array(P.zscore_stats_f32_statement(run.reshape(1, -1))[:2]))), c
            elif s == CT:
                assert np.array_equal(bits(p.stats[c]), bits(P.ct_f32_parameters(FIP[str(c)])[:2]))
    return got


@pytest.mark.parametrize('name,data,holes', SHAPES, ids=[s[0] for s in SHAPES])
def test_the_fill_shapes_equal_the_statement(name, data, holes):
    assert min(b[0] for b in P.crop_box3_statement(data)) > 0                        # a non-zero crop offset
    _check(data, [Z, Z], [True, True], holes)
    if 'serpentine' in name:                                                         # 21 rounds of the 64 the entry runs
        assert stack_masked_statement(data, [Z, Z], [True, True])[3] == 21


def test_a_masked_run_above_one_chunk_that_is_no_multiple_of_it():
    a = solid(31, 4, 50, 70, c=1)
    a[:, 1:3, 10:20, 10:30] = 0
    a[:, 0, 0:9, 0:13] = 0                                                           # n_m = 14000 - 117: the chunk boundary lies inside a slice
    _check(embed(a), [Z], [True])


@pytest.mark.parametrize('schemes,use_mask', [([Z, CT], [True, True]), ([CT, Z], [False, True]), ([Z, Z], [True, False]), ([Z, Z], [False, True]),
                                              ([Z, RS], [True, True]), ([NO, Z], [True, True])],
                         ids=['masked + CT', 'CT + masked', 'masked + unmasked', 'unmasked + masked', 'masked + rescale', 'none + masked'])
def test_mixed_schemes(schemes, use_mask):
    a = solid(32, 5, 37, 70)
    a[:, 1:4, 10:20, 30:68] = 0
    a[:, 2, 30, 0:5] = 0
    _check(embed(a), schemes, use_mask)


def _run_case(data, spacing, extra, use_mask=(True, True)):
    pm = SimpleNamespace(transpose_forward=[0, 1, 2], plans={'foreground_intensity_properties_per_channel': FIP})
    cm = SimpleNamespace(spacing=[1.5, 1.5], normalization_schemes=[Z, Z], use_mask_for_norm=list(use_mask))
    props = dict({'spacing': (3.0,) + tuple(spacing)}, **extra)
    with np.errstate(all='ignore'):
        out, _, props = P.DefaultPreprocessor(verbose=False).run_case_npy(data.copy(), None, props, pm, cm, {})
    return out, props


ON = {'device_normalize_stack_masked': 0, 'device_normalize_stack': 0, 'device_resample': 0}


def test_an_off_spacing_case_through_run_case_npy_with_the_resample_on_the_handle(monkeypatch):
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    calls = []
    orig = P.DevicePlanes.crop_normalize_stack_masked
    monkeypatch.setattr(P.DevicePlanes, 'crop_normalize_stack_masked', lambda s, *a, **kw: (lambda box: (calls.append(box), box)[1])(orig(s, *a, **kw)))
    a = solid(33, 3, 40, 30)
    a[:, 1, 10:20, 8:22] = 0
    data = embed(a)
    (host, ph), (dev, pd) = _run_case(data, (1.0, 0.8), {}), _run_case(data, (1.0, 0.8), ON)
    assert calls == [[[1, 4], [2, 42], [3, 33]]] and dev.shape == host.shape == (2, 3, 27, 16) and np.array_equal(bits(dev), bits(host)) and pd == ph
    (host, ph), (dev, pd) = _run_case(data, (1.5, 1.5), {}, (True, False)), _run_case(data, (1.5, 1.5), ON, (True, False))      # ... and on the plan spacing
    assert len(calls) == 2 and dev.shape == (2, 3, 40, 30) and np.array_equal(bits(dev), bits(host)) and pd == ph


def test_status_bits(monkeypatch):
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    long = embed(serpentine(141))                                                    # 71 rounds: more than the entry runs
    assert stack_masked_statement(long, [Z, Z], [True, True])[2:] == (P.PLANES_FILL_ROUNDS, 71)
    with P.DevicePlanes(long, 0, stack=True) as p:
        assert p.crop_normalize_stack_masked([Z, Z], [True, True], FIP) is None and p.status == P.PLANES_FILL_ROUNDS
    with P.DevicePlanes(long, 0, stack=True) as p:                                   # ... which the fill alone raises: no masked channel, no fill
        assert p.crop_normalize_stack_masked([Z, Z], [False, False], FIP) is not None and p.status == 0
    (host, ph), (dev, pd) = _run_case(long, (1.5, 1.5), {}), _run_case(long, (1.5, 1.5), ON)
    assert np.array_equal(bits(dev), bits(host)) and pd == ph
    a = solid(34, 4, 20, 30)
    a[:, 1:3, 5:9, 5:9] = 0
    nan = embed(a); nan[1, 2, 7, 17] = np.nan
    with P.DevicePlanes(nan, 0, stack=True) as p:
        assert p.crop_normalize_stack_masked([Z, Z], [True, True], FIP) is None and p.status == P.PLANES_NONFINITE
    (host, ph), (dev, pd) = _run_case(nan, (1.5, 1.5), {}), _run_case(nan, (1.5, 1.5), ON)
    assert np.array_equal(bits(dev), bits(host)) and pd == ph and np.isnan(host).any()
    zeros = np.zeros((2, 3, 20, 30), np.float32); zeros[1, 2, 3, 4] = -0.0
    with P.DevicePlanes(zeros, 0, stack=True) as p:
        assert p.crop_normalize_stack_masked([Z, Z], [True, True], FIP) is None and p.status == P.PLANES_EMPTY_MASK
    with P.DevicePlanes(zeros, 0, stack=True) as p:                                  # ... which is the masked scheme's alone
        assert p.crop_normalize_stack_masked([Z, CT], [False, True], FIP) == [[0, 3], [0, 20], [0, 30]] and p.status == 0


def test_more_than_2_24_masked_samples():
    rng = np.random.default_rng(35)
    data = (rng.standard_normal((1, 65, 520, 500), np.float32) * 30 + 7).astype(np.float32)
    data[data == 0] = 1.0
    data[0, 20:40, 100:300, 100:400] = 0                                             # a closed cavity of 1.2 M voxels
    data[0, 0, :50, :50] = 0                                                         # and a corner that stays outside
    box, want, status, rounds = stack_masked_statement(data, [Z], [True])
    assert status == 0 and data.size - 2500 > 1 << 24
    with P.DevicePlanes(data, 0, stack=True) as p:
        assert p.crop_normalize_stack_masked([Z], [True], FIP) == box and p.status == 0
        got = p.download()
        assert np.array_equal(bits(got), bits(want))
        assert got[0, 30, 200, 200] != 0 and got[0, 0, 10, 10] == 0                  # the cavity is normalised, the corner is not
