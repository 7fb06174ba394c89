"""Masked normalisation of slice stacks as far as it goes without a GPU: the six-sweep statement of the 3-D hole filling pinned to
``scipy.ndimage.binary_fill_holes`` (and the crop-box argument behind ts2d_planes_crop_normalize_stack_masked), its round counts, the masked statement
pinned to ``crop_to_nonzero`` + ``normalize_channel``, the symbol, and the routing of ``DefaultPreprocessor.run_case_npy`` under the key
``device_normalize_stack_masked`` with a stand-in for the handle."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
import pytest
from scipy.ndimage import binary_fill_holes, gaussian_filter

from tests.prep_schemes_util import CT_PROPS, bits
from tests.stack_masked_util import StackMaskedStandInLib, Z, embed, fill_shapes, serpentine, solid, stack_masked_statement
from tests.test_prep_cpu import _same
from tests.test_stack_cpu import _run
from totalsegmentator2d_amd import _lib
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.model import HIPModel

SHAPES = list(fill_shapes())


def _blob(seed, shape):
    """A head-like mask: a smooth blob with smooth cavities, some of them open to the outside."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing='ij')
    head = zz ** 2 + yy ** 2 + xx ** 2 < 0.8
    return head & (gaussian_filter(rng.standard_normal(shape), 2.5) < 0.04)


# ------------------------------------------------------------------------------------------------ the fill against scipy
@pytest.mark.parametrize('name,data,holes', SHAPES, ids=[s[0] for s in SHAPES])
def test_the_sweeps_equal_scipy_on_the_fill_shapes_inside_the_crop_box(name, data, holes):
    raw = (data != 0).any(axis=0)
    (z0, z1), (r0, r1), (c0, c1) = P.crop_box3_statement(data)
    assert min(z0, r0, c0) > 0                                                       # a non-zero crop offset
    want = binary_fill_holes(raw)                                                    # upstream: the fill of the whole array, then the crop
    got, rounds = P.fill_holes_sweeps_statement(raw[z0:z1, r0:r1, c0:c1])
    assert got.dtype == bool and np.array_equal(got, want[z0:z1, r0:r1, c0:c1]) and not want[:z0].any() and not want[:, :r0].any() and not want[:, :, :c0].any()
    assert (got != raw[z0:z1, r0:r1, c0:c1]).any() == holes and 1 <= rounds <= P.FILL_MAX_ROUNDS
    whole, _ = P.fill_holes_sweeps_statement(raw)
    assert np.array_equal(whole, want)


def test_the_sweeps_equal_scipy_on_random_small_volumes_and_the_box_is_enough():
    rng = np.random.default_rng(7)
    for _ in range(400):
        shape = tuple(rng.integers(1, 10, 3))
        m = rng.random(shape) < rng.uniform(0.2, 0.9)
        want = binary_fill_holes(m)
        got, rounds = P.fill_holes_sweeps_statement(m)
        assert np.array_equal(got, want) and rounds >= 1, (shape, m)
        if m.any():                                                                  # the fill inside the box of the mask = the crop of the fill
            sl = tuple(slice(int(np.flatnonzero(m.any(axis=tuple(i for i in range(3) if i != ax)))[0]),
                             int(np.flatnonzero(m.any(axis=tuple(i for i in range(3) if i != ax)))[-1]) + 1) for ax in range(3))
            assert np.array_equal(P.fill_holes_sweeps_statement(m[sl])[0], want[sl]), (shape, m)
            outside = want.copy(); outside[sl] = False
            assert not outside.any()
    with pytest.raises(ValueError, match='fill_holes_sweeps_statement'):
        P.fill_holes_sweeps_statement(np.zeros((3, 4), bool))


def test_round_counts():
    """What makes the cap of 64 rounds a condition the statement itself meets on every input the device does not hand back."""
    for height, rounds in ((41, 21), (141, 71)):
        raw = (serpentine(height) != 0).any(axis=0)
        got, n = P.fill_holes_sweeps_statement(raw)
        assert n == rounds == (height - 1) // 2 + 1 and np.array_equal(got, binary_fill_holes(raw)), (height, n)
        assert not got[1].all() and got[3].all()                                     # the corridor stays outside, the cavity is filled
    assert 21 <= P.FILL_MAX_ROUNDS < 71 and P.FILL_MAX_ROUNDS == 64
    assert stack_masked_statement(embed(serpentine(141)), [Z, Z], [True, True])[2:] == (P.PLANES_FILL_ROUNDS, 71)
    for seed, shape in ((1, (24, 96, 96)), (2, (16, 128, 128)), (3, (40, 64, 80))):
        m = _blob(seed, shape)
        want = binary_fill_holes(m)
        got, n = P.fill_holes_sweeps_statement(m)
        assert np.array_equal(got, want) and (want != m).sum() > 10 and n < 10, (seed, n)


# ------------------------------------------------------------------------------------------------ the masked statement against the host route
@pytest.mark.parametrize('name,data,holes', SHAPES[5:9], ids=[s[0] for s in SHAPES[5:9]])
def test_the_masked_statement_is_crop_to_nonzero_and_normalize_channel(name, data, holes):
    box, want, status, _ = stack_masked_statement(data, [Z, Z], [True, False])
    assert status == 0
    crop, bbox, mask = P.crop_to_nonzero(data, return_mask=True)
    assert bbox == box
    host = np.stack([P.normalize_channel(crop[0], Z, True, mask, None), P.normalize_channel(crop[1], Z, False, mask, None)])
    assert host.dtype == want.dtype == np.float32 and np.array_equal(bits(want), bits(host))
    raw = stack_masked_statement(data, [Z, Z], [True, False], fill=False)[1]
    assert (bits(raw[0]) != bits(want[0])).any() == holes and np.array_equal(bits(raw[1]), bits(want[1]))


def test_the_chunks_of_the_masked_run_cross_the_slices():
    a = solid(11, 4, 50, 70, c=1)
    a[:, 1:3, 10:20, 10:30] = 0                                                      # a closed cavity ...
    a[:, 0, 0:9, 0:13] = 0                                                           # ... and a corner that stays outside
    data = embed(a)
    box, want, status, rounds = stack_masked_statement(data, [Z], [True])
    n_m = 4 * 50 * 70 - 9 * 13
    assert status == 0 and P.SUM_CHUNK < n_m < 2 * P.SUM_CHUNK and n_m % P.SUM_CHUNK and 2 * 50 * 70 < P.SUM_CHUNK      # the chunk boundary lies inside slice 2
    crop, _, mask = P.crop_to_nonzero(data, return_mask=True)
    assert int(mask.sum()) == n_m and np.array_equal(bits(want[0]), bits(P.normalize_channel(crop[0], Z, True, mask, None)))


# ------------------------------------------------------------------------------------------------ C-ABI
def test_the_entry_is_declared_exported_bound_and_optional():
    hdr = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r'int\s+ts2d_planes_crop_normalize_stack_masked\s*\(([^)]*)\)\s*;', hdr)
    old = re.search(r'int\s+ts2d_planes_crop_normalize_stack\s*\(([^)]*)\)\s*;', hdr)
    assert m and old and [' '.join(p.split()) for p in m.group(1).split(',')] == [' '.join(p.split()) for p in old.group(1).split(',')]
    assert re.search(r'#define\s+TS2D_PLANES_FILL_ROUNDS\s+16\b', hdr) and P.PLANES_FILL_ROUNDS == 16
    assert 'ts2d_planes_crop_normalize_stack_masked' in _lib.OPTIONAL and 'ts2d_planes_crop_normalize_stack_masked' in _lib.SYMBOLS
    lib = _lib.load()
    c = ctypes
    assert hasattr(lib, 'ts2d_planes_crop_normalize_stack_masked')
    assert lib.ts2d_planes_crop_normalize_stack_masked.argtypes == lib.ts2d_planes_crop_normalize_stack.argtypes
    a = np.zeros(8, np.float32)                                                      # refused before any device work: no GPU is needed
    box, status = (c.c_int32 * 6)(*[7] * 6), c.c_int(7)
    assert lib.ts2d_planes_crop_normalize_stack_masked(None, a.ctypes.data, a.ctypes.data, a.ctypes.data, c.byref(box), a.ctypes.data, c.byref(status)) == -1
    assert 'ts2d_planes_crop_normalize_stack_masked: null argument' in _lib.last_error() and list(box) == [7] * 6 and status.value == 7


# ------------------------------------------------------------------------------------------------ routing of run_case_npy
FIP = {'0': CT_PROPS, '1': dict(CT_PROPS, mean=-3, std=11.5)}
ON = {'device_normalize_stack_masked': 2}
PLANS = {'foreground_intensity_properties_per_channel': FIP}


def _stand(monkeypatch, **kw):
    stand = StackMaskedStandInLib(fip=FIP, **kw)
    monkeypatch.setattr(P, 'planes_device_entries', lambda: stand)
    monkeypatch.setattr(P, 'cubic_device_entry', lambda: None)
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    return stand


def _case(seed=21):
    a = solid(seed, 3, 8, 23)
    a[:, 1, 3:5, 5:15] = 0                                                           # a hole
    a[:, 2, 7, 20:23] = 0                                                            # zeros on a face
    return embed(a, (1, 2, 3), (0, 0, 4))                                            # [2, 4, 10, 30], the box [[1, 4], [2, 10], [3, 26]]


CASES = [('masked z-score', dict(use_mask=[True, True])), ('masked + unmasked z-score', dict(use_mask=[True, False])),
         ('CT + masked z-score', dict(schemes=['CTNormalization', Z], use_mask=[True, True], plans=PLANS)),
         ('masked z-score + rescale', dict(schemes=[Z, 'RescaleTo01Normalization'], use_mask=[True, True]))]


@pytest.mark.parametrize('name,kw', CASES, ids=[c[0] for c in CASES])
def test_run_case_npy_takes_the_masked_key_and_returns_the_same_bytes_and_properties(monkeypatch, name, kw):
    stand = _stand(monkeypatch)
    data = _case()
    host = _run(data, (1.5, 1.5), {}, **kw)
    assert stand.calls == []
    dev = _run(data, (1.5, 1.5), ON, **kw)
    assert stand.calls == [('create_stack', 2, 2, 4, 10, 30), ('crop_normalize_stack_masked',), ('download',), ('destroy',)]
    assert _same(dev, host) and 'device_normalize_stack_masked' not in dev[1] and dev[1]['bbox_used_for_cropping'] == [[1, 4], [2, 10], [3, 26]]
    assert dev[1]['shape_after_cropping_and_before_resampling'] == (3, 8, 23) and dev[0].shape == (2, 3, 8, 23)
    # ... which a route without the fill would not return
    raw = stack_masked_statement(data, kw.get('schemes', [Z, Z]), kw['use_mask'], FIP, fill=False)[1]
    assert not np.array_equal(bits(raw), bits(host[0]))
    # off the plan spacing: the resample happens on the handle; every other key beside it changes nothing (their predicates refuse the case)
    del stand.calls[:]
    host = _run(data, (1.0, 0.8), {}, **kw)
    dev = _run(data, (1.0, 0.8), dict(ON, device_resample=2, device_normalize=2, device_normalize_schemes=2, device_normalize_stack=2), **kw)
    assert stand.calls == [('create_stack', 2, 2, 4, 10, 30), ('crop_normalize_stack_masked',), ('resample', 5, 12), ('download',), ('destroy',)] and _same(dev, host)
    assert dev[0].shape == (2, 3, 5, 12) and not stand.planes


def test_without_the_key_or_eligibility_no_call_is_made(monkeypatch):
    stand = _stand(monkeypatch)
    data = _case(22)
    masked = dict(use_mask=[True, True])

    def quiet(d, on, **kw):
        assert _same(_run(d, (1.5, 1.5), on, **kw), _run(d, (1.5, 1.5), {}, **kw)) and stand.calls == [], kw
    quiet(data, {}, **masked)
    quiet(data, {'device_normalize': 0, 'device_normalize_schemes': 0, 'device_resample': 0, 'device_normalize_stack': 0}, **masked)      # the old keys alone
    quiet(data, ON, tf=(0, 2, 1), **masked)                                          # a transposed plan
    quiet(data, ON, tf=(1, 0, 2), **masked)
    quiet(data[:, 1:2], ON, **masked)                                                # Z = 1 is no stack
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', data.size + 1)           # below the size gate
    quiet(data, ON, **masked)
    monkeypatch.setattr(P, 'DEVICE_NORMALIZE_MIN_SAMPLES', 0)
    quiet(data, ON)                                                                  # no masked channel: the key of the unmasked route is not set
    quiet(data, ON, schemes=['CTNormalization'] * 2, use_mask=[True, True], plans=PLANS)      # use_mask on CT is ignored: no masked channel either
    with np.errstate(all='ignore'):
        quiet(data, ON, schemes=['CTNormalization', Z], use_mask=[True, True],
              plans={'foreground_intensity_properties_per_channel': {'0': dict(CT_PROPS, percentile_99_5=1e40)}})
    # without a masked channel the new key leaves the unmasked route to its own key
    assert _same(_run(data, (1.5, 1.5), dict(ON, device_normalize_stack=2)), _run(data, (1.5, 1.5), {}))
    assert stand.calls == [('create_stack', 2, 2, 4, 10, 30), ('crop_normalize_stack',), ('download',), ('destroy',)]
    del stand.calls[:]

    class Old:                                                                       # a library built before the entry
        def __getattr__(self, name):
            if name.endswith('_stack_masked'):
                raise AttributeError(name)
            return getattr(stand, name)
    monkeypatch.setattr(P, 'planes_device_entries', lambda: Old())
    quiet(data, ON, **masked)
    monkeypatch.setattr(P, 'planes_device_entries', lambda: None)
    quiet(data, ON, **masked)


def test_every_status_bit_falls_back_to_the_host_route_and_destroys_the_handle(monkeypatch):
    stand = _stand(monkeypatch)
    three = [('create_stack', 2, 2, 4, 10, 30), ('crop_normalize_stack_masked',), ('destroy',)]
    masked = dict(use_mask=[True, True])
    data = _case(23)
    nan = data.copy(); nan[1, 2, 5, 7] = np.nan
    dev, host = _run(nan, (1.5, 1.5), ON, **masked), _run(nan, (1.5, 1.5), {}, **masked)
    assert np.array_equal(dev[0], host[0], equal_nan=True) and dev[1] == host[1] and stand.calls == three and not stand.planes
    del stand.calls[:]
    zeros = np.zeros_like(data)                                                      # an empty mask: numpy's NaNs, and its warning
    assert stack_masked_statement(zeros, [Z, Z], [True, True])[2] == P.PLANES_EMPTY_MASK
    with pytest.warns(RuntimeWarning):
        dev = P.DefaultPreprocessor(verbose=False).run_case_npy(zeros.copy(), None, dict({'spacing': (2.5, 1.5, 1.5)}, **ON),
                                                                SimpleNamespace(transpose_forward=[0, 1, 2], plans={}),
                                                                SimpleNamespace(spacing=[1.5, 1.5], normalization_schemes=[Z, Z], use_mask_for_norm=[True, True]), {})
    assert stand.calls == three and not stand.planes and dev[0].shape == data.shape
    del stand.calls[:]
    long = embed(serpentine(141))                                                    # 71 rounds: the device gives up, the host route fills
    dev, host = _run(long, (1.5, 1.5), ON, **masked), _run(long, (1.5, 1.5), {}, **masked)
    assert _same(dev, host) and stand.calls == [('create_stack', 2, 2) + long.shape[1:], ('crop_normalize_stack_masked',), ('destroy',)] and not stand.planes
    for bit in (P.PLANES_NONFINITE, P.PLANES_RGB_RANGE, P.PLANES_EMPTY_MASK, P.PLANES_ZERO_SIGN, P.PLANES_FILL_ROUNDS):      # every bit alone, whatever raised it
        forced = _stand(monkeypatch, force_status=bit)
        assert _same(_run(data, (1.5, 1.5), ON, **masked), _run(data, (1.5, 1.5), {}, **masked)) and forced.calls == three and not forced.planes


def test_the_switch_exists_and_the_preprocess_key_tells_the_masked_key():
    m = HIPModel.__new__(HIPModel)
    m._discover = lambda: None
    HIPModel.__init__(m, {'param': {}})
    assert m.device_input_stack_masked is True and m.device_input_stack is True
    p = SimpleNamespace(configuration_manager=SimpleNamespace(spacing=[1.5, 1.5]), plans_manager=SimpleNamespace(), dataset_json={})
    key = HIPModel._preprocess_key
    assert len({key(p, {}), key(p, {'device_normalize_stack_masked': 0}), key(p, {'device_normalize_stack_masked': 1}), key(p, {'device_normalize_stack': 1})}) == 4
