"""Shared by tests/test_prep_schemes_cpu.py and tests/test_gpu_prep_schemes.py: a case of ts2d_planes_crop_normalize computed by the numpy statements
of preprocess.py, the stand-in library that answers the entry with it, and the planes both files normalise."""
import ctypes

import numpy as np

from tests.test_prep_cpu import _StandInLib
from totalsegmentator2d_amd import preprocess as P

SCHEMES = tuple(P.NORM_SCHEME_IDS)
CT_PROPS = {'percentile_00_5': -50.0, 'percentile_99_5': 60.0, 'mean': 5.0, 'std': 20.0}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def plane_statement(plane, scheme, masked, mask, props):
    """One channel by its statement (what preprocess.normalize_channel computes of it)."""
    if scheme == 'ZScoreNormalization':
        return P.masked_zscore_f32_statement(plane, mask) if masked else P.zscore_f32_statement(plane)
    if scheme == 'CTNormalization':
        return P.ct_f32_statement(plane, props)
    if scheme == 'RescaleTo01Normalization':
        return P.rescale01_f32_statement(plane)
    if scheme == 'RGBTo01Normalization':
        return P.rgb01_f32_statement(plane)
    assert scheme == 'NoNormalization'
    return np.ascontiguousarray(plane, np.float32).copy()


def case_statement(data, schemes, use_mask, fip):
    """``(box, planes [C, 1, h, w] or None, status)`` of ts2d_planes_crop_normalize for ``data`` [C, 1, H, W]: the statements, and the PLANES_* bits
    where the entry answers with them instead."""
    box = P.crop_box_statement(data)
    (_, _), (r0, r1), (c0, c1) = box
    planes = [np.ascontiguousarray(data[c, 0, r0:r1, c0:c1]) for c in range(data.shape[0])]
    mask = np.any([p != 0 for p in planes], axis=0)
    masked = [schemes[c] == 'ZScoreNormalization' and bool(use_mask[c]) for c in range(len(planes))]
    status = 0
    if any(masked) and not mask.any():
        status |= P.PLANES_EMPTY_MASK
    for p, s in zip(planes, schemes):
        if s == 'RGBTo01Normalization' and (p.min() < 0 or p.max() > 255):
            status |= P.PLANES_RGB_RANGE
        if s == 'RescaleTo01Normalization' and (p == 0).any() and np.signbit(p[p == 0]).any() and not (p < 0).any():
            status |= P.PLANES_ZERO_SIGN
    if status & (P.PLANES_EMPTY_MASK | P.PLANES_RGB_RANGE):
        return box, None, status
    with np.errstate(all='ignore'):
        out = np.stack([plane_statement(p, s, m, mask, (fip or {}).get(str(c))) for c, (p, s, m) in enumerate(zip(planes, schemes, masked))])[:, None]
    if not np.isfinite(out).all():
        status |= P.PLANES_NONFINITE
    return box, (None if status else out), status


class SchemesStandInLib(_StandInLib):
    """tests/test_prep_cpu.py's stand-in for the ts2d_planes_* entries, with ts2d_planes_crop_normalize computed by the numpy statements."""
    def __init__(self, fip=None, force_status=0):
        super().__init__()
        self.fip, self.force_status = fip or {}, force_status

    def ts2d_planes_crop_normalize(self, hnd, ids, params, use_mask, box, stats, status):
        self.calls.append(('crop_normalize',))
        st = self.planes[hnd.value]
        n = len(st['a'])
        ids = np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_int32)), (n,))
        params = np.ctypeslib.as_array(ctypes.cast(params, ctypes.POINTER(ctypes.c_float)), (n, 4))
        use_mask = np.ctypeslib.as_array(ctypes.cast(use_mask, ctypes.POINTER(ctypes.c_uint8)), (n,))
        schemes = [SCHEMES[i] for i in ids]
        for c, s in enumerate(schemes):                       # the parameters that arrive are the statement's
            if s == 'CTNormalization':
                assert np.array_equal(bits(params[c]), bits(P.ct_f32_parameters(self.fip[str(c)])))
        bx, out, code = case_statement(st['a'][:, None], schemes, use_mask, self.fip)
        code |= self.force_status
        status._obj.value = code
        if code:
            return 0
        st['a'] = out[:, 0]
        st['lo_hi'] = [(p.min(), p.max()) for p in st['a']]
        for i, v in enumerate((bx[1][0], bx[1][1], bx[2][0], bx[2][1])):
            box._obj[i] = v
        return 0


def planes_of_every_kind(rng, h, w):
    """(name, plane): N(0,1) * 30 + 7, integer-valued, constant, all-zero, high-dynamic-range, -0.0 and denormals, values on and beyond CT_PROPS' bounds."""
    yield 'normal', (rng.standard_normal((h, w)) * 30 + 7).astype(np.float32)
    yield 'ints', rng.integers(0, 256, (h, w)).astype(np.float32)
    yield 'constant', np.full((h, w), np.float32(rng.standard_normal() * 100), np.float32)
    yield 'zero', np.zeros((h, w), np.float32)
    yield 'hdr', (rng.standard_normal((h, w)) * 10.0 ** rng.uniform(-6, 6, (h, w))).astype(np.float32)
    tiny = rng.choice(np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, -3e-41, 1.5, -2.0], np.float32), (h, w))
    yield 'zeros and denormals', tiny
    yield 'negative zero', np.full((h, w), -0.0, np.float32)
    edge = rng.choice(np.array([-50.0, 60.0, np.nextafter(np.float32(-50), np.float32(-60)), np.nextafter(np.float32(60), np.float32(70)), -51.0, 61.0, 0.0, -0.0,
                                1e4, -1e4, 59.999996, -49.999996], np.float32), (h, w))
    yield 'on and beyond the bounds', edge
