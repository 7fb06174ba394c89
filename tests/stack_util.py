"""Shared by tests/test_stack_cpu.py and tests/test_gpu_stack.py: a stack [C, Z, H, W] under a 2-D plan computed by the numpy statements of
preprocess.py (the box over three axes, every channel normalised as ONE flattened run), and the stand-in library that answers the two stack entries
with it."""
import ctypes

import numpy as np

from tests.prep_schemes_util import SCHEMES, SchemesStandInLib, bits, plane_statement
from totalsegmentator2d_amd import preprocess as P


def volume_statement(vol, scheme, props=None):
    """One channel's cropped volume [Z, h, w] by the statement of its scheme over the flattened, C-ordered run - what numpy reduces."""
    flat = np.ascontiguousarray(vol, np.float32).reshape(1, -1)
    return plane_statement(flat, scheme, False, None, props).reshape(np.shape(vol))


def stack_statement(data, schemes, fip=None):
    """``(box, volume [C, Z', h', w'] or None, status)`` of ts2d_planes_crop_normalize_stack for ``data`` [C, Z, H, W]."""
    box = P.crop_box3_statement(data)
    (z0, z1), (r0, r1), (c0, c1) = box
    vols = [np.ascontiguousarray(data[c, z0:z1, r0:r1, c0:c1]) for c in range(data.shape[0])]
    status = 0
    for v, s in zip(vols, schemes):
        if s == 'RGBTo01Normalization' and (v.min() < 0 or v.max() > 255):
            status |= P.PLANES_RGB_RANGE
        if s == 'RescaleTo01Normalization' and (v == 0).any() and np.signbit(v[v == 0]).any() and not (v < 0).any():
            status |= P.PLANES_ZERO_SIGN
    if status & P.PLANES_RGB_RANGE:
        return box, None, status
    with np.errstate(all='ignore'):
        out = np.stack([volume_statement(v, s, (fip or {}).get(str(c))) for c, (v, s) in enumerate(zip(vols, schemes))])
    if not np.isfinite(out).all():
        status |= P.PLANES_NONFINITE
    return box, (None if status else out), status


def stack_case(seed, c, z, h, w, border=(0, 0, 0, 0, 0, 0), rgb=False):
    """N(0,1) * 30 + 7 inside ``border`` = (front, back, top, bottom, left, right) slices / rows / columns of zeros, every slice scaled by its own
    factor so that the slices' value ranges differ; ``rgb``: integers of 0 ... 255."""
    rng = np.random.default_rng(seed)
    data = np.zeros((c, z, h, w), np.float32)
    f, b, t, bo, l, r = border
    inner = (rng.standard_normal((c, z - f - b, h - t - bo, w - l - r)) * 30 + 7) * (1 + 0.25 * np.arange(z - f - b))[None, :, None, None]
    if rgb:
        inner = rng.integers(1, 256, inner.shape)
    data[:, f:z - b, t:h - bo, l:w - r] = inner.astype(np.float32)
    return data


class StackStandInLib(SchemesStandInLib):
    """The stand-in of tests/prep_schemes_util.py with the two stack entries: the handle's planes are the slices [C * Z, h, w]."""
    def ts2d_planes_create_stack(self, device, src, channels, slices, h, w, out):
        self.calls.append(('create_stack', device, channels, slices, h, w))
        a = np.ctypeslib.as_array(ctypes.cast(src, ctypes.POINTER(ctypes.c_float)), (channels * slices, h, w)).copy()
        out._obj.value = self.next
        self.planes[self.next] = {'a': a, 'lo_hi': None, 'z': slices}
        self.next += 1
        return 0

    def ts2d_planes_crop_normalize_stack(self, hnd, ids, params, use_mask, box, stats, status):
        self.calls.append(('crop_normalize_stack',))
        st = self.planes[hnd.value]
        z = st['z']
        n = len(st['a']) // z
        ids = np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_int32)), (n,))
        params = np.ctypeslib.as_array(ctypes.cast(params, ctypes.POINTER(ctypes.c_float)), (n, 4))
        use_mask = np.ctypeslib.as_array(ctypes.cast(use_mask, ctypes.POINTER(ctypes.c_uint8)), (n,))
        schemes = [SCHEMES[i] for i in ids]
        assert not any(m and s == 'ZScoreNormalization' for m, s in zip(use_mask, schemes)), 'the entry refuses a masked scheme: the caller must not send one'
        for c, s in enumerate(schemes):                       # the parameters that arrive are the statement's
            if s == 'CTNormalization':
                assert np.array_equal(bits(params[c]), bits(P.ct_f32_parameters(self.fip[str(c)])))
        bx, out, code = stack_statement(st['a'].reshape((n, z) + st['a'].shape[1:]), schemes, self.fip)
        code |= self.force_status
        status._obj.value = code
        if code:
            return 0
        st['a'], st['z'] = out.reshape((-1,) + out.shape[2:]), out.shape[1]
        st['lo_hi'] = [(p.min(), p.max()) for p in st['a']]
        for i, v in enumerate(v for b in bx for v in b):
            box._obj[i] = v
        return 0
