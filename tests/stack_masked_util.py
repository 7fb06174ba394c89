"""Shared by tests/test_stack_masked_cpu.py and tests/test_gpu_stack_masked.py: a stack [C, Z, H, W] with a masked z-score channel computed by the numpy
statements of preprocess.py (the box over three axes, the non-zero mask hole-filled by the six-sweep rounds, each masked channel normalised inside it
as ONE flattened run), the volumes with holes both files fill, and the stand-in library that answers ts2d_planes_crop_normalize_stack_masked."""
import ctypes

import numpy as np

from tests.prep_schemes_util import SCHEMES, bits
from tests.stack_util import StackStandInLib, volume_statement
from totalsegmentator2d_amd import preprocess as P

Z = 'ZScoreNormalization'


def stack_masked_statement(data, schemes, use_mask, fip=None, fill=True):
    """``(box, volume [C, Z', h', w'] or None, status, rounds)`` of ts2d_planes_crop_normalize_stack_masked for ``data`` [C, Z, H, W].  ``fill=False``: the
    raw, unfilled mask - what a route that skips the fill would compute."""
    box = P.crop_box3_statement(data)
    (z0, z1), (r0, r1), (c0, c1) = box
    vols = [np.ascontiguousarray(data[c, z0:z1, r0:r1, c0:c1]) for c in range(data.shape[0])]
    masked = [schemes[c] == Z and bool(use_mask[c]) for c in range(len(vols))]
    mask, rounds = np.any([v != 0 for v in vols], axis=0), 0
    if any(masked) and fill:
        mask, rounds = P.fill_holes_sweeps_statement(mask)
        if rounds > P.FILL_MAX_ROUNDS:
            return box, None, P.PLANES_FILL_ROUNDS, rounds
    if any(masked) and not mask.any():
        return box, None, P.PLANES_EMPTY_MASK, rounds
    status = 0
    for v, s in zip(vols, schemes):
        if s == 'RGBTo01Normalization' and (v.min() < 0 or v.max() > 255):
            status |= P.PLANES_RGB_RANGE
        if s == 'RescaleTo01Normalization' and (v == 0).any() and np.signbit(v[v == 0]).any() and not (v < 0).any():
            status |= P.PLANES_ZERO_SIGN
    if status & P.PLANES_RGB_RANGE:
        return box, None, status, rounds
    with np.errstate(all='ignore'):
        out = np.stack([P.masked_zscore_stack_statement(v, mask) if m else volume_statement(v, s, (fip or {}).get(str(c)))
                        for c, (v, s, m) in enumerate(zip(vols, schemes, masked))])
    if not np.isfinite(out).all():
        status |= P.PLANES_NONFINITE
    return box, (None if status else out), status, rounds


def embed(inner, offset=(1, 2, 3), pad=(1, 1, 2)):
    """``inner`` [C, bz, bh, bw] inside zeros: ``offset`` slices / rows / columns before it, ``pad`` after it - a non-zero crop offset on every axis."""
    c, bz, bh, bw = inner.shape
    data = np.zeros((c, bz + offset[0] + pad[0], bh + offset[1] + pad[1], bw + offset[2] + pad[2]), np.float32)
    data[:, offset[0]:offset[0] + bz, offset[1]:offset[1] + bh, offset[2]:offset[2] + bw] = inner
    return data


def solid(seed, bz, bh, bw, c=2):
    """[c, bz, bh, bw] without a zero: N(0,1) * 30 + 7, every slice scaled by its own factor."""
    a = (np.random.default_rng(seed).standard_normal((c, bz, bh, bw)) * 30 + 7) * (1 + 0.25 * np.arange(bz))[None, :, None, None]
    a = a.astype(np.float32)
    a[a == 0] = 1.0
    return a


def serpentine(height, width=7):
    """A one-voxel corridor of zeros, ``height`` rows high, winding through slice 1 of a solid [2, 5, height + 1, width + 2] block: rows 0, 2, 4 ...
    run from column 1 to column ``width``, rows 1, 3, ... are one voxel at alternating ends.  Row 0 lies on a face of the box (the seeds), the last row of
    the block is solid.  The six-sweep rounds advance two rows each: ``(height - 1) // 2 + 1`` rounds, the last one adding nothing.  The whole corridor is
    connected to the face: nothing of it is a hole; the one hole of the block is a closed cavity in slice 3, which no sweep reaches."""
    assert height % 2 == 1
    a = solid(1000 + height, 5, height + 1, width + 2)
    a[:, 3, 2:4, 2:4] = 0
    for k in range(height):
        if k % 2 == 0:
            a[:, 1, k, 1:width + 1] = 0
        else:
            a[:, 1, k, width if (k // 2) % 2 == 0 else 1] = 0
    return a


def fill_shapes():
    """``(name, data [2, Z, H, W], holes)``: the volumes whose masks are filled, each embedded at a non-zero crop offset; ``holes`` tells whether the filled
    mask differs from the raw one."""
    for bw in (23, 64, 70, 128, 130):                    # the tail word, the exact word, a carry across one and across two word boundaries
        a = solid(bw, 4, 6, bw)
        a[:, 1:3, 2:4, 2:bw - 2] = 0                     # a closed cavity nearly as wide as the box
        a[:, 2, 4, bw - 1] = 0                           # ... and a zero voxel on the last column: outside
        yield f'bw = {bw}', embed(a), True
    a = solid(1, 4, 7, 80)
    a[:, 1:3, 3, 62:66] = 0                              # a closed cavity that straddles the word boundary at x = 64
    yield 'a cavity across a word boundary', embed(a), True
    a = solid(2, 2, 6, 9)
    a[:, :, 2:4, 3:6] = 0                                # two slices: every voxel is on a face, nothing is enclosed
    yield 'bz = 2', embed(a), False
    a = solid(3, 3, 6, 9)
    a[:, 1, 2:4, 3:6] = 0
    yield 'bz = 3, a cavity in the middle slice', embed(a), True
    a = solid(4, 4, 6, 9)
    a[:, 1, 0, 0] = 0                                    # a zero voxel on an edge of the box ...
    a[:, 1, 1, 1] = 0                                    # ... and one that touches it only diagonally: still a hole
    yield 'a cavity that touches the outside diagonally', embed(a), True
    a = solid(5, 4, 8, 70)
    a[:, 2, 3, 0:66] = 0                                 # a tunnel open to the face x = 0, across a word boundary: no hole
    a[:, 1, 6, 30:34] = 0                                # (and a closed cavity beside it)
    yield 'a tunnel open to a face', embed(a), True
    a = solid(6, 4, 8, 70)
    a[0, 2, 3, 0:66] = 0                                 # the same tunnel, but non-zero in channel 1: it belongs to the mask
    a[0, 1, 2, 10:14] = 0                                # ... as does a would-be hole that is non-zero there
    a[:, 1, 6, 30:34] = 0
    yield 'a would-be hole and a tunnel that are non-zero in channel 1 only', embed(a), True
    yield 'the 41-high serpentine', embed(serpentine(41)), True


class StackMaskedStandInLib(StackStandInLib):
    """The stand-in of tests/stack_util.py with ts2d_planes_crop_normalize_stack_masked answered by the statements."""
    def ts2d_planes_crop_normalize_stack_masked(self, hnd, ids, params, use_mask, box, stats, status):
        self.calls.append(('crop_normalize_stack_masked',))
        st = self.planes[hnd.value]
        z = st['z']
        n = len(st['a']) // z
        ids = np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_int32)), (n,))
        params = np.ctypeslib.as_array(ctypes.cast(params, ctypes.POINTER(ctypes.c_float)), (n, 4))
        use_mask = np.ctypeslib.as_array(ctypes.cast(use_mask, ctypes.POINTER(ctypes.c_uint8)), (n,))
        schemes = [SCHEMES[i] for i in ids]
        assert any(m and s == Z for m, s in zip(use_mask, schemes)), 'without a masked channel the caller takes the other entry'
        for c, s in enumerate(schemes):
            if s == 'CTNormalization':
                assert np.array_equal(bits(params[c]), bits(P.ct_f32_parameters(self.fip[str(c)])))
        bx, out, code, _ = stack_masked_statement(st['a'].reshape((n, z) + st['a'].shape[1:]), schemes, use_mask, self.fip)
        code |= self.force_status
        status._obj.value = code
        if code:
            return 0
        st['a'], st['z'] = out.reshape((-1,) + out.shape[2:]), out.shape[1]
        st['lo_hi'] = [(p.min(), p.max()) for p in st['a']]
        for i, v in enumerate(v for b in bx for v in b):
            box._obj[i] = v
        return 0
