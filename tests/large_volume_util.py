"""TEST INFRASTRUCTURE (never imported by the product) of tests/test_gpu_large_volumes.py and tests/test_large_volumes_cpu.py: inputs of 2^31
voxels that cost two small islands, their TWINS, and references that a test can afford at such a size.

ISLANDS AND TWINS.  A large input is ``np.zeros`` (untouched pages cost nothing) with two small windows of seeded random labels: one in the first
z-slabs at the low corner, one in the last z-slabs at the high corner, whose last voxel is index n - 1.  The twin is the same volume with empty
z-slabs cut out of the middle (``keep_near`` slabs stay in front, ``keep_far`` behind, each with at least one empty slab beside its island, so the
islands do not come to touch).  Every integer result of the large volume follows from the twin's: counts and x / y results are the twin's; a z index
grows by the removed slabs for what lies in the far island; a linear index (a component's first voxel) by the removed voxels.  Where the removed ROWS
(slabs * H) are a multiple of 64, every surviving row keeps its lane of the level-2 summation tree (csrc/stats_tree.h: lane = row % 64, in
increasing row order), the removed rows contribute +0.0, and the float64 sums keep their bits: :func:`twin_of` asserts it unless told that only
integers are compared.  tests/test_large_volumes_cpu.py proves all of this on the host at moderate size - and that the float sums DO change where
the removed rows are no multiple of 64.

BOXED DISTANCES.  ``evaluate.volume_distance_profile_statement`` is O(voxels * H) in time and O(H * H) / O(W * W) in memory: minutes on a twin of a
few 1024 x 1024 slabs, and 8.6 GB of ``[W, W]`` offsets at an extent of 32767.  :func:`boxed_distance_statement` is the same definition evaluated
only where it is asked for: the statement's own border, line and row passes on a CROP that holds every voxel of the labels (outside it all is
background, which is also what the statement pads with), passes 2 and 3 evaluated - with the statement's operations in the statement's order - only
at the rows and voxels of the own side's border, and the sum's terms placed on the rows and columns of the FULL extent before they meet in
``statistics``'s tree.  tests/test_large_volumes_cpu.py holds it against the statement bit for bit on seeded cases, crops and offsets included.
"""
import time

import numpy as np
import pytest

from totalsegmentator2d_amd import evaluate as E, statistics as S

TAG = '[large-vol]'


# ------------------------------------------------------------------------------------------------------------------ memory
def mem_available() -> int:
    """MemAvailable of /proc/meminfo in bytes (a very large number where the file does not say)."""
    try:
        with open('/proc/meminfo') as f:
            for line in f:
                if line.startswith('MemAvailable:'):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return 1 << 62


def require(tag: str, device_bytes: int, host_bytes: int):
    """Print what the case needs; skip only where the device or the host shows less."""
    import torch
    free, avail = int(torch.cuda.mem_get_info()[0]), mem_available()
    print(f'{TAG} {tag}: needs {device_bytes / 2 ** 30:.2f} GiB on the device ({free / 2 ** 30:.1f} free), {host_bytes / 2 ** 30:.2f} GiB on the host '
          f'({avail / 2 ** 30:.1f} available)')
    if free < device_bytes or avail < host_bytes:
        pytest.skip(f'{tag}: needs {device_bytes} device and {host_bytes} host bytes; {free} and {avail} are there')


class Clock:
    """``with Clock(tag) as c: ...; c.result = ...`` prints the wall time and the result of a case."""

    def __init__(self, tag):
        self.tag, self.result = tag, ''

    def __enter__(self):
        self.t0 = time.time()
        return self

    def __exit__(self, kind, *_):
        print(f'{TAG} {self.tag}: {time.time() - self.t0:.2f} s {"FAILED" if kind else self.result}')


# ------------------------------------------------------------------------------------------------------------------ islands and twins
def _draw(rng, window, values, density):
    pick = np.asarray([0] + [int(v) for v in values], np.uint8)
    return np.where(rng.random(window) < density, pick[rng.integers(1, len(pick), window)], 0).astype(np.uint8)


def two_islands(shape, window, seed, near_values, far_values=None, density=0.45, out=None):
    """A label map [Z, H, W] of zeros with ``window = (slabs, wy, wx)`` of random labels at the low corner (``near_values``) and at the high corner
    (``far_values``, default the same); the last voxel belongs to the last far value.  ``out``: a zero array [Z, H, W] to write them into (a plane)."""
    Z, H, W = shape
    s, wy, wx = window
    far_values = near_values if far_values is None else far_values
    rng = np.random.default_rng(seed)
    big = np.zeros(shape, np.uint8) if out is None else out
    big[:s, :wy, :wx] = _draw(rng, window, near_values, density)
    big[Z - s:, H - wy:, W - wx:] = _draw(rng, window, far_values, density)
    big[-1, -1, -1] = far_values[-1]
    return big


def twin_of(big, keep_near, keep_far, axis=0, integers_only=False):
    """``(twin, removed slabs)``: ``big`` without the z-slabs ``keep_near ... Z - keep_far - 1`` (``axis``: where z is), which must be empty."""
    Z, H = big.shape[axis], big.shape[axis + 1]
    removed = Z - keep_near - keep_far
    assert removed > 0 and (integers_only or removed * H % 64 == 0), (Z, H, keep_near, keep_far)
    front, back = [slice(None)] * big.ndim, [slice(None)] * big.ndim
    front[axis], back[axis] = slice(0, keep_near), slice(Z - keep_far, Z)
    return np.concatenate([big[tuple(front)], big[tuple(back)]], axis=axis), removed


def middle_is_empty(big, keep_near, keep_far, axis=0) -> bool:
    mid = [slice(None)] * big.ndim
    mid[axis] = slice(keep_near, big.shape[axis] - keep_far)
    return int(np.count_nonzero(big[tuple(mid)])) == 0


def shifted_statistics(st: dict, twin, values, keep_near: int, removed: int, Z: int) -> dict:
    """The statement's dict of the large volume from the twin's (``statistics.label_statistics_statement(twin, ...)``; ``values`` None: planes): the
    z index sum grows by (voxels in the far part) * removed, the box's z by removed where that end lies in the far part; an absent label's smallest z
    is the extent.  Everything else - the float64 fields with their bits - stands."""
    out = {k: np.array(v) for k, v in st.items()}
    K = len(out['count'])
    for k in range(K):
        mask = (twin[k] > 0) if values is None else (twin == values[k])
        far = int(np.count_nonzero(mask[keep_near:]))
        if out['count'][k] == 0:
            out['bbox_min'][k, 0] = Z
            continue
        out['index_sum'][k, 0] += far * removed
        if far:
            out['bbox_max'][k, 0] += removed
        if far == out['count'][k]:
            out['bbox_min'][k, 0] += removed
    return out


def same_dict(got: dict, want: dict, fields) -> bool:
    return all(np.asarray(got[f]).dtype == np.asarray(want[f]).dtype and np.asarray(got[f]).tobytes() == np.asarray(want[f]).tobytes() for f in fields)


def shifted_components(want, twin_voxels_near: int, removed_voxels: int):
    """The statement's component list of the large volume from the twin's: a first voxel at or past the twin's near part moves by the removed
    voxels.  (The order - label, size descending, first voxel - stands: the far roots stay above the near ones.)"""
    rows = want.copy()
    rows[rows[:, 1] >= twin_voxels_near, 1] += removed_voxels
    return rows


# ------------------------------------------------------------------------------------------------------------------ boxed distances
def _d2_volume_at_border(own, other, spacing):
    """``evaluate.d2_from_planes(own, plane_distance(line_distance(other)))`` evaluated only at the rows and voxels of ``own``: the same float64
    operations in the same order (f = (d * s) * (d * s); (f_z + f_y), its minimum over y'; + f_x, its minimum over x')."""
    sz, sy, sx = (np.float64(v) for v in spacing)
    Z, H, W = own.shape
    g = E.line_distance(other)
    with np.errstate(invalid='ignore'):
        rz = np.where(g < 0, np.inf, g.astype(np.float64)) * sz
        fz = rz * rz
    zs, ys, xs = np.nonzero(own)
    out = np.empty(len(zs), np.float64)
    ay, ax = np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64)
    h_of = {}
    for i, (z, y, x) in enumerate(zip(zs.tolist(), ys.tolist(), xs.tolist())):
        if (z, y) not in h_of:
            ry = np.abs(y - ay).astype(np.float64) * sy
            h_of = {(z, y): (fz[z] + (ry * ry)[:, None]).min(axis=0)}          # (np.nonzero order: a row's voxels follow each other)
        rx = np.abs(x - ax).astype(np.float64) * sx
        out[i] = (h_of[z, y] + rx * rx).min()
    return out


def _d2_plane_at_border(own, other, spacing_hw):
    """``evaluate.d2_from_rows(own, row_distance(other))`` without its ``[W, W]`` table: the same operations per border pixel."""
    sy, sx = np.float64(spacing_hw[0]), np.float64(spacing_hw[1])
    g = E.row_distance(other)
    with np.errstate(invalid='ignore'):
        ry = np.where(g < 0, np.inf, g.astype(np.float64)) * sy
        dy2 = ry * ry
    ys, xs = np.nonzero(own)
    ax = np.arange(own.shape[1], dtype=np.int64)
    out = np.empty(len(ys), np.float64)
    for i, (y, x) in enumerate(zip(ys.tolist(), xs.tolist())):
        rx = np.abs(x - ax).astype(np.float64) * sx
        out[i] = (dy2[y] + rx * rx).min()
    return out


def boxed_distance_statement(a, kind_a, b, kind_b, values, spacing, tolerances, percentiles, origin=None, full_shape=None, want_sum=True):
    """``evaluate.volume_distance_profile_statement`` (3 spatial axes) or ``evaluate.distance_profile_statement`` (2) of the FULL extent
    ``full_shape`` whose only labelled voxels lie in the crop ``a``, ``b`` at ``origin`` (defaults: the crop is the extent) - the module
    docstring says how.  The same keys, dtypes and bits (``want_sum`` False: ``dist_sum`` stays zero, for extents whose tree alone takes seconds)."""
    a, b, spatial, K = E._sides(a, kind_a, b, kind_b, values)
    nd = len(spatial)
    origin = (0,) * nd if origin is None else tuple(origin)
    full = tuple(spatial) if full_shape is None else tuple(full_shape)
    qs = E._percentiles(percentiles, 'boxed_distance_statement')
    tol = np.asarray(list(tolerances), np.float64)
    tol_sq = tol * tol
    T, P = len(tol), len(qs)
    border = E.border_of_volume if nd == 3 else E.border_of
    d2_of = _d2_volume_at_border if nd == 3 else _d2_plane_at_border
    full_rows = int(np.prod(full[:-1]))
    out = {'border': np.zeros((K, 2), np.int64), 'd2_max': np.full((K, 2), -np.inf, np.float64), 'within': np.zeros((K, 2, T), np.int64),
           'dist_sum': np.zeros((K, 2), np.float64), 'd2_rank': np.full((K, 2, P, 2), -np.inf, np.float64), 'rank_weight': np.zeros((K, 2, P), np.float64)}
    for k in range(K):
        ba, bb = border(E._mask(a, kind_a, values, k)), border(E._mask(b, kind_b, values, k))
        for d, (own, other) in enumerate(((ba, bb), (bb, ba))):
            n = int(np.count_nonzero(own))
            out['border'][k, d] = n
            if n == 0:
                continue
            d2 = d2_of(own, other, spacing)
            out['d2_max'][k, d] = d2.max()
            for t in range(T):
                out['within'][k, d, t] = np.count_nonzero(d2 <= tol_sq[t])
            # the sum: the terms of the crop's rows on the full extent's columns (level 1), their partials on the full extent's rows (level 2)
            if want_sum:
                at = np.nonzero(own)
                row = (at[0] + origin[0]) * full[1] + at[1] + origin[1] if nd == 3 else at[0] + origin[0]
                live, inverse = np.unique(row, return_inverse=True)
                terms = np.zeros((len(live), full[-1]), np.float64)
                terms[inverse, at[-1] + origin[-1]] = np.sqrt(d2)
                partial = np.zeros(full_rows, np.float64)
                partial[live] = S._lanes(terms)
                out['dist_sum'][k, d] = np.float64(S._lanes(partial))
            ordered = np.sort(d2)
            for p, q in enumerate(qs):
                i, j, t = E.percentile_ranks(n, q)
                out['d2_rank'][k, d, p] = ordered[i], ordered[j]
                out['rank_weight'][k, d, p] = t
    return out


DISTANCE_FIELDS = ('border', 'within', 'd2_max', 'dist_sum', 'd2_rank', 'rank_weight')
STATISTICS_FIELDS = ('count', 'index_sum', 'bbox_min', 'bbox_max', 'sum', 'ssq', 'mean', 'std', 'min', 'max')
PERCENTILE_FIELDS = ('count', 'rank_value', 'rank_weight', 'percentile')
