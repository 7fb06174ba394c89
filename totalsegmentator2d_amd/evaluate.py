"""Score a segmentation against a reference: the label projection of a 3-D label volume, overlap counts (Dice, IoU, precision, recall) and, for
2-D planes, boundary distances (surface Dice, Hausdorff distance; on request its percentiles - HD95 - and the average surface distances).

The functions ``*_statement`` and :func:`project_labels` are the project's definition - written in numpy, they are the host route and the
oracle of the device route (C-ABI ``ts2d_project_labels_coronal``, ``ts2d_label_overlap``, ``ts2d_surface_distances``,
``ts2d_surface_distance_profile`` - the two are one path, the first the second without its extras -; ``csrc/kernels_evaluate.h``,
``csrc/kernels_evaluate_profile.h``), which reproduces them bit for bit, as
``statistics.py``, ``visual.py`` and ``postprocess.py`` are for their entries.

LABEL PROJECTION.  TotalSegmentator 2D is trained and evaluated on 3-D label volumes projected into one binary plane per label: the reference's
``project(..., 'multiclass:<num>')`` (``ts2d/core/util/image.py:164-194``, ``_project_multiclass``).  :func:`project_labels` restates it.  Its
result is a vector image, so it has a function of its own: ``image.project`` keeps refusing the mode.

CONFUSION MATRIX.  What a structure was taken for: :func:`confusion_statement` counts, for every pair of a row of one side and a row of the other
(none of the labels, each label, every sample), the samples in both; :func:`confusion` reports it with rows the reference and columns the
prediction.  Device route: C-ABI ``ts2d_label_confusion`` (``csrc/kernels_confusion.h``), one integer matrix product; the same integers.

KINDS.  A segmentation is handed over as planes ``[K, *spatial]`` (label ``k`` is ``planes[k] > 0``) or as a label map ``[*spatial]`` with
``values[K]`` (label ``k`` is ``map == values[k]``) - the two kinds of ``ts2d_label_statistics`` -, and the two sides may be mixed.

BORDER AND DISTANCE (2-D).  A border pixel of a mask is a foreground pixel with at least one of its four neighbours background; outside the image
counts as background (``mask & ~scipy.ndimage.binary_erosion(mask)``).  For a border pixel ``p`` of A

    d2(p) = min over border pixels q of B of ((|py - qy| * sy) * (|py - qy| * sy) + (|px - qx| * sx) * (|px - qx| * sx))

in float64, every product and the sum rounded on their own (no fused multiply-add), ``+inf`` where B has no border.  The minimum of a set does
not depend on order, so the bits are a function of the input alone.  The statement computes it by the exact two-pass decomposition the kernels use
(``csrc/surface_dist.h`` has the argument): per column the integer row distance ``g`` to the nearest border pixel of B, then per border pixel the
minimum over the columns ``x'`` of the formula with ``|py - qy| = g(py, x')``.  tests/test_evaluate_cpu.py holds it against the brute force over
all border pairs, bit for bit.

BORDER AND DISTANCE (3-D; on request: ``evaluate(..., volume_distances=True)``, :func:`volume_surface_statement`,
:func:`volume_distance_profile_statement`; device route C-ABI ``ts2d_volume_surface_distances``, ``csrc/kernels_evaluate_volume.h``).  A border
voxel of a mask ``[Z, H, W]`` is a foreground voxel with at least one of its SIX face neighbours background, outside the volume being background
(``mask & ~scipy.ndimage.binary_erosion(mask)`` with the default 3-D cross; :func:`border_of_volume`).  With ``Z == 1`` every foreground voxel is
therefore a border voxel: that is what the definition says, it is not the 2-D border, and :func:`evaluate` never sends a unit-axis image there.
With ``f(n, s) = (n * s) * (n * s)`` (two roundings), for a border voxel ``p`` of A

    d2(p) = min over border voxels q of B of ((f(|pz - qz|, sz) + f(|py - qy|, sy)) + f(|px - qx|, sx))

in float64, that association, every operation rounded on its own, ``+inf`` where B has no border.  Three exact passes (``csrc/surface_dist.h``
has the argument: ``f`` is monotone in ``n`` and ``u -> fl(u + v)`` is monotone in ``u``, so a line's nearest voxel gives the line's smallest
candidate and the minimum over ``y'`` commutes with adding the x term): per line ``(y', x')`` along z the integer ``g(z, y', x')`` to the
nearest border voxel of B on the line (:func:`line_distance`); per ``(z, y, x')`` the float64
``h = min over y' of (f(g(z, y', x'), sz) + f(|y - y'|, sy))`` (:func:`plane_distance`); per border voxel of A
``d2 = min over x' of (h(pz, py, x') + f(|px - x'|, sx))`` (:func:`d2_from_planes`).  tests/test_evaluate_volume_cpu.py holds them against the
brute force over all border pairs, bit for bit.  The sum of a volume's profile is ``statistics.tree_sum`` over the terms as ``[Z * H, W]``.
"""
from __future__ import annotations

import json
import math
from typing import Dict, Optional, Sequence

import numpy as np

from .nrrd import Image

PLANES, LABELMAP = 0, 1          # _lib.STATS_PLANES, _lib.STATS_LABELMAP: the kinds of ts2d_label_statistics
MAX_TOLERANCES = 8               # _lib.EVAL_MAX_TOLERANCES
MAX_PERCENTILES = 8              # _lib.EVAL_MAX_PERCENTILES
_AXES = {'a': 2, 'ax': 2, 'axial': 2, 's': 0, 'sag': 0, 'sagittal': 0, 'c': 1, 'cor': 1, 'coronal': 1}
# No size gate: the device route lost at no measured size, the small end included - 117 labels at 53 x 133 take 0.17 ms (overlap) and 0.56 ms
# (distances) there against 0.38 ms and 25.6 ms for the statements; the narrowest win is the overlap of 18 labels at 600 x 512, 0.56 ms against
# 0.69 ... 0.87 ms (scripts/gpu_evaluate_case.py, profiles/r29_evaluate_case.txt).  The distance profile likewise: 0.65 ... 0.70 ms against 32 ms
# there, 4.7 ms against 990 ms for 117 labels at 644 x 337 (scripts/gpu_evaluate_profile_case.py, profiles/r30_distance_profile_case.txt).


# ------------------------------------------------------------------------------------------------------------------ label projection
def project_labels(img: Image, num: int, axis='coronal') -> Image:
    """The reference's ``project(img, 'multiclass:<num>', axis)`` (``_project_multiclass``, image.py:164-194).

    Scalar integer volume (:166-188): the result has ``num`` uint8 components; component ``k`` is 1 where any sample of the ray along ``axis``
    equals ``k + 1`` (:177-181: the non-zero samples scatter a 1 into plane ``value - 1``), else 0.  The projected axis keeps size 1 and its
    origin, as in ``image.project`` (:97-100).  Multi-component input (:189-193): the per-component maximum along the axis, in the input type.

    The result has the layout of a multilabel segmentation as ``TS2D`` returns it (plane-major memory behind the ``[..., label]`` view; a scalar
    image for ``num = 1``), so it goes straight to ``statistics.label_statistics`` and to :func:`evaluate`.

    A sample outside ``0 ... num`` raises ``ValueError``.  (The reference raises ``IndexError`` for a sample above ``num`` and silently WRAPS a
    negative one: ``-1 - 1`` indexes plane ``num - 2`` from the end.  Neither is a result.)  ``num`` runs from 1 to 255; a float volume raises
    ``ValueError``."""
    ax = _AXES[axis.lower()] if isinstance(axis, str) else list(range(img.dimension))[axis]
    npax = img.dimension - 1 - ax
    a = img.array
    if img.components > 1:
        r = a.max(axis=npax, keepdims=True)
        return Image(np.ascontiguousarray(r), img.spacing, img.origin, img.direction, img.components, dict(img.meta), img.space)
    num = _check_num(num)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"project_labels: a label volume has an integer type, found {a.dtype}")
    if a.size and (int(a.min()) < 0 or int(a.max()) > num):
        raise ValueError(f"project_labels: the volume holds samples outside 0 ... {num} (minimum {int(a.min())}, maximum {int(a.max())})")
    moved = np.moveaxis(a, npax, 0)                                          # the ray first, as the reference has it (:175)
    idx = np.nonzero(moved)
    planes = np.zeros((num, 1) + moved.shape[1:], np.uint8)
    planes[(moved[idx].astype(np.intp) - 1, 0) + idx[1:]] = 1                # (:177-181; every sample is inside 1 ... num here)
    return _planes_image(np.moveaxis(planes, 1, npax + 1), img)


def _check_num(num) -> int:
    n = int(num)
    if not 1 <= n <= 255:
        raise ValueError(f"project_labels: num = {num} outside 1 ... 255")
    return n


def _planes_image(planes: np.ndarray, like: Image, spacing=None, origin=None, direction=None) -> Image:
    num = planes.shape[0]
    arr = planes[0] if num == 1 else np.moveaxis(planes, 0, -1)
    return Image(arr, like.spacing if spacing is None else spacing, like.origin if origin is None else origin,
                 like.direction if direction is None else direction, num, dict(like.meta), like.space)


def device_projects(img: Image) -> bool:
    """Does ``ts2d_project_labels_coronal`` serve the volume?  A scalar 3-D volume of an integer type of the device projection, and a library that
    has the symbol."""
    from . import engine
    from .image import _GPU_DTYPES
    if img.dimension != 3 or img.components != 1 or img.array.dtype.name not in _GPU_DTYPES or not np.issubdtype(img.array.dtype, np.integer):
        return False
    return engine.has_entry('ts2d_project_labels_coronal')


def project_labels_coronal_gpu(img: Image, num: int, device: int = 0) -> Image:
    """``project_labels(reorient_image(img), num, 'coronal')`` on the device (C-ABI ``ts2d_project_labels_coronal``), without the host
    reorientation copy: the entry reads the reoriented strided view of ``image._coronal_view``.  One pass over the volume whatever ``num`` is.
    A sample outside ``0 ... num`` is a status bit of the entry and raises the statement's ``ValueError``: there is no silent fall-back."""
    from . import _lib, engine
    from .image import _coronal_view, _reoriented_geometry
    num = _check_num(num)
    if not device_projects(img):
        raise RuntimeError(f"project_labels_coronal_gpu needs a scalar 3-D volume of type int16, uint8, uint16 or int32 and a library with "
                           f"ts2d_project_labels_coronal, found {img.array.dtype} with {img.components} components in {img.dimension}-D")
    a, (nz, ny, nx), strides, base, perm, flips = _coronal_view(img)
    planes, status = engine.project_labels_coronal(a, (nz, ny, nx), strides, base, num, device)
    if status & _lib.LABELS_RANGE:
        raise ValueError(f"project_labels: the volume holds samples outside 0 ... {num}")
    geo = _reoriented_geometry(img, perm, flips)
    return _planes_image(planes.reshape(num, nz, 1, nx), img, tuple(img.spacing[ax] for ax in perm), geo[0], geo[1])


# ------------------------------------------------------------------------------------------------------------------ the statements
def _sides(a, kind_a, b, kind_b, values):
    a, b = np.asarray(a), np.asarray(b)
    for kind in (kind_a, kind_b):
        if kind not in (PLANES, LABELMAP):
            raise ValueError(f"kind {kind} is neither planes ({PLANES}) nor label map ({LABELMAP})")
    if LABELMAP in (kind_a, kind_b) and values is None:
        raise ValueError("a label map needs the values of its labels")
    sa = a.shape[1:] if kind_a == PLANES else a.shape
    sb = b.shape[1:] if kind_b == PLANES else b.shape
    if tuple(sa) != tuple(sb):
        raise ValueError(f"the two segmentations differ in shape: {tuple(sa)} and {tuple(sb)}")
    ks = [x.shape[0] for x, kind in ((a, kind_a), (b, kind_b)) if kind == PLANES] + ([len(values)] if values is not None else [])
    if len(set(ks)) != 1:
        raise ValueError(f"the two segmentations and the values differ in their number of labels: {ks}")
    return a, b, tuple(sa), ks[0]


def _mask(x: np.ndarray, kind: int, values, k: int) -> np.ndarray:
    return (x[k] > 0) if kind == PLANES else (x == values[k])


def overlap_statement(a, kind_a: int, b, kind_b: int, values=None) -> dict:
    """THE DEFINITION of the overlap counts.  ``a`` and ``b``: each plane-major ``[K, *spatial]`` (kind ``PLANES``) or a label map ``[*spatial]``
    with ``values[K]`` (kind ``LABELMAP``), of one spatial shape.  Returns int64 arrays over the K labels: ``n_a``, ``n_b`` (the samples of the
    label on either side) and ``n_both`` (the samples of the label on both)."""
    a, b, _, K = _sides(a, kind_a, b, kind_b, values)
    out = {f: np.zeros(K, np.int64) for f in ('n_a', 'n_b', 'n_both')}
    for k in range(K):
        ma, mb = _mask(a, kind_a, values, k), _mask(b, kind_b, values, k)
        out['n_a'][k], out['n_b'][k], out['n_both'][k] = np.count_nonzero(ma), np.count_nonzero(mb), np.count_nonzero(ma & mb)
    return out


def confusion_statement(a, kind_a: int, b, kind_b: int, values=None) -> np.ndarray:
    """THE DEFINITION of the confusion (co-occurrence) matrix.  ``a``, ``b``, the kinds and ``values`` exactly as in :func:`overlap_statement`.
    Returns int64 ``[K + 2, K + 2]``.  Either side has ``K + 2`` indicator rows over the ``N`` samples: row ``1 + k`` is the mask of label ``k``;
    row ``0`` is "none of the K labels" (planes: every plane is 0 there; a label map: the byte is not among ``values``); row ``K + 1`` is every
    sample - the margins.  ``M[i][j]`` is the number of samples in row ``i`` of ``a`` and in row ``j`` of ``b``.

    So ``M[1 + k][1 + k]``, ``M[1 + k][K + 1]`` and ``M[K + 1][1 + k]`` are ``n_both``, ``n_a`` and ``n_b`` of :func:`overlap_statement`, and
    ``M[K + 1][K + 1] == N``.  Between two label maps with distinct ``values`` every sample is in exactly one of the first ``K + 1`` rows of either
    side: the inner ``(K + 1)²`` block sums to ``N`` and its row sums are the margins.  With a planes side a sample can be in several rows and the
    inner block may sum to more than ``N``: that is the definition, not an error."""
    a, b, _, K = _sides(a, kind_a, b, kind_b, values)

    def rows(x, kind):
        masks = [np.asarray(_mask(x, kind, values, k)).reshape(-1) for k in range(K)]
        none = ~np.logical_or.reduce(masks)
        return [none] + masks + [np.ones(none.shape, bool)]
    ra, rb = rows(a, kind_a), rows(b, kind_b)
    out = np.zeros((K + 2, K + 2), np.int64)
    for i, x in enumerate(ra):
        if not x.any():
            continue                                                                     # an empty row meets nothing
        for j, y in enumerate(rb):
            out[i, j] = np.count_nonzero(x & y)
    return out


def border_of(mask: np.ndarray) -> np.ndarray:
    """The border pixels of a 2-D mask: foreground with at least one of the four neighbours background, outside the image being background."""
    m = np.asarray(mask, bool)
    p = np.pad(m, 1)
    return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def row_distance(border: np.ndarray) -> np.ndarray:
    """Pass 1: int64 [H, W], per pixel the row distance ``|y - y'|`` to the nearest border pixel of its COLUMN (a downward and an upward scan);
    -1 where the column has none."""
    H, W = border.shape
    big = np.int64(1) << 40
    y = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(border, y, -big), axis=0)                     # the nearest border row at or above
    below = np.minimum.accumulate(np.where(border, y, big)[::-1], axis=0)[::-1]          # ... at or below
    g = np.minimum(y - above, below - y)
    return np.where(g >= H, -1, g)


def d2_from_rows(border_a: np.ndarray, g_b: np.ndarray, spacing_hw) -> np.ndarray:
    """Pass 2: float64 d2 of every border pixel of A (in ``np.nonzero`` order) from the row distances of B's border."""
    sy, sx = np.float64(spacing_hw[0]), np.float64(spacing_hw[1])
    H, W = border_a.shape
    ys, xs = np.nonzero(border_a)
    with np.errstate(invalid='ignore'):
        ry = np.where(g_b < 0, np.inf, g_b.astype(np.float64)) * sy
        dy2 = ry * ry                                                                    # [H, W]: (g * sy) * (g * sy), +inf without a border
    rx = np.abs(np.arange(W, dtype=np.int64)[:, None] - np.arange(W, dtype=np.int64)[None, :]).astype(np.float64) * sx
    dx2 = rx * rx                                                                        # [W, W]: (|x - x'| * sx) * (|x - x'| * sx)
    out = np.empty(len(ys), np.float64)
    step = max(1, (1 << 22) // max(W, 1))
    for i in range(0, len(ys), step):
        out[i:i + step] = (dy2[ys[i:i + step]] + dx2[xs[i:i + step]]).min(axis=1)
    return out


def border_of_volume(mask: np.ndarray) -> np.ndarray:
    """The border voxels of a 3-D mask: foreground with at least one of the six face neighbours background, outside the volume being background."""
    m = np.asarray(mask, bool)
    if m.ndim != 3:
        raise ValueError(f"border_of_volume: a mask [Z, H, W], found the extent {m.shape}")
    p = np.pad(m, 1)
    return m & ~(p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])


def line_distance(border: np.ndarray) -> np.ndarray:
    """Pass 1 of a volume: int64 [Z, H, W], per voxel ``|z - z'|`` to the nearest border voxel of its LINE along z (:func:`row_distance` with the
    lines as its columns); -1 where the line has none."""
    Z, H, W = border.shape
    return row_distance(border.reshape(Z, H * W)).reshape(Z, H, W)


def plane_distance(g: np.ndarray, sz, sy, chunk_bytes: int = 1 << 25) -> np.ndarray:
    """Pass 2 of a volume: float64 [Z, H, W], ``h(z, y, x') = min over y' of (f(g(z, y', x'), sz) + f(|y - y'|, sy))``, ``+inf`` without a
    candidate.  Chunked over z, so no ``[Z, H, H, W]`` is allocated at once."""
    sz, sy = np.float64(sz), np.float64(sy)
    Z, H, W = g.shape
    with np.errstate(invalid='ignore'):
        rz = np.where(g < 0, np.inf, g.astype(np.float64)) * sz
        fz = rz * rz                                                                     # [Z, H(y'), W]
    ry = np.abs(np.arange(H, dtype=np.int64)[:, None] - np.arange(H, dtype=np.int64)[None, :]).astype(np.float64) * sy
    fy = ry * ry                                                                         # [H(y), H(y')]
    h = np.empty((Z, H, W), np.float64)
    step = max(1, chunk_bytes // max(8 * H * H * W, 1))
    for z in range(0, Z, step):
        h[z:z + step] = (fz[z:z + step, None, :, :] + fy[None, :, :, None]).min(axis=2)
    return h


def d2_from_planes(border_a: np.ndarray, h_b: np.ndarray, sx) -> np.ndarray:
    """Pass 3 of a volume: float64 d2 of every border voxel of A (in ``np.nonzero`` order) from pass 2 of B's border."""
    sx = np.float64(sx)
    W = border_a.shape[2]
    zs, ys, xs = np.nonzero(border_a)
    rx = np.abs(np.arange(W, dtype=np.int64)[:, None] - np.arange(W, dtype=np.int64)[None, :]).astype(np.float64) * sx
    dx2 = rx * rx
    out = np.empty(len(zs), np.float64)
    step = max(1, (1 << 22) // max(W, 1))
    for i in range(0, len(zs), step):
        out[i:i + step] = (h_b[zs[i:i + step], ys[i:i + step]] + dx2[xs[i:i + step]]).min(axis=1)
    return out


def _percentiles(percentiles, who: str) -> list:
    qs = [float(q) for q in percentiles]
    if len(qs) > MAX_PERCENTILES or any(not (math.isfinite(q) and 0.0 <= q <= 100.0) for q in qs):
        raise ValueError(f"{who}: at most {MAX_PERCENTILES} percentiles, each finite and in 0 ... 100, found {qs}")
    return qs


def percentile_ranks(n: int, q: float):
    """``(i, j, t)``: the sorted positions and the weight of percentile ``q`` among ``n >= 1`` values - ``h = (n - 1) * (q / 100)`` in float64,
    ``i = min(floor(h), n - 1)``, ``j = min(i + 1, n - 1)``, ``t = h - i`` (``sd_percentile_ranks`` of csrc/surface_dist.h)."""
    h = np.float64(n - 1) * (np.float64(q) / np.float64(100))
    i = min(int(np.floor(h)), n - 1)
    return i, min(i + 1, n - 1), np.float64(h - np.float64(i))


def percentile_of_ranks(d2_i, d2_j, t) -> np.float64:
    """The percentile of the DISTANCES from the two selected squared distances and the weight (:func:`percentile_ranks`): numpy's linear method
    spelled out, every operation rounded on its own.  ``lo = sqrt(d2_i)``, ``hi = sqrt(d2_j)``; ``lo`` where ``t == 0`` or ``hi == lo``, else
    ``lo + (hi - lo) * t`` for ``t < 0.5`` and ``hi - (hi - lo) * (1 - t)`` from there.  Infinite distances give ``inf`` (``np.percentile`` gives
    NaN as soon as one is in the set), and the index arithmetic does not depend on the numpy at hand."""
    lo, hi, t = np.sqrt(np.float64(d2_i)), np.sqrt(np.float64(d2_j)), np.float64(t)
    if t == 0 or hi == lo:
        return lo
    if t < 0.5:
        return lo + (hi - lo) * t
    return hi - (hi - lo) * (np.float64(1) - t)


def _distance_walk(who: str, a, kind_a: int, b, kind_b: int, values, spacing, tolerances: Sequence[float], qs: Optional[list],
                   volume: bool = False) -> dict:
    """The ONE walk over the labels and the two directions behind :func:`surface_statement` (``qs`` None: border, d2_max, within, and neither a
    root nor a sort is taken) and :func:`distance_profile_statement` (``qs`` the checked percentiles: also dist_sum, d2_rank, rank_weight), and
    with ``volume`` behind :func:`volume_surface_statement` and :func:`volume_distance_profile_statement`: the dimension chooses the border, the
    passes of ``d2`` and the rows of the sum's tree, and nothing else."""
    a, b, spatial, K = _sides(a, kind_a, b, kind_b, values)
    if volume:
        if len(spatial) != 3 or min(spatial) < 1:
            raise ValueError(f"{who}: boundary distances of volumes are defined for [Z, H, W], found the extent {tuple(spatial)}")
        sz, sy, sx = spacing
        border, rows = border_of_volume, (spatial[0] * spatial[1], spatial[2])

        def d2_of(own, other):
            return d2_from_planes(own, plane_distance(line_distance(other), sz, sy), sx)
    else:
        if len(spatial) == 3 and spatial[0] == 1:
            spatial = spatial[1:]
            a = a.reshape((K,) + spatial if kind_a == PLANES else spatial)
            b = b.reshape((K,) + spatial if kind_b == PLANES else spatial)
        if len(spatial) != 2:
            raise ValueError(f"{who}: boundary distances are defined for 2-D planes, found the extent {tuple(spatial)}")
        border, rows = border_of, spatial

        def d2_of(own, other):
            return d2_from_rows(own, row_distance(other), spacing)
    tol = np.asarray(list(tolerances), np.float64)
    tol_sq = tol * tol
    T = len(tol)
    out = {'border': np.zeros((K, 2), np.int64), 'd2_max': np.full((K, 2), -np.inf, np.float64), 'within': np.zeros((K, 2, T), np.int64)}
    if qs is not None:
        from .statistics import tree_sum
        P = len(qs)
        out.update(dist_sum=np.zeros((K, 2), np.float64), d2_rank=np.full((K, 2, P, 2), -np.inf, np.float64),
                   rank_weight=np.zeros((K, 2, P), np.float64))
    for k in range(K):
        ba, bb = border(_mask(a, kind_a, values, k)), border(_mask(b, kind_b, values, k))
        for d, (own, other) in enumerate(((ba, bb), (bb, ba))):
            n = int(np.count_nonzero(own))
            out['border'][k, d] = n
            if n == 0:
                continue
            d2 = d2_of(own, other)
            out['d2_max'][k, d] = d2.max()
            for t in range(T):
                out['within'][k, d, t] = np.count_nonzero(d2 <= tol_sq[t])
            if qs is None:
                continue
            terms = np.zeros(spatial, np.float64)
            terms[own] = np.sqrt(d2)                                                     # (np.nonzero order on both sides)
            out['dist_sum'][k, d] = tree_sum(terms.reshape(rows))
            ordered = np.sort(d2)
            for p, q in enumerate(qs):
                i, j, t = percentile_ranks(n, q)
                out['d2_rank'][k, d, p] = ordered[i], ordered[j]
                out['rank_weight'][k, d, p] = t
    return out


def surface_statement(a, kind_a: int, b, kind_b: int, values, spacing_hw, tolerances: Sequence[float]) -> dict:
    """THE DEFINITION of the boundary distances of 2-D planes (module docstring).  ``a``, ``b``: planes ``[K, 1, H, W]`` / ``[K, H, W]`` or label
    maps ``[1, H, W]`` / ``[H, W]``; a volume (``Z > 1``) raises ``ValueError``.  ``spacing_hw``: (mm per row, mm per column).

    Returns over the K labels and the two directions (0: A to B, 1: B to A): ``border`` int64 [K, 2] (the border pixels of the direction's own
    side), ``d2_max`` float64 [K, 2] (``-inf`` for an empty border, ``+inf`` where the other side has none) and ``within`` int64 [K, 2, T]: per
    tolerance ``t`` (mm) the border pixels with ``d2 <= t * t``, the square taken once in float64."""
    return _distance_walk('surface_statement', a, kind_a, b, kind_b, values, spacing_hw, tolerances, None)


def distance_profile_statement(a, kind_a: int, b, kind_b: int, values, spacing_hw, tolerances: Sequence[float], percentiles: Sequence[float]) -> dict:
    """THE DEFINITION of the distance profile: the inputs, the refusals and the results of :func:`surface_statement` (the same bits), and over
    the K labels and the two directions

    ``dist_sum`` float64 [K, 2]: ``statistics.tree_sum`` over terms [H, W] - ``np.sqrt(d2)`` at a border pixel of the direction's own side,
    ``+0.0`` elsewhere; ``+0.0`` for an empty border, ``+inf`` where only the other side's is empty (no term is negative: never a NaN).
    ``d2_rank`` float64 [K, 2, P, 2]: per percentile the ``d2`` at the sorted positions ``i`` and ``j`` of :func:`percentile_ranks` - exact
    bits, ties being repeated values; both ``-inf`` for an empty border.
    ``rank_weight`` float64 [K, 2, P]: its ``t``; ``+0.0`` for an empty border.

    The root is monotone, so the order statistics of the distances are the roots of those of ``d2``: :func:`percentile_of_ranks` makes the
    percentile of the two."""
    return _distance_walk('distance_profile_statement', a, kind_a, b, kind_b, values, spacing_hw, tolerances,
                          _percentiles(percentiles, 'distance_profile_statement'))


def volume_surface_statement(a, kind_a: int, b, kind_b: int, values, spacing_zhw, tolerances: Sequence[float]) -> dict:
    """THE DEFINITION of the boundary distances of volumes (module docstring): :func:`surface_statement` with one more axis.  ``a``, ``b``: planes
    ``[K, Z, H, W]`` or label maps ``[Z, H, W]``, and nothing else (``ValueError``); ``Z == 1`` is a volume of one slice, whose every foreground
    voxel is a border voxel.  ``spacing_zhw``: mm per array axis.  The same kinds, refusals and result keys: ``border``, ``d2_max``, ``within``."""
    return _distance_walk('volume_surface_statement', a, kind_a, b, kind_b, values, spacing_zhw, tolerances, None, volume=True)


def volume_distance_profile_statement(a, kind_a: int, b, kind_b: int, values, spacing_zhw, tolerances: Sequence[float],
                                      percentiles: Sequence[float]) -> dict:
    """THE DEFINITION of the distance profile of volumes: :func:`volume_surface_statement` (the same bits) and ``dist_sum``, ``d2_rank``,
    ``rank_weight`` as :func:`distance_profile_statement` has them, the terms of the sum meeting in ``statistics.tree_sum`` as ``[Z * H, W]``."""
    return _distance_walk('volume_distance_profile_statement', a, kind_a, b, kind_b, values, spacing_zhw, tolerances,
                          _percentiles(percentiles, 'volume_distance_profile_statement'), volume=True)


# ------------------------------------------------------------------------------------------------------------------ the device route
def device_serves(a: np.ndarray, kind_a: int, b: np.ndarray, kind_b: int, values, spatial, K: int) -> bool:
    """Do ``ts2d_label_overlap`` and ``ts2d_surface_distances`` serve the case?  uint8 samples, 1 ... 255 labels (label-map values 1 ... 255), at
    most 2^31 - 1 samples, and a library that has the symbols."""
    from . import engine
    if a.dtype != np.uint8 or b.dtype != np.uint8 or not 1 <= K <= 255:
        return False
    if min(spatial, default=0) < 1 or int(np.prod(spatial, dtype=np.int64)) > 2 ** 31 - 1:
        return False
    if LABELMAP in (kind_a, kind_b) and not all(1 <= int(v) <= 255 for v in values):
        return False
    return engine.has_entry('ts2d_label_overlap', 'ts2d_surface_distances')


def _device_overlap(a, kind_a, b, kind_b, values, spatial, device: int) -> dict:
    from . import engine
    zhw = (1,) * (3 - len(spatial)) + tuple(int(v) for v in spatial)
    o = engine.label_overlap(np.ascontiguousarray(a), kind_a, np.ascontiguousarray(b), kind_b, values, zhw, device)
    return {'n_a': o[:, 0].copy(), 'n_b': o[:, 1].copy(), 'n_both': o[:, 2].copy()}


def device_profiles() -> bool:
    """Does the library have ``ts2d_surface_distance_profile``?  (It serves what :func:`device_serves` serves.)"""
    from . import engine
    return engine.has_entry('ts2d_surface_distance_profile')


def _device_distances(a, kind_a, b, kind_b, values, hw, spacing_hw, tolerances, percentiles, want_sum: bool, device: int,
                      max_scratch_bytes: int = 0) -> dict:
    """The statements on the device, as :func:`_distance_walk` has them: ``percentiles`` None - :func:`surface_statement` by
    ``ts2d_surface_distances``; a list - :func:`distance_profile_statement` by ``ts2d_surface_distance_profile``, ``dist_sum`` only with
    ``want_sum``."""
    from . import engine
    tol = np.asarray(list(tolerances), np.float64)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if percentiles is None:
        oi, of = engine.surface_distances(a, kind_a, b, kind_b, values, hw, spacing_hw, tol * tol, max_scratch_bytes, device)
        extras = {}
    else:
        oi, of, osum, orank, oweight = engine.surface_distance_profile(a, kind_a, b, kind_b, values, hw, spacing_hw, tol * tol, list(percentiles),
                                                                       want_sum, max_scratch_bytes, device)
        extras = dict({'d2_rank': orank, 'rank_weight': oweight}, **({'dist_sum': osum} if want_sum else {}))
    return dict({'border': oi[:, :, 0].copy(), 'd2_max': of, 'within': oi[:, :, 1:].copy()}, **extras)


def _device_surface(a, kind_a, b, kind_b, values, hw, spacing_hw, tolerances, device: int, max_scratch_bytes: int = 0) -> dict:
    return _device_distances(a, kind_a, b, kind_b, values, hw, spacing_hw, tolerances, None, False, device, max_scratch_bytes)


def _device_profile(a, kind_a, b, kind_b, values, hw, spacing_hw, tolerances, percentiles, want_sum: bool, device: int,
                    max_scratch_bytes: int = 0) -> dict:
    return _device_distances(a, kind_a, b, kind_b, values, hw, spacing_hw, tolerances, list(percentiles), want_sum, device, max_scratch_bytes)


VOLUME_SCRATCH_BYTES = 4 << 30       # the default bound of ts2d_volume_surface_distances: what ONE label's box may take at the most
# No size gate for the volume route either: 18 labels at 16 x 128 x 128 take 0.98 ms (plain) and 2.3 ms (95th percentile and sum) against 35 ... 40 ms
# for scipy's EDT inside the joint boxes and 1.7 ... 2.2 s for the statements; at 64 x 512 x 512, 7.8 and 12.4 ms against 2.27 s
# (scripts/gpu_evaluate_volume_case.py, profiles/r34_volume_distances_case.txt).


def device_serves_volume(a: np.ndarray, kind_a: int, b: np.ndarray, kind_b: int, values, spatial, K: int) -> bool:
    """Does ``ts2d_volume_surface_distances`` serve the case?  What :func:`device_serves` asks, three extents of at most
    ``_lib.EVAL_MAX_EXTENT`` each, a label filling the whole volume within the default scratch bound, and a library that has the symbol."""
    from . import _lib, engine
    if len(spatial) != 3 or max(spatial) > _lib.EVAL_MAX_EXTENT or not device_serves(a, kind_a, b, kind_b, values, spatial, K):
        return False
    if engine.volume_scratch_per_label(spatial, 1, True) > VOLUME_SCRATCH_BYTES:
        return False
    return engine.has_entry('ts2d_volume_surface_distances')


def _device_volume_distances(a, kind_a, b, kind_b, values, zhw, spacing_zhw, tolerances, percentiles, want_sum: bool, device: int,
                             max_scratch_bytes: int = 0) -> dict:
    """The volume statements on the device by ``ts2d_volume_surface_distances``: ``percentiles`` None - :func:`volume_surface_statement` (the
    plain form of the entry); a list - :func:`volume_distance_profile_statement`, ``dist_sum`` only with ``want_sum``."""
    from . import engine
    tol = np.asarray(list(tolerances), np.float64)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    plain = percentiles is None
    oi, of, osum, orank, oweight = engine.volume_surface_distances(a, kind_a, b, kind_b, values, zhw, spacing_zhw, tol * tol,
                                                                   [] if plain else list(percentiles), bool(want_sum) and not plain,
                                                                   max_scratch_bytes, device)
    extras = {} if plain else dict({'d2_rank': orank, 'rank_weight': oweight}, **({'dist_sum': osum} if want_sum else {}))
    return dict({'border': oi[:, :, 0].copy(), 'd2_max': of, 'within': oi[:, :, 1:].copy()}, **extras)


# ------------------------------------------------------------------------------------------------------------------ evaluate
def _plane_axes(img: Image):
    """The (array axes, (spacing_h, spacing_w)) of a 2-D input: a 2-D image as it is, a 3-D image with an axis of size 1 without that axis (the
    coronal one first: what ``TS2D`` leaves behind); None for a volume."""
    nd = img.dimension
    shape = img.array.shape[:nd]
    if nd == 2:
        keep = [0, 1]
    elif nd == 3 and 1 in shape:
        drop = 1 if shape[1] == 1 else list(shape).index(1)
        keep = [k for k in range(3) if k != drop]
    else:
        return None
    return keep, tuple(float(img.spacing[nd - 1 - k]) for k in keep)


def _side(seg: Image, vals, who: str):
    """(array, kind) of one side for the labels ``vals``: the planes ``vals[k] - 1`` of a multi-component image, plane-major, or its label map."""
    if seg.components > 1:
        bad = [v for v in vals if not 1 <= v <= seg.components]
        if bad:
            raise ValueError(f"evaluate: labels {bad} name a component beyond the {who}'s {seg.components}")
        planes = np.moveaxis(seg.array, -1, 0)
        idx = [v - 1 for v in vals]
        planes = planes[idx[0]:idx[0] + len(idx)] if idx == list(range(idx[0], idx[0] + len(idx))) else planes[idx]
        return (planes if planes.flags['C_CONTIGUOUS'] else np.ascontiguousarray(planes)), PLANES
    return np.ascontiguousarray(seg.array), LABELMAP


def _ratio(n, d):
    return None if d == 0 else float(np.float64(n) / np.float64(d))


def tolerance_key(t) -> str:
    """The key of a tolerance in ``surface_dice``: ``repr`` of the float, so a dumped evaluation reads back to the dict."""
    return repr(float(t))


def percentile_key(q) -> str:
    """The key of a percentile in ``hausdorff_percentile``: ``repr`` of the float, as :func:`tolerance_key`."""
    return repr(float(q))


def evaluate(pred: Image, ref: Image, device: Optional[int] = None, tolerances: Sequence[float] = (2.0,), percentiles: Sequence[float] = (),
             average_distance: bool = False, volume_distances: bool = False) -> Dict[str, dict]:
    """name -> scores of ``pred`` against ``ref`` for every named label of ``pred`` (``image.get_annotation_labels(pred)``).

    ``pred``, ``ref``: each a multi-component segmentation (label ``v`` is component ``v - 1`` > 0) or a label map (label ``v`` is ``seg == v``),
    of one spatial shape (else ``ValueError`` with both extents).

    Per label: ``value``, ``count_pred``, ``count_ref``, ``count_both``, ``dice = 2 both / (pred + ref)``, ``iou = both / (pred + ref - both)``,
    ``precision = both / pred``, ``recall = both / ref`` (float64 quotients of integers), ``mm_pred`` / ``mm_ref`` = count * prod(spacing), and
    for 2-D inputs (:func:`_plane_axes`) ``surface_dice[tolerance_key(t)] = (within_ab + within_ba) / (border_a + border_b)`` and
    ``hausdorff = sqrt(max(d2_max_ab, d2_max_ba))`` in mm.  A ratio with a zero denominator is None; a mask that is empty on one side only gives
    ``hausdorff = inf``; empty on both, None.  For a volume ``surface_dice`` and ``hausdorff`` are absent - unless ``volume_distances=True``
    asks for them: a volume (three spatial axes, all above 1) then gains exactly the keys of the 2-D case, those on request included, with the
    same formulas and the same None / ``inf`` rules, from the 3-D border and distance of the module docstring
    (:func:`volume_surface_statement`, :func:`volume_distance_profile_statement`; the spacing of array axis ``k`` is ``spacing[2 - k]``).  On a
    2-D input the flag changes nothing.

    On request, for 2-D inputs too (absent for a volume, and absent without the request: the default call returns what it always did):
    ``percentiles`` (at most ``MAX_PERCENTILES``, each finite and in 0 ... 100, else ``ValueError``) adds
    ``hausdorff_percentile[percentile_key(q)]``, the robust Hausdorff distance as Metrics Reloaded and MONAI define HD95 for ``q = 95``: the
    larger of the two directed ``q``-th percentiles of the boundary distances (numpy's linear method, :func:`percentile_of_ranks`), taken over the
    directions that have a border; None where both borders are empty, ``inf`` where exactly one is.  ``average_distance=True`` adds
    ``asd_pred_to_ref`` and ``asd_ref_to_pred`` (the mean distance of a side's border pixels to the other border: the float64 sum of the
    distances in the fixed order of ``statistics.tree_sum`` over the border count), ``assd`` (both sums over both counts) and ``masd`` (the mean
    of the two directed averages; None if either is).  A zero denominator gives None, a border on one side only ``inf``.

    Route: ``ts2d_label_overlap`` and ``ts2d_surface_distances`` where ``device`` is given, the library has the symbols and the case is served
    (:func:`device_serves`), else the statements; with ``percentiles`` or ``average_distance`` the ONE call ``ts2d_surface_distance_profile``
    (:func:`device_profiles`) in the place of ``ts2d_surface_distances``, else :func:`distance_profile_statement`.  The numbers are the same bit
    for bit either way.  A volume's distances: ``ts2d_volume_surface_distances`` where ``device`` is given and :func:`device_serves_volume`
    holds, else the statements."""
    from .image import get_annotation_labels
    names = get_annotation_labels(pred)
    sp_pred, sp_ref = tuple(pred.array.shape[:pred.dimension]), tuple(ref.array.shape[:ref.dimension])
    if sp_pred != sp_ref:
        raise ValueError(f"evaluate: the segmentation has the extent {sp_pred}, the reference {sp_ref}")
    tolerances = [float(t) for t in tolerances]
    if len(tolerances) > MAX_TOLERANCES or any(not (t >= 0.0 and math.isfinite(t)) for t in tolerances):
        raise ValueError(f"evaluate: at most {MAX_TOLERANCES} tolerances, each finite and not negative, found {tolerances}")
    percentiles = _percentiles(percentiles, 'evaluate')
    profile = bool(percentiles) or bool(average_distance)
    out: Dict[str, dict] = {}
    if not names:
        return out
    vals = [int(i['value']) for i in names.values()]
    a, kind_a = _side(pred, vals, 'segmentation')
    b, kind_b = _side(ref, vals, 'reference')
    K = len(vals)
    flat = _plane_axes(pred)
    hw = tuple(sp_pred[k] for k in flat[0]) if flat else None
    on_device = device is not None and device_serves(a, kind_a, b, kind_b, vals, sp_pred, K)
    if on_device:
        ov = _device_overlap(a, kind_a, b, kind_b, vals, sp_pred, int(device))
    else:
        ov = overlap_statement(a, kind_a, b, kind_b, vals)
    sf = None
    if flat:
        a2 = a.reshape(((K,) if kind_a == PLANES else ()) + hw)
        b2 = b.reshape(((K,) if kind_b == PLANES else ()) + hw)
        qs = percentiles if profile else None                                            # the ONE decision "profile or not", for either route
        if on_device and (qs is None or device_profiles()):
            sf = _device_distances(a2, kind_a, b2, kind_b, vals, hw, flat[1], tolerances, qs, bool(average_distance), int(device))
        else:
            sf = _distance_walk('evaluate', a2, kind_a, b2, kind_b, vals, flat[1], tolerances, qs)
    elif volume_distances and pred.dimension == 3 and min(sp_pred) > 1:
        a3 = a.reshape(((K,) if kind_a == PLANES else ()) + sp_pred)
        b3 = b.reshape(((K,) if kind_b == PLANES else ()) + sp_pred)
        spacing_zhw = tuple(float(pred.spacing[2 - k]) for k in range(3))
        qs = percentiles if profile else None
        if device is not None and device_serves_volume(a, kind_a, b, kind_b, vals, sp_pred, K):
            sf = _device_volume_distances(a3, kind_a, b3, kind_b, vals, sp_pred, spacing_zhw, tolerances, qs, bool(average_distance), int(device))
        else:
            sf = _distance_walk('evaluate', a3, kind_a, b3, kind_b, vals, spacing_zhw, tolerances, qs, volume=True)
    mm = np.float64(np.prod(np.asarray(pred.spacing, dtype=np.float64)))
    mm_ref = np.float64(np.prod(np.asarray(ref.spacing, dtype=np.float64)))
    for k, (name, info) in enumerate(names.items()):
        na, nb, both = int(ov['n_a'][k]), int(ov['n_b'][k]), int(ov['n_both'][k])
        e = {'value': int(info['value']), 'count_pred': na, 'count_ref': nb, 'count_both': both, 'dice': _ratio(2 * both, na + nb),
             'iou': _ratio(both, na + nb - both), 'precision': _ratio(both, na), 'recall': _ratio(both, nb),
             'mm_pred': float(np.float64(na) * mm), 'mm_ref': float(np.float64(nb) * mm_ref)}
        if sf is not None:
            ba, bb = int(sf['border'][k, 0]), int(sf['border'][k, 1])
            e['surface_dice'] = {tolerance_key(t): _ratio(int(sf['within'][k, 0, i]) + int(sf['within'][k, 1, i]), ba + bb)
                                 for i, t in enumerate(tolerances)}
            top = max(float(sf['d2_max'][k, 0]), float(sf['d2_max'][k, 1]))
            e['hausdorff'] = None if ba + bb == 0 else float(np.sqrt(np.float64(top)))
            if percentiles:
                e['hausdorff_percentile'] = {}
                for p, q in enumerate(percentiles):
                    directed = [percentile_of_ranks(sf['d2_rank'][k, d, p, 0], sf['d2_rank'][k, d, p, 1], sf['rank_weight'][k, d, p])
                                for d, n in enumerate((ba, bb)) if n > 0]
                    e['hausdorff_percentile'][percentile_key(q)] = float(max(directed)) if directed else None
            if average_distance:
                s0, s1 = np.float64(sf['dist_sum'][k, 0]), np.float64(sf['dist_sum'][k, 1])
                e['asd_pred_to_ref'], e['asd_ref_to_pred'], e['assd'] = _ratio(s0, ba), _ratio(s1, bb), _ratio(s0 + s1, ba + bb)
                e['masd'] = None if ba == 0 or bb == 0 else float((np.float64(e['asd_pred_to_ref']) + np.float64(e['asd_ref_to_pred'])) / np.float64(2))
        out[name] = e
    return out


# No size gate for the confusion matrix: the device lost at no measured size - 117 labels at 53 x 133 take 0.6 ms against 12.5 ms for the statement
# and 34 ms for an int64 matrix product in numpy; the narrowest win is 18 labels at 600 x 512, 0.62 ms against 7.1 ms; a label-map stack
# 64 x 512 x 512 takes 1.1 ms against 84 ms for np.bincount and 0.63 s for the statement (scripts/gpu_confusion_case.py,
# profiles/r37_confusion_case.txt).


def device_confuses(a: np.ndarray, kind_a: int, b: np.ndarray, kind_b: int, values, spatial, K: int) -> bool:
    """Does ``ts2d_label_confusion`` serve the case?  Everything :func:`device_serves` asks, and a library that has the symbol."""
    from . import engine
    return device_serves(a, kind_a, b, kind_b, values, spatial, K) and engine.has_entry('ts2d_label_confusion')


def _device_confusion(a, kind_a, b, kind_b, values, spatial, device: int) -> np.ndarray:
    from . import engine
    zhw = (1,) * (3 - len(spatial)) + tuple(int(v) for v in spatial)
    same = a is b
    a = np.ascontiguousarray(a)
    return engine.label_confusion(a, kind_a, a if same else np.ascontiguousarray(b), kind_b, values, zhw, device)


def confusion(pred: Image, ref: Image, device: Optional[int] = None, top: int = 3) -> dict:
    """The confusion matrix of ``pred`` against ``ref`` over the named labels of ``pred`` (``image.get_annotation_labels(pred)``, in that order):
    what every structure of the reference was taken for.  The sides are prepared as :func:`evaluate` prepares them (multi-component planes or a
    label map each, mixed at will) and an extent mismatch raises the same ``ValueError``.  A volume and a 2-D plane are the same case: only the
    number of samples matters.

    Returns a dict (:func:`dump_evaluation` writes it as it is): ``classes`` = ``['background', name_1 ... name_K]``, ``values`` =
    ``[0, v_1 ... v_K]``, ``samples`` = N, and ``matrix``, K + 1 lists of K + 1 ints with ROWS THE REFERENCE AND COLUMNS THE PREDICTION
    (``'rows': 'reference', 'columns': 'prediction'``): ``matrix[r][p]`` counts the samples of reference class ``r`` and predicted class ``p``,
    class 0 being "none of the K labels" (the transpose of the inner block of ``confusion_statement(pred, ..., ref, ...)``).  ``count_ref``,
    ``count_pred``: the margins, K + 1 ints each, index 0 the background.  ``exclusive``: both sides are label maps, so every sample is in exactly
    one class on either side; only then ``accuracy = trace / N`` and Cohen's ``kappa = (po - pe) / (1 - pe)`` with ``po = trace / N`` and
    ``pe = sum(count_ref[i] * count_pred[i]) / N²`` are given (else None) - the integers exact, each ONE float64 division
    (``kappa = (trace * N - S) / (N * N - S)`` with ``S`` that sum; None where ``1 - pe == 0``).  With a planes side a sample may carry several
    labels and the matrix is a co-occurrence matrix whose entries may sum to more than N.

    ``labels[name]``: ``value``; ``predicted_as`` - where the reference's samples of the label went: the classes ``p != r`` with
    ``matrix[r][p] > 0`` by count descending, then class index, at most ``top`` of them, each ``{'class', 'value', 'count', 'fraction'}`` with
    ``fraction = count / count_ref[r]``; ``predicted_from`` - what lies under the prediction of the label: the same over column ``p``, with
    ``fraction = count / count_pred[p]``.

    ``confusion(seg, seg)`` is the label co-occurrence INSIDE one multilabel result - which structures overlap in the projection: a symmetric
    matrix with the labels' counts on its diagonal.

    Route: ``ts2d_label_confusion`` where ``device`` is given and :func:`device_confuses` holds, else :func:`confusion_statement`; the integers
    are the same either way."""
    from .image import get_annotation_labels
    top = int(top)
    if top < 0:
        raise ValueError(f"confusion: top = {top} is negative")
    names = get_annotation_labels(pred)
    sp_pred, sp_ref = tuple(pred.array.shape[:pred.dimension]), tuple(ref.array.shape[:ref.dimension])
    if sp_pred != sp_ref:
        raise ValueError(f"evaluate: the segmentation has the extent {sp_pred}, the reference {sp_ref}")
    vals = [int(i['value']) for i in names.values()]
    K = len(vals)
    N = int(np.prod(sp_pred, dtype=np.int64))
    exclusive = pred.components == 1 and ref.components == 1
    if K == 0:
        M = np.full((2, 2), N, np.int64)
    else:
        a, kind_a = _side(pred, vals, 'segmentation')
        b, kind_b = (a, kind_a) if ref is pred else _side(ref, vals, 'reference')
        if device is not None and device_confuses(a, kind_a, b, kind_b, vals, sp_pred, K):
            M = _device_confusion(a, kind_a, b, kind_b, vals, sp_pred, int(device))
        else:
            M = confusion_statement(a.reshape(((K,) if kind_a == PLANES else ()) + sp_pred), kind_a,
                                    b.reshape(((K,) if kind_b == PLANES else ()) + sp_pred), kind_b, vals)
    classes, values = ['background'] + list(names), [0] + vals
    matrix = [[int(M[p, r]) for p in range(K + 1)] for r in range(K + 1)]
    count_ref, count_pred = [int(M[K + 1, i]) for i in range(K + 1)], [int(M[i, K + 1]) for i in range(K + 1)]
    out = {'classes': classes, 'values': values, 'samples': N, 'rows': 'reference', 'columns': 'prediction', 'matrix': matrix,
           'count_ref': count_ref, 'count_pred': count_pred, 'exclusive': bool(exclusive), 'accuracy': None, 'kappa': None, 'labels': {}}
    if exclusive:
        trace = sum(matrix[i][i] for i in range(K + 1))
        agree = sum(count_ref[i] * count_pred[i] for i in range(K + 1))
        out['accuracy'], out['kappa'] = _ratio(trace, N), _ratio(trace * N - agree, N * N - agree)

    def others(own: int, counts, total: int):
        order = sorted((c for c in range(K + 1) if c != own and counts[c] > 0), key=lambda c: (-counts[c], c))
        return [{'class': classes[c], 'value': values[c], 'count': counts[c], 'fraction': _ratio(counts[c], total)} for c in order[:top]]
    for k, name in enumerate(names):
        c = 1 + k
        out['labels'][name] = {'value': values[c], 'predicted_as': others(c, matrix[c], count_ref[c]),
                               'predicted_from': others(c, [matrix[r][c] for r in range(K + 1)], count_pred[c])}
    return out


def dump_evaluation(result: dict, path: str) -> str:
    """``json.dump`` with sorted keys; Python floats, so the file reads back to the dict (None is ``null``, an infinite distance ``Infinity``)."""
    with open(path, 'w') as f:
        json.dump(result, f, sort_keys=True, indent=1)
        f.write('\n')
    return path
