"""Grow, shrink, open and close every label of a 2-D segmentation by a margin in mm, with an exact Euclidean disc: a safety margin around an
organ, a rim peeled off before intensities are measured, pin-holes closed and thin bridges opened before ``--keep-largest``.  It serves
multilabel planes (the merged result of ``TS2D.predict``) and label maps alike.

:func:`label_morphology_statement` is the project's definition, the host route and the oracle of the device route (C-ABI
``ts2d_label_morphology``, ``csrc/kernels_morph.h``), which reproduces it byte for byte, counters included.

THE DISC.  A mask ``M[H][W]`` has pixel spacings ``(sy, sx)``; a radius ``r >= 0`` is in their unit.  ``r2 = float64(r) * float64(r)``, one
rounding.  Offset ``(dy, dx)`` belongs to the disc ``B`` iff :func:`sd_candidate` ``(|dy|, |dx|, sy, sx) <= r2`` - ``(|dy| * sy)**2 +
(|dx| * sx)**2`` in float64 with the roundings of ``csrc/surface_dist.h``: both products of a term and the sum each rounded on their own.  The
comparison is ``<=``: a pixel exactly on the circle belongs.

- dilate: ``D(M)`` = the pixels ``p`` inside the image with some ``q`` in ``M`` and ``p - q`` in ``B``.
- erode: the dual INSIDE the image, ``E(M) = ~D(~M)``.  Pixels outside the image are ignored: they count neither as background nor as
  foreground, so a mask that touches the image edge is not eaten from that edge.  That is ``skimage.morphology.binary_erosion`` and
  ``scipy.ndimage.binary_erosion(border_value=1)``; scipy's DEFAULT (``border_value=0``) erodes from the edge and is not this.
- open = ``D(E(M))``, close = ``E(D(M))``.  With this convention open is anti-extensive, close is extensive and both are idempotent, on the
  bounded image too.
- ``r = 0`` returns the input bytes.

THE SCAN FORM is what the statement and the device compute (``csrc/morph.h`` has the argument; ``tests/test_morphology_cpu.py`` holds it
against the disc form through scipy).  :func:`cover_table` turns the float64 comparison into integers: ``cover[n]`` is the largest column offset
the disc admits at row offset ``n``.  ``g(y, x')`` is the row distance to the nearest pixel of ``M`` in column ``x'``; column ``x'`` covers the
interval ``[x' - cover[g], x' + cover[g]]`` of row ``y`` (nothing where ``g`` is beyond the table), and the union of the intervals is one prefix
maximum and one suffix minimum along the row: O(H W) per label whatever the radius.

LABELS.  Planes ``[K, H, W]``: label ``k`` is ``seg[k] > 0`` and is processed on its own; a pixel that stays set keeps its byte, a cleared pixel
becomes 0, a newly set one 1.  Label map ``[H, W]`` with ``values``: label ``k`` is ``seg == values[k]``; each selected label's result ``R_k`` is
computed on its own mask (everything that is not ``values[k]`` counts as outside the mask).  Shrinking operations (erode, open): a pixel of label
``k`` not in ``R_k`` becomes 0.  Growing operations (dilate, close): only samples equal to 0 are painted, in the order of ``values``, so the first
label wins; a non-zero sample is never overwritten, whether its value is named or not.  Growth towards the NEAREST label
(``skimage.segmentation.expand_labels``) is out of scope.  ``select``: None, or K booleans; an unselected label is returned untouched, and in a
label map it stays an obstacle.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .nrrd import Image

OPS = ('dilate', 'erode', 'open', 'close')                  # TS2D_MORPH_DILATE, _ERODE, _OPEN, _CLOSE
COUNTER_NAMES = ('pixels', 'pixels_after', 'added', 'removed')
MAX_EXTENT = 32767                                          # TS2D_EVAL_MAX_EXTENT: g and the table are uint16 on the device
# No size gate: the device route lost to the statement at no measured size (scripts/gpu_morphology_case.py, profiles/r39_morphology_case.txt).


def _op(op, who: str) -> int:
    if op not in OPS:
        raise ValueError(f"{who}: op {op!r} is none of {', '.join(OPS)}")
    return OPS.index(op)


def _radius_spacing(radius, spacing_hw, who: str):
    r = np.float64(radius)
    if not (math.isfinite(r) and r >= 0):
        raise ValueError(f"{who}: radius {radius!r} must be finite and not negative")
    sy, sx = (np.float64(v) for v in spacing_hw)
    if not (math.isfinite(sy) and math.isfinite(sx) and sy > 0 and sx > 0):
        raise ValueError(f"{who}: spacing {tuple(spacing_hw)!r} must be finite and positive")
    return r, sy, sx


def _r2(r) -> np.float64:
    """``r * r`` in float64, one rounding; +inf for a radius whose square is beyond float64: then every offset belongs."""
    with np.errstate(over='ignore'):
        return np.float64(r) * np.float64(r)


def sd_candidate(dy, dx, sy, sx):
    """``(dy * sy) * (dy * sy) + (dx * sx) * (dx * sx)`` in float64, every operation rounded on its own (``sd_candidate`` of
    ``csrc/surface_dist.h``); ``dy``, ``dx``: non-negative integers or arrays of them."""
    ry = np.asarray(dy, dtype=np.float64) * np.float64(sy)
    rx = np.asarray(dx, dtype=np.float64) * np.float64(sx)
    return ry * ry + rx * rx


def disc(radius: float, sy: float, sx: float, H: int, W: int) -> np.ndarray:
    """The disc ``B`` as a boolean structuring element ``[2 H - 1, 2 W - 1]`` centred on ``(H - 1, W - 1)``: every offset that two pixels of an
    ``H x W`` image can have.  What a user hands to ``scipy.ndimage.binary_dilation``."""
    r, sy, sx = _radius_spacing(radius, (sy, sx), 'disc')
    dy = np.abs(np.arange(-(H - 1), H))[:, None]
    dx = np.abs(np.arange(-(W - 1), W))[None, :]
    return sd_candidate(dy, dx, sy, sx) <= _r2(r)


def cover_table(radius: float, sy: float, sx: float, H: int, W: int) -> np.ndarray:
    """``cover[n]`` for ``n = 0, 1, ...``: the largest ``dx`` in ``[0, W - 1]`` with ``sd_candidate(n, dx) <= r2``.  The table ends before the
    first ``n`` that admits no ``dx``, or at ``H``; it has at least the entry of ``n = 0``.  ``sd_candidate`` is monotone in both integers, bits
    included, so the table carries everything the float64 comparison decides."""
    r, sy, sx = _radius_spacing(radius, (sy, sx), 'cover_table')
    inside = sd_candidate(np.arange(H)[:, None], np.arange(W)[None, :], sy, sx) <= _r2(r)
    count = inside.sum(axis=1)                  # monotone in dx: the admitted offsets of a row are 0 ... count - 1
    T = int(np.argmax(count == 0)) if (count == 0).any() else H
    return (count[:T] - 1).astype(np.int64)


def _dilate(mask: np.ndarray, cover: np.ndarray) -> np.ndarray:
    """The scan form of ``D(mask)`` for a boolean ``[..., H, W]``."""
    H, W = mask.shape[-2:]
    T = len(cover)
    g = np.full(mask.shape, T, np.int64)
    last = np.full(mask.shape[:-2] + (W,), -1, np.int64)
    for y in range(H):                          # the nearest member at or above
        last = np.where(mask[..., y, :], y, last)
        g[..., y, :] = np.where(last < 0, T, np.minimum(y - last, T))
    last = np.full(mask.shape[:-2] + (W,), -1, np.int64)
    for y in range(H - 1, -1, -1):              # ... at or below
        last = np.where(mask[..., y, :], y, last)
        g[..., y, :] = np.minimum(g[..., y, :], np.where(last < 0, T, np.minimum(last - y, T)))
    has = g < T
    c = np.concatenate([cover, [0]])[g]
    x = np.arange(W, dtype=np.int64)
    right = np.maximum.accumulate(np.where(has, x + c, -1), axis=-1)
    left = np.minimum.accumulate(np.where(has, x - c, np.iinfo(np.int64).max)[..., ::-1], axis=-1)[..., ::-1]
    return (right >= x) | (left <= x)


def _apply(mask: np.ndarray, op: int, cover: np.ndarray) -> np.ndarray:
    def erode(m):
        return ~_dilate(~m, cover)
    if op == 0:
        return _dilate(mask, cover)
    if op == 1:
        return erode(mask)
    if op == 2:
        return _dilate(erode(mask), cover)
    return erode(_dilate(mask, cover))


def binary_morphology(mask: np.ndarray, op: str, radius: float, spacing_hw=(1.0, 1.0)) -> np.ndarray:
    """``op`` of one boolean mask ``[H, W]`` (or a stack ``[..., H, W]``, every plane on its own): the module docstring's definition."""
    code = _op(op, 'binary_morphology')
    mask = np.asarray(mask) > 0
    if mask.ndim < 2:
        raise ValueError(f"binary_morphology: a mask has two axes, found shape {mask.shape}")
    r, sy, sx = _radius_spacing(radius, spacing_hw, 'binary_morphology')
    return _apply(mask, code, cover_table(r, sy, sx, *mask.shape[-2:]))


def label_morphology_statement(seg: np.ndarray, values: Optional[Sequence[int]], op: str, radius: float, spacing_hw, select=None
                               ) -> Tuple[np.ndarray, np.ndarray]:
    """THE DEFINITION.  ``seg``, ``values``: with ``values=None`` planes ``[K, H, W]``, label ``k`` is ``seg[k] > 0``; with ``values`` a label
    map ``[H, W]``, label ``k`` is ``seg == values[k]``.  ``spacing_hw``: the spacings of the two axes; ``radius`` in their unit.  ``select``:
    None or K booleans.  The rules: the module docstring.

    Returns ``(out, counters)``: ``out`` of the shape and dtype of ``seg``; ``counters`` int64 [K, 4] = pixels before, pixels after, added,
    removed - of a label map counted after painting.  A volume (more than two spatial axes above 1) is refused by name."""
    who = 'label_morphology_statement'
    code = _op(op, who)
    seg = np.asarray(seg)
    r, sy, sx = _radius_spacing(radius, spacing_hw, who)
    planes = values is None
    spatial = seg.shape[1:] if planes else seg.shape
    if len(spatial) > 2 and sum(int(e) > 1 for e in spatial) > 2:
        raise ValueError(f"{who}: extents {tuple(int(e) for e in spatial)} are a volume; the morphology is 2-D (at most two axes above 1)")
    if len(spatial) != 2:
        raise ValueError(f"{who}: {len(spatial)} spatial axes; hand the two axes of the plane and their spacings")
    if min(spatial) < 1:
        raise ValueError(f"{who}: extents {tuple(int(e) for e in spatial)} hold no pixel")
    K = seg.shape[0] if planes else len(values)
    if select is None:
        select = [True] * K
    select = [bool(s) for s in select]
    if len(select) != K:
        raise ValueError(f"{who}: select has {len(select)} entries for {K} labels")
    if not planes and (len({int(v) for v in values}) != K or any(int(v) == 0 for v in values)):
        raise ValueError(f"{who}: the values of a label map are distinct and not 0, found {list(values)!r}")
    H, W = spatial
    cover = cover_table(r, sy, sx, H, W)
    out = np.array(seg, order='C')
    counters = np.zeros((K, len(COUNTER_NAMES)), np.int64)
    grows = code in (0, 3)
    for k in range(K):
        if not select[k]:
            continue
        mask = (seg[k] > 0) if planes else (seg == values[k])
        res = _apply(mask, code, cover)
        if planes:
            out[k] = np.where(res, np.where(mask, seg[k], 1), 0).astype(seg.dtype)
        elif grows:
            out[res & (out == 0)] = values[k]
        else:
            out[mask & ~res] = 0
    for k in range(K):
        before = (seg[k] > 0) if planes else (seg == values[k])
        after = (out[k] > 0) if planes else (out == values[k])
        counters[k] = (np.count_nonzero(before), np.count_nonzero(after), np.count_nonzero(after & ~before), np.count_nonzero(before & ~after))
    return out, counters


def device_serves(planes: np.ndarray, values, spatial) -> bool:
    """Does ``ts2d_label_morphology`` serve the case?  The gates of ``components.device_serves`` - uint8 samples, 1 ... 255 labels with distinct
    values 1 ... 255, at most 2^31 - 1 pixels, a library that has the symbol -, two spatial axes, and every extent at most 32767."""
    K = planes.shape[0] if values is None else len(values)
    if planes.dtype != np.uint8 or len(spatial) != 2 or not 1 <= K <= 255:
        return False
    if min(spatial) < 1 or max(spatial) > MAX_EXTENT or int(np.prod(spatial, dtype=np.int64)) > 2 ** 31 - 1:
        return False
    if values is not None and (not all(1 <= int(v) <= 255 for v in values) or len({int(v) for v in values}) != K):
        return False
    from . import engine
    return engine.has_entry('ts2d_label_morphology')


def _morphology(planes: np.ndarray, values, op: str, radius: float, spacing_hw, select, device: Optional[int]):
    """``(out, counters)`` from the device where it serves the case, else from the statement: the same bytes."""
    spatial = planes.shape[1:] if values is None else planes.shape
    if device is not None and device_serves(planes, values, spatial):
        from . import _lib, engine
        return engine.label_morphology(planes, _lib.STATS_PLANES if values is None else _lib.STATS_LABELMAP, values, spatial, spacing_hw,
                                       OPS.index(op), radius, select=select, device=int(device))
    return label_morphology_statement(planes, values, op, radius, spacing_hw, select)


def label_morphology(seg: Image, op: str, radius_mm: float, device: Optional[int] = None, labels='all') -> Tuple[Image, Dict[str, dict]]:
    """``seg`` with ``op`` ('dilate', 'erode', 'open', 'close') applied to its labels by ``radius_mm``: ``(image, counters)`` - a NEW image with
    the geometry and metadata of ``seg`` (``seg`` itself is untouched) and per name ``pixels``, ``pixels_after``, ``added`` and ``removed``.
    ``labels``: 'all', or a subset of the names of ``image.get_annotation_labels(seg)``; the others stay untouched (obstacles of a label map).
    Every named plane of a multi-component segmentation is worked on its own, and every named value of a label map (the rules: the module
    docstring).  A 3-D image with one unit axis - what ``TS2D.predict`` returns - is the 2-D case of its other two axes AND THEIR spacings; a
    volume is refused by name.  Route: ``ts2d_label_morphology`` where ``device`` is given and :func:`device_serves`, else
    :func:`label_morphology_statement`; the bytes are the same."""
    from .components import _label_side
    from .evaluate import _plane_axes
    who = 'label_morphology'
    _op(op, who)
    names, planes, values, index, spatial = _label_side(seg, who)
    flat = _plane_axes(seg)
    if flat is None:
        raise ValueError(f"{who}: extents {tuple(int(s) for s in spatial)} are a volume; the morphology is 2-D (a 3-D image needs an axis of size 1)")
    keep, spacing_hw = flat
    hw = tuple(int(spatial[a]) for a in keep)
    K = planes.shape[0] if values is None else len(values)
    if isinstance(labels, str) and labels == 'all':
        chosen = set(names)
    else:
        chosen = {str(n) for n in ([labels] if isinstance(labels, str) else labels)}
        unknown = sorted(chosen - set(names))
        if unknown:
            raise ValueError(f"{who}: labels {unknown} are not among the segmentation's {sorted(names)}")
    meta = dict(seg.meta) if seg.meta is not None else None
    if K == 0 or not names:
        return Image(np.array(seg.array), seg.spacing, seg.origin, seg.direction, seg.components, meta, seg.space), {}
    select = [False] * K
    for name in chosen:
        select[index[name]] = True
    flat_planes = planes.reshape(((K,) if values is None else ()) + hw)        # dropping a unit axis keeps the order of the samples
    out, counters = _morphology(flat_planes, values, op, radius_mm, spacing_hw, select, device)
    out = out.reshape(planes.shape)
    array = np.moveaxis(out, 0, -1) if values is None else out                  # (plane-major behind the interleaved view, as export.py builds it)
    image = Image(array, seg.spacing, seg.origin, seg.direction, seg.components, meta, seg.space)
    return image, {name: {c: int(v) for c, v in zip(COUNTER_NAMES, counters[index[name]])} for name in names}
