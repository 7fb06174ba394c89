"""Connected components of every label of a segmentation: is a label ONE piece, how large are its pieces, and a clean-up rule - keep the
largest piece of every label, drop every piece below a size - what TotalSegmentator users know as "keep the largest blob" and
``--remove_small_blobs``.  It serves multilabel planes (the merged result of ``TS2D.predict``) and label maps alike; the plan route of a label-map
or region model (``postprocess.py``, one union of labels per step) stays what it is.

:func:`label_components_statement` is the project's definition - ``scipy.ndimage.label`` per label, ``np.bincount``, the first voxel of every piece -, the host
route and the oracle of the device route (C-ABI ``ts2d_label_components``, ``csrc/kernels_components.h``), which labels ALL labels in the same
six or seven launches and reproduces it byte for byte, as ``statistics.label_statistics_statement`` is for its entry.

THE RULE.  The components of label ``k`` are those of its mask on its own, under ``'full'`` (8 / 26 neighbours: what the postprocessing plans
use) or ``'faces'`` (4 / 6: scipy's default, hence TotalSegmentator's blob removal) connectivity; two labels that touch in a label map never
join, nor do plane ``k`` and plane ``k + 1``.  Component ``c`` of label ``k``, of size ``s``, is REMOVED iff
``(keep_largest and s < largest_k) or s < min_voxels[k]``: components that tie for the largest all stay, ``s == min_voxels[k]`` stays.  Removed
voxels become 0 - the background of a label map, that plane's voxel of planes.

SIZES IN MM.  ``min_size_mm`` is an area or a volume in the unit of ``mm`` of the statistics, ``count * prod(spacing)``; the integer threshold
is :func:`min_voxels_of`: the smallest ``n`` with ``float64(n) * voxel_mm >= min_size_mm``.  Both routes are handed that integer.
"""
from __future__ import annotations

import json
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .nrrd import Image

CONNECTIVITIES = ('full', 'faces')
COUNTER_NAMES = ('voxels', 'components', 'largest', 'voxels_removed', 'components_removed')
# No size gate: the device route lost to the statement at no measured size (scripts/gpu_components_case.py, profiles/r36_components_case.txt).


def _connectivity(connectivity, who: str) -> int:
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"{who}: connectivity {connectivity!r} is neither 'full' nor 'faces'")
    return CONNECTIVITIES.index(connectivity)


def min_voxels_of(min_size_mm: float, voxel_mm: float) -> int:
    """The smallest integer ``n >= 0`` with ``float64(n) * voxel_mm >= min_size_mm`` (one float64 product, as ``mm`` of the statistics is
    formed): a component of ``n`` voxels is the smallest that stays.  ``min_size_mm`` must be finite and not negative, ``voxel_mm`` finite and
    positive."""
    size, mm = np.float64(min_size_mm), np.float64(voxel_mm)
    if not (math.isfinite(size) and size >= 0):
        raise ValueError(f"min_size_mm = {min_size_mm!r} must be finite and not negative")
    if not (math.isfinite(mm) and mm > 0):
        raise ValueError(f"the size of a voxel, {voxel_mm!r}, must be finite and positive")
    if size == 0:
        return 0
    n = int(math.ceil(float(size / mm)))          # within a few of the answer: the quotient is rounded once
    while n > 0 and np.float64(n - 1) * mm >= size:
        n -= 1
    while np.float64(n) * mm < size:
        n += 1
    return n


def label_components_statement(seg: np.ndarray, values: Optional[Sequence[int]] = None, connectivity: str = 'full', keep_largest: bool = False,
                               min_voxels: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """THE DEFINITION.  ``seg``, ``values``: as in ``statistics.label_statistics_statement`` - with ``values=None`` planes ``[K, *spatial]``, label
    ``k`` is ``seg[k] > 0``; with ``values`` a label map ``[*spatial]``, label ``k`` is ``seg == values[k]`` -, two or three spatial axes (a 2-D
    case is Z = 1).  ``connectivity``: ``'full'`` (``generate_binary_structure(nd, nd)``) or ``'faces'`` (``generate_binary_structure(nd, 1)``).
    ``min_voxels``: None or K non-negative integers.  The rule: the module docstring.

    Returns ``(cleaned, counters, components)``: the cleaned array, of the shape and dtype of ``seg``; ``counters`` int64 [K, 5] = voxels,
    components, largest size, voxels removed, components removed; ``components`` int64 [N, 3] = ``(k, first, size)`` of every component of the
    INPUT, ``first`` the smallest linear index of the component inside ``[Z][H][W]``, sorted by ``(k, -size, first)``.  An absent label: zeros
    and no rows."""
    from scipy import ndimage
    faces = _connectivity(connectivity, 'label_components_statement')
    seg = np.asarray(seg)
    if values is None:
        spatial, K = seg.shape[1:], seg.shape[0]
    else:
        spatial, K = seg.shape, len(values)
    nd = len(spatial)
    if nd not in (2, 3):
        raise ValueError(f"label_components_statement: {nd} spatial axes; a segmentation has two or three")
    if min_voxels is not None:
        min_voxels = [int(v) for v in min_voxels]
        if len(min_voxels) != K or any(v < 0 for v in min_voxels):
            raise ValueError(f"label_components_statement: min_voxels must be {K} non-negative integers, found {min_voxels!r}")
    structure = ndimage.generate_binary_structure(nd, 1 if faces else nd)
    out = np.array(seg, order='C')
    counters = np.zeros((K, len(COUNTER_NAMES)), np.int64)
    rows = []
    for k in range(K):
        mask = (seg[k] > 0) if values is None else (seg == values[k])
        n_mask = int(np.count_nonzero(mask))
        if n_mask == 0:
            continue
        lab, n = ndimage.label(mask, structure=structure)
        flat = lab.reshape(-1)
        sizes = np.bincount(flat, minlength=n + 1).astype(np.int64)
        at = np.flatnonzero(flat)
        first = np.zeros(n + 1, np.int64)
        first[flat[at[::-1]]] = at[::-1]          # (of the values assigned to one entry the last stays: in reverse, the smallest index)
        sizes[0] = 0
        largest = int(sizes.max())
        drop = np.zeros(n + 1, bool)
        if keep_largest:
            drop |= sizes < largest
        if min_voxels is not None:
            drop |= sizes < min_voxels[k]
        drop[0] = False
        gone = drop[lab]
        (out[k] if values is None else out)[gone] = 0
        counters[k] = (n_mask, n, largest, int(sizes[drop].sum()), int(np.count_nonzero(drop)))
        rows.append(np.stack([np.full(n, k, np.int64), first[1:], sizes[1:]], axis=1))
    components = np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)
    components = components[np.lexsort((components[:, 1], -components[:, 2], components[:, 0]))]
    return out, counters, components


def device_serves(planes: np.ndarray, values, spatial) -> bool:
    """Does ``ts2d_label_components`` serve the case?  The gates of ``statistics.device_serves`` - uint8 samples, 2 or 3 spatial axes, at most
    2^31 - 1 voxels, 1 ... 255 labels with values 1 ... 255 -, distinct values, and a library that has the symbol."""
    K = planes.shape[0] if values is None else len(values)
    if planes.dtype != np.uint8 or len(spatial) not in (2, 3) or not 1 <= K <= 255:
        return False
    if min(spatial) < 1 or int(np.prod(spatial, dtype=np.int64)) > 2 ** 31 - 1:
        return False
    if values is not None and (not all(1 <= int(v) <= 255 for v in values) or len({int(v) for v in values}) != K):
        return False
    from . import engine
    return engine.has_entry('ts2d_label_components')


def _components(planes: np.ndarray, values, spatial, faces: int, keep_largest: bool, min_voxels, device: Optional[int], want_seg: bool,
                want_list: bool):
    """``(cleaned or None, counters, components or None)`` from the device where it serves the case and does not give up, else from the
    statement: the same bytes."""
    if device is not None and device_serves(planes, values, spatial):
        from . import _lib, engine
        zhw = (1,) * (3 - len(spatial)) + tuple(int(v) for v in spatial)
        got = engine.label_components(planes, _lib.STATS_PLANES if values is None else _lib.STATS_LABELMAP, values, zhw, faces, keep_largest,
                                      min_voxels, want_seg=want_seg, want_list=want_list, device=int(device))
        if got is not None:
            return got
    return label_components_statement(planes, values, CONNECTIVITIES[faces], keep_largest, min_voxels)


def _label_side(seg: Image, who: str):
    """``(names, planes, values, index, spatial)`` of a segmentation image, as ``statistics.label_statistics`` reads it: plane-major planes
    (without a copy where the image holds them so) or a label map with the values of its named labels."""
    from .image import get_annotation_labels
    names = get_annotation_labels(seg)
    spatial = tuple(seg.array.shape[:seg.dimension])
    if seg.components > 1:
        planes = np.moveaxis(seg.array, -1, 0)
        if not planes.flags['C_CONTIGUOUS']:
            planes = np.ascontiguousarray(planes)
        bad = [n for n, i in names.items() if not 1 <= int(i['value']) <= seg.components]
        if bad:
            raise ValueError(f"{who}: labels {bad} name a component beyond the segmentation's {seg.components}")
        return names, planes, None, {n: int(i['value']) - 1 for n, i in names.items()}, spatial
    return names, np.ascontiguousarray(seg.array), [int(i['value']) for i in names.values()], {n: j for j, n in enumerate(names)}, spatial


def label_components(seg: Image, device: Optional[int] = None, connectivity: str = 'full') -> Dict[str, dict]:
    """name -> the components of every named label of ``seg`` (the names and values of ``image.get_annotation_labels``, as in
    ``statistics.label_statistics``): ``count`` and ``mm`` (= count * prod(spacing)) of the label, ``components`` (how many pieces),
    ``largest`` and ``largest_mm``, ``sizes`` and ``sizes_mm`` (every piece, largest first) and ``first_index`` (per piece the array index
    ``[z, y, x]`` or ``[y, x]`` of its first voxel in index order).  Route: ``ts2d_label_components`` where ``device`` is given and
    :func:`device_serves`, else :func:`label_components_statement`; the numbers are the same."""
    faces = _connectivity(connectivity, 'label_components')
    names, planes, values, index, spatial = _label_side(seg, 'label_components')
    if not names:
        return {}
    _, counters, rows = _components(planes, values, spatial, faces, False, None, device, False, True)
    mm = np.float64(np.prod(np.asarray(seg.spacing, dtype=np.float64)))
    out: Dict[str, dict] = {}
    for name in names:
        j = index[name]
        mine = rows[rows[:, 0] == j]
        at = np.stack(np.unravel_index(mine[:, 1], spatial), axis=1) if len(mine) else np.zeros((0, len(spatial)), np.int64)
        out[name] = {'count': int(counters[j, 0]), 'mm': float(np.float64(counters[j, 0]) * mm), 'components': int(counters[j, 1]),
                     'largest': int(counters[j, 2]), 'largest_mm': float(np.float64(counters[j, 2]) * mm),
                     'sizes': [int(v) for v in mine[:, 2]], 'sizes_mm': [float(np.float64(v) * mm) for v in mine[:, 2]],
                     'first_index': [[int(v) for v in row] for row in at]}
    return out


def clean_components(seg: Image, device: Optional[int] = None, connectivity: str = 'full', keep_largest: bool = False,
                     min_size_mm: float = 0.0) -> Tuple[Image, Dict[str, dict]]:
    """``seg`` with the rule of the module docstring applied to every label: ``(image, counters)`` - a NEW image with the geometry and metadata
    of ``seg`` (``seg`` itself is untouched) and per name ``voxels``, ``components``, ``largest``, ``voxels_removed`` and
    ``components_removed``.  ``min_size_mm``: pieces below this area or volume go (:func:`min_voxels_of` of it and ``prod(spacing)``).  Every
    plane of a multi-component segmentation is cleaned, and every NAMED value of a label map.  With the defaults nothing is removed.  Routes as
    in :func:`label_components`: the same bytes."""
    faces = _connectivity(connectivity, 'clean_components')
    names, planes, values, index, spatial = _label_side(seg, 'clean_components')
    K = planes.shape[0] if values is None else len(values)
    threshold = min(min_voxels_of(min_size_mm, float(np.prod(np.asarray(seg.spacing, dtype=np.float64)))), 2 ** 62)      # (no piece is that large)
    meta = dict(seg.meta) if seg.meta is not None else None
    if K == 0:
        return Image(np.array(seg.array), seg.spacing, seg.origin, seg.direction, seg.components, meta, seg.space), {}
    cleaned, counters, _ = _components(planes, values, spatial, faces, bool(keep_largest), [threshold] * K if threshold else None, device, True, False)
    array = np.moveaxis(cleaned, 0, -1) if values is None else cleaned          # (plane-major behind the interleaved view, as export.py builds it)
    image = Image(array, seg.spacing, seg.origin, seg.direction, seg.components, meta, seg.space)
    return image, {name: {c: int(v) for c, v in zip(COUNTER_NAMES, counters[index[name]])} for name in names}


def dump_components(components: dict, path: str) -> str:
    """``json.dump`` with sorted keys; Python ints and floats, so the file reads back to the dict."""
    with open(path, 'w') as f:
        json.dump(components, f, sort_keys=True, indent=1)
        f.write('\n')
    return path
