"""Per-label statistics of a segmentation: is a structure there, how large is it, where is it, and how bright is the image under it.

The reference has the primitives (``ts2d/core/util/meta.py:64-80``: ``get_labels_voxels``, ``get_voxel_mm``; ``:289-330``:
``get_annotation_labels(seg, fetch=True, counts=True)``); :func:`label_statistics_statement` is the project's definition of everything beyond
them - written in numpy, it is the host route and the oracle of the device route (C-ABI ``ts2d_label_statistics``, ``csrc/kernels_stats.h``),
which reproduces it bit for bit, as ``postprocess.keep_largest_components_statement`` and ``visual.py`` are for their entries.

Per label: ``count`` (int64), the inclusive bounding box and the int64 sums of the indices along every array axis (so a centroid is a function
of the input alone), and per float32 intensity channel ``min`` and ``max`` (on the order-preserving keys of ``csrc/ray_select.h``:
``-0.0 < +0.0``), the float64 ``sum``, ``mean = sum / count``, ``ssq = sum((x - mean)^2)`` and ``std = sqrt(ssq / count)`` - two passes,
difference, product and sum rounded on their own, IEEE divide and square root: the arithmetic the ``std`` projection mode pins.

SUMMATION ORDER.  A float sum must not depend on the order in which partial results arrive, so the statement fixes a tree
(``csrc/stats_tree.h`` spells the same in C++).  The volume is ``rows`` rows of ``W`` samples (every axis but the last flattened).  A term is
the sample's value where the sample belongs to the label and ``+0.0`` where it does not.

    level 1, per row    lane ``l`` of 64 adds the terms at ``x = l, l + 64, ...`` in increasing ``x``, starting from ``+0.0``; the 64 lane
                        values are halved: ``v[l] + v[l + 32]`` for ``l < 32``, then ``+ 16`` ... down to ``+ 1``
    level 2, per label  the row partials meet the same way: lane ``l`` adds the partials of rows ``l, l + 64, ...``, then the halving

The shape is a function of ``(rows, W)`` alone.  It vectorises in numpy (reshape to ``[..., 64]``, loop over the leading axis, halve) and maps
to one wave per (label, row) with cross-lane adds.  Adding ``+0.0`` for a sample outside the label equals skipping it: a partial sum that
starts at ``+0.0`` never becomes ``-0.0``.

A non-finite intensity under a label is a status at the device entry (it writes nothing); the statement computes what numpy computes (NaN or
inf), and :func:`label_statistics` hands such a case to it.

PERCENTILES.  On request (``percentiles``: at most 8, each in 0 ... 100) the median and any other percentile of every intensity channel under
every label - numpy's linear method.  :func:`label_percentiles_statement` is the definition: the samples of a channel under a label are ordered
by their keys (``-0.0`` right below ``+0.0``, equal values repeated), percentile ``q`` among ``n`` samples selects the sorted positions ``i`` and
``j`` and the weight ``t`` of ``evaluate.percentile_ranks``, and :func:`percentile_of_values` interpolates between the two samples in float64.
The device route (C-ABI ``ts2d_label_percentiles``, ``csrc/kernels_stats_select.h``) SELECTS only - a most-significant-digit-first radix
selection straight over (segmentation, intensity) pairs inside the label's box, the counts, the two samples and the weight bit for bit -; the
interpolation runs on the host on both routes, so the percentiles are the same bits either way.
"""
from __future__ import annotations

import json
from typing import Dict, Optional, Sequence

import numpy as np

from .nrrd import Image

from .evaluate import _percentiles, percentile_key, percentile_ranks

LANES = 64
# No size gate: the device route lost at no measured size, the small end included - 117 labels at 53 x 133 with 2 channels take 1.05 ms there
# against 15.8 ms for the statement and 5.8 ms for plain per-label numpy (scripts/gpu_statistics_case.py, profiles/r28_statistics_case.txt).
# No size gate for the percentiles either: at the same small end q = (5, 50, 95) take 1.44 ms on the device against 11.1 ms for the statement and
# 14.4 ms for np.percentile per label and channel (scripts/gpu_statistics_percentiles_case.py, profiles/r35_statistics_percentiles_case.txt).


def float_keys(x: np.ndarray) -> np.ndarray:
    """``rs_key`` of csrc/ray_select.h for float32: uint32 keys with ``a < b <=> key(a) < key(b)``, ``-0.0`` right below ``+0.0``."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def float_unkeys(k: np.ndarray) -> np.ndarray:
    """The inverse of :func:`float_keys`."""
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _halve(v: np.ndarray) -> np.ndarray:
    """[..., 64] -> [...]: v[l] + v[l + 32], then + 16, ..., + 1."""
    n = LANES // 2
    while n >= 1:
        v = v[..., :n] + v[..., n:2 * n]
        n //= 2
    return v[..., 0]


def _lanes(t: np.ndarray) -> np.ndarray:
    """[..., N] -> [...]: lane l adds t[l], t[l + 64], ... in that order from +0.0, then the halving.  The lanes beyond N hold +0.0."""
    n = t.shape[-1]
    steps = -(-n // LANES)
    pad = np.zeros(t.shape[:-1] + (steps * LANES,), np.float64)
    pad[..., :n] = t
    pad = pad.reshape(t.shape[:-1] + (steps, LANES))
    acc = np.zeros(t.shape[:-1] + (LANES,), np.float64)
    for j in range(steps):
        acc = acc + pad[..., j, :]
    return _halve(acc)


def tree_sum(terms: np.ndarray) -> np.float64:
    """The fixed summation tree over float64 ``terms`` [rows, W] (module docstring): rows first, then the row partials."""
    return np.float64(_lanes(_lanes(np.asarray(terms, dtype=np.float64))))


def label_statistics_statement(seg: np.ndarray, intensities: Optional[np.ndarray], spacing: Sequence[float], values: Optional[Sequence[int]] = None) -> dict:
    """THE DEFINITION.  ``seg``: with ``values=None`` the planes of a multi-component segmentation, plane-major ``[K, *spatial]`` - label
    ``k`` (from 1) is ``seg[k - 1] > 0``, as in ``image.get_label_mask``; with ``values`` a label map ``[*spatial]`` - label ``k`` is
    ``seg == values[k - 1]``.  ``intensities``: ``[C, *spatial]`` float32 (C >= 0) or None.  ``spacing``: the image's, for ``mm``.

    Returns arrays over the K labels: ``count`` int64, ``exists`` bool, ``mm`` float64 = ``count * prod(spacing)`` (the reference's
    ``get_voxel_mm``: every axis, a unit axis included), ``bbox_min`` / ``bbox_max`` int64 [K, nd] (inclusive, per ARRAY axis; an empty
    label: the extents and -1), ``index_sum`` int64 [K, nd], and [K, C]: ``min`` / ``max`` float32, ``sum`` / ``ssq`` / ``mean`` / ``std``
    float64 (an empty label: zeros - the callers report None)."""
    seg = np.asarray(seg)
    if values is None:
        spatial, K = seg.shape[1:], seg.shape[0]
    else:
        spatial, K = seg.shape, len(values)
    nd = len(spatial)
    if nd < 1:
        raise ValueError("label_statistics_statement: the segmentation has no spatial axis")
    x = None
    if intensities is not None and np.asarray(intensities).shape[0] > 0:
        x = np.asarray(intensities)
        if x.shape[1:] != tuple(spatial):
            raise ValueError(f"label_statistics_statement: intensities {x.shape[1:]} do not have the segmentation's shape {tuple(spatial)}")
        x = np.ascontiguousarray(x, dtype=np.float32)
    C = 0 if x is None else x.shape[0]
    W = spatial[-1]
    rows = int(np.prod(spatial[:-1], dtype=np.int64))
    x64 = [x[c].reshape(rows, W).astype(np.float64) for c in range(C)]
    keys = [float_keys(x[c]).reshape(rows, W) for c in range(C)]
    out = {'count': np.zeros(K, np.int64), 'bbox_min': np.tile(np.asarray(spatial, np.int64), (K, 1)), 'bbox_max': np.full((K, nd), -1, np.int64),
           'index_sum': np.zeros((K, nd), np.int64), 'min': np.zeros((K, C), np.float32), 'max': np.zeros((K, C), np.float32),
           'sum': np.zeros((K, C), np.float64), 'ssq': np.zeros((K, C), np.float64), 'mean': np.zeros((K, C), np.float64),
           'std': np.zeros((K, C), np.float64)}
    zero = np.float64(0.0)
    for k in range(K):
        mask = (seg[k] > 0) if values is None else (seg == values[k])
        n = int(np.count_nonzero(mask))
        out['count'][k] = n
        if n == 0:
            continue
        for a in range(nd):          # the samples per index along axis a: box and index sum from them, in integers
            per = np.count_nonzero(mask, axis=tuple(b for b in range(nd) if b != a)).astype(np.int64) if nd > 1 else mask.astype(np.int64)
            at = np.flatnonzero(per)
            out['bbox_min'][k, a], out['bbox_max'][k, a] = at[0], at[-1]
            out['index_sum'][k, a] = int((per * np.arange(spatial[a], dtype=np.int64)).sum())
        m2 = mask.reshape(rows, W)
        live = np.flatnonzero(m2.any(axis=1))          # a row without a sample of the label has the partial +0.0: only the others are walked
        m2 = m2[live]

        def tree(terms):
            partial = np.zeros(rows, np.float64)
            partial[live] = _lanes(terms)
            return np.float64(_lanes(partial))

        with np.errstate(invalid='ignore', over='ignore'):
            for c in range(C):
                kk = keys[c][live][m2]
                out['min'][k, c] = float_unkeys(kk.min())
                out['max'][k, c] = float_unkeys(kk.max())
                xl = x64[c][live]
                s = tree(np.where(m2, xl, zero))
                mean = s / np.float64(n)
                d = xl - mean
                ssq = tree(np.where(m2, d * d, zero))          # (numpy rounds the product before the sum: no fused multiply-add)
                out['sum'][k, c], out['mean'][k, c], out['ssq'][k, c] = s, mean, ssq
                out['std'][k, c] = np.sqrt(ssq / np.float64(n))
    out['exists'] = out['count'] > 0
    out['mm'] = out['count'].astype(np.float64) * np.float64(np.prod(np.asarray(spacing, dtype=np.float64)))
    return out


def _device_statistics(planes, values, spatial, x, spacing, device: int, max_scratch_bytes: int = 0) -> Optional[dict]:
    """The statement's dict from ``ts2d_label_statistics``; None where the entry set a status bit."""
    from . import _lib, engine
    nd = len(spatial)
    zhw = (1,) * (3 - nd) + tuple(int(v) for v in spatial)
    got = engine.label_statistics(planes, _lib.STATS_PLANES if values is None else _lib.STATS_LABELMAP, values, zhw, x, max_scratch_bytes, device)
    if got is None:
        return None
    oi, of = got
    ax = slice(3 - nd, 3)
    out = {'count': oi[:, 0].copy(), 'index_sum': oi[:, 1:4][:, ax].copy(), 'bbox_min': oi[:, 4:10:2][:, ax].copy(), 'bbox_max': oi[:, 5:10:2][:, ax].copy(),
           'sum': of[:, :, 0].copy(), 'ssq': of[:, :, 1].copy(), 'mean': of[:, :, 2].copy(), 'std': of[:, :, 3].copy(),
           'min': of[:, :, 4].astype(np.float32), 'max': of[:, :, 5].astype(np.float32)}          # (exact: the entry widened float32 values)
    out['exists'] = out['count'] > 0
    out['mm'] = out['count'].astype(np.float64) * np.float64(np.prod(np.asarray(spacing, dtype=np.float64)))
    return out


def percentile_of_values(lo, hi, t) -> np.float64:
    """The percentile from the two selected samples and the weight (``evaluate.percentile_ranks``): numpy's linear method on the two values
    widened exactly to float64, every operation rounded on its own.  ``lo`` where ``t == 0`` or ``hi == lo``, else ``lo + (hi - lo) * t`` for
    ``t < 0.5`` and ``hi - (hi - lo) * (1 - t)`` from there (``evaluate.percentile_of_ranks`` without the roots).  Infinite samples give what
    IEEE gives."""
    lo, hi, t = np.float64(lo), np.float64(hi), np.float64(t)
    if t == 0 or hi == lo:
        return lo
    with np.errstate(invalid='ignore', over='ignore'):
        if t < 0.5:
            return lo + (hi - lo) * t
        return hi - (hi - lo) * (np.float64(1) - t)


def _percentiles_of_ranks(count: np.ndarray, rank_value: np.ndarray, rank_weight: np.ndarray) -> np.ndarray:
    """float64 [K, C, P]: :func:`percentile_of_values` of every selected pair; zeros for an empty label."""
    K, C, P = rank_value.shape[:3]
    out = np.zeros((K, C, P), np.float64)
    for k in range(K):
        if count[k] > 0:
            for c in range(C):
                for p in range(P):
                    out[k, c, p] = percentile_of_values(rank_value[k, c, p, 0], rank_value[k, c, p, 1], rank_weight[k, p])
    return out


def label_percentiles_statement(seg: np.ndarray, intensities: np.ndarray, percentiles: Sequence[float], values: Optional[Sequence[int]] = None) -> dict:
    """THE DEFINITION of the percentiles under a label.  ``seg``, ``values``: as in :func:`label_statistics_statement`; ``intensities``:
    ``[C, *spatial]`` float32, C >= 1; ``percentiles``: at most 8, each finite and in 0 ... 100 (``evaluate``'s check), else ``ValueError``.

    For label ``k`` with ``n > 0`` samples and percentile ``q``, ``(i, j, t) = evaluate.percentile_ranks(n, q)``; the samples of channel ``c``
    under the label are ordered by their keys (:func:`float_keys`).  Returns ``count`` int64 [K]; ``rank_value`` float32 [K, C, P, 2], the
    samples at the sorted positions ``i`` and ``j``; ``rank_weight`` float64 [K, P] = ``t``; ``percentile`` float64 [K, C, P] =
    :func:`percentile_of_values` of them.  An empty label: zeros everywhere (the callers report None).  A NaN under the label makes every
    percentile of that (label, channel) NaN, as ``np.percentile`` does; infinities are ordinary keys.  The definition is the sorted order; the
    two positions are taken with ``np.partition``."""
    qs = _percentiles(percentiles, 'label_percentiles_statement')
    seg = np.asarray(seg)
    if values is None:
        spatial, K = seg.shape[1:], seg.shape[0]
    else:
        spatial, K = seg.shape, len(values)
    if len(spatial) < 1:
        raise ValueError("label_percentiles_statement: the segmentation has no spatial axis")
    x = np.asarray(intensities)
    if x.ndim != len(spatial) + 1 or x.shape[0] < 1 or x.shape[1:] != tuple(spatial):
        raise ValueError(f"label_percentiles_statement: intensities {x.shape} are not [C >= 1, *{tuple(spatial)}]")
    x = np.ascontiguousarray(x, dtype=np.float32)
    C, P = x.shape[0], len(qs)
    keys = [float_keys(x[c]) for c in range(C)]
    out = {'count': np.zeros(K, np.int64), 'rank_value': np.zeros((K, C, P, 2), np.float32), 'rank_weight': np.zeros((K, P), np.float64)}
    nan = np.zeros((K, C), bool)
    for k in range(K):
        mask = (seg[k] > 0) if values is None else (seg == values[k])
        n = int(np.count_nonzero(mask))
        out['count'][k] = n
        if n == 0 or P == 0:
            continue
        ranks = [percentile_ranks(n, q) for q in qs]
        at = sorted({r for i, j, _ in ranks for r in (i, j)})
        out['rank_weight'][k] = [t for _, _, t in ranks]
        for c in range(C):
            kk = np.partition(keys[c][mask], at)
            nan[k, c] = bool(np.isnan(x[c][mask]).any())
            for p, (i, j, _) in enumerate(ranks):
                out['rank_value'][k, c, p] = float_unkeys(kk[[i, j]])
    out['percentile'] = _percentiles_of_ranks(out['count'], out['rank_value'], out['rank_weight'])
    out['percentile'][nan] = np.nan
    return out


def _device_percentiles(planes, values, spatial, x, qs, device: int, max_scratch_bytes: int = 0) -> Optional[dict]:
    """The statement's dict from ``ts2d_label_percentiles`` (the interpolation on the host); None where the entry set a status bit."""
    from . import _lib, engine
    nd = len(spatial)
    zhw = (1,) * (3 - nd) + tuple(int(v) for v in spatial)
    got = engine.label_percentiles(planes, _lib.STATS_PLANES if values is None else _lib.STATS_LABELMAP, values, zhw, x, qs, max_scratch_bytes, device)
    if got is None:
        return None
    count, rank_value, rank_weight = got
    return {'count': count, 'rank_value': rank_value, 'rank_weight': rank_weight, 'percentile': _percentiles_of_ranks(count, rank_value, rank_weight)}


def device_serves_percentiles(planes: np.ndarray, values, spatial, C: int, P: int) -> bool:
    """Does ``ts2d_label_percentiles`` serve the case?  What :func:`device_serves` asks, at least one channel and one percentile, and a library
    that has the symbol."""
    from . import engine
    return C >= 1 and P >= 1 and device_serves(planes, values, spatial, C) and engine.has_entry('ts2d_label_percentiles')


def device_serves(planes: np.ndarray, values, spatial, C: int) -> bool:
    """Does ``ts2d_label_statistics`` serve the case?  uint8 samples, 2 or 3 spatial axes, at most 2^31 - 1 voxels, 1 ... 255 labels with values
    1 ... 255, at most 64 channels, and a library that has the symbol."""
    from . import _lib
    K = planes.shape[0] if values is None else len(values)
    if planes.dtype != np.uint8 or len(spatial) not in (2, 3) or not 1 <= K <= 255 or C > _lib.STATS_MAX_CHANNELS:
        return False
    if min(spatial) < 1 or int(np.prod(spatial, dtype=np.int64)) > 2 ** 31 - 1:
        return False
    if values is not None and not all(1 <= int(v) <= 255 for v in values):
        return False
    from . import engine
    return engine.has_entry('ts2d_label_statistics')


def _array_of(img) -> np.ndarray:
    if isinstance(img, Image):
        if img.components != 1:
            raise ValueError(f"label_statistics: an intensity image has {img.components} components; hand over its channels one by one")
        return img.array
    return np.asarray(img)


def label_statistics(seg: Image, intensities: Optional[dict] = None, device: Optional[int] = None, percentiles: Sequence[float] = ()) -> Dict[str, dict]:
    """name -> statistics for every named label of ``seg`` (the names and values of ``image.get_annotation_labels``).

    ``seg``: a multi-component segmentation (label ``v`` is component ``v - 1`` > 0) or a label map (label ``v`` is ``seg == v``).
    ``intensities``: ``{channel name: scalar Image or array}`` of the segmentation's spatial shape (for a ``TS2D`` result the images of
    ``Result.get_projection()``; for ``HIPModel.apply`` the input's channels), cast to float32; a mismatch raises ``ValueError``.

    Per label: ``value``, ``exists``, ``count``, ``mm`` (= count * prod(spacing)), ``bbox`` = [[min per array axis], [max per array axis]]
    (inclusive), ``centroid_index`` = index sums / count per ARRAY axis (float64), ``centroid_physical`` = origin + D @ (spacing * index) in
    the image's (x, y[, z]) order, ``intensity[channel]`` = ``{min, max, mean, std}``; for an empty label every field from ``bbox`` on is None.

    Route: ``ts2d_label_statistics`` where ``device`` is given, the library has the symbol and the entry serves the case
    (:func:`device_serves`), else :func:`label_statistics_statement`; a status bit of the entry (a non-finite intensity under a label) sends
    the case to the statement too.  The numbers are the same bit for bit.  A plane-major multi-component segmentation (the merged result,
    what ``export.py`` builds) is handed over without a copy; an interleaved one (a file read back) is made plane-major first.

    ``percentiles`` (at most 8, each finite and in 0 ... 100, else ``ValueError``) adds to every ``intensity[channel]`` the key
    ``'percentile'``: ``{evaluate.percentile_key(q): value}``, numpy's linear percentile of the channel's samples under the label (50: the
    median); an empty label gets None for every ``q``.  Route: ``ts2d_label_percentiles`` under the conditions above and with at least one
    channel (:func:`device_serves_percentiles`), else :func:`label_percentiles_statement`; a status bit sends the case to the statement.  The
    device selects, the host interpolates (:func:`percentile_of_values`) on both routes: the same bits.  With ``percentiles=()`` the dict and
    the device calls are those of before."""
    from .image import get_annotation_labels
    qs = _percentiles(percentiles, 'label_statistics')
    names = get_annotation_labels(seg)
    multi = seg.components > 1
    spatial = tuple(seg.array.shape[:seg.dimension])
    if multi:
        planes = np.moveaxis(seg.array, -1, 0)
        if not planes.flags['C_CONTIGUOUS']:
            planes = np.ascontiguousarray(planes)
        values = None
        bad = [n for n, i in names.items() if not 1 <= int(i['value']) <= seg.components]
        if bad:
            raise ValueError(f"label_statistics: labels {bad} name a component beyond the segmentation's {seg.components}")
        index = {n: int(i['value']) - 1 for n, i in names.items()}
    else:
        planes = np.ascontiguousarray(seg.array)
        values = [int(i['value']) for i in names.values()]
        index = {n: j for j, n in enumerate(names)}
    chans = list((intensities or {}).keys())
    x = None
    if chans:
        arrs = [_array_of(intensities[c]) for c in chans]
        for c, a in zip(chans, arrs):
            if tuple(a.shape) != spatial:
                raise ValueError(f"label_statistics: intensity image {c!r} has shape {tuple(a.shape)}, the segmentation {spatial}")
        x = np.ascontiguousarray(np.stack(arrs), dtype=np.float32)
    raw = None
    if names and device is not None and device_serves(planes, values, spatial, len(chans)):
        raw = _device_statistics(planes, values, spatial, x, seg.spacing, int(device))
    if raw is None:
        raw = label_statistics_statement(planes, x, seg.spacing, values) if names else None
    pct = None
    if qs and names and chans:
        if device is not None and device_serves_percentiles(planes, values, spatial, len(chans), len(qs)):
            pct = _device_percentiles(planes, values, spatial, x, qs, int(device))
        if pct is None:
            pct = label_percentiles_statement(planes, x, qs, values)
    nd = len(spatial)
    origin = np.asarray(seg.origin, np.float64)
    D = np.asarray(seg.direction, np.float64).reshape(nd, nd)
    sp = np.asarray(seg.spacing, np.float64)
    out: Dict[str, dict] = {}
    for name, info in names.items():
        j = index[name]
        n = int(raw['count'][j])
        e = {'value': int(info['value']), 'exists': n > 0, 'count': n, 'mm': float(raw['mm'][j]), 'bbox': None, 'centroid_index': None,
             'centroid_physical': None, 'intensity': {c: {'min': None, 'max': None, 'mean': None, 'std': None} for c in chans}}
        if qs:
            for c in chans:
                e['intensity'][c]['percentile'] = {percentile_key(q): None for q in qs}
        if n > 0:
            e['bbox'] = [[int(v) for v in raw['bbox_min'][j]], [int(v) for v in raw['bbox_max'][j]]]
            ci = raw['index_sum'][j].astype(np.float64) / np.float64(n)
            e['centroid_index'] = [float(v) for v in ci]
            e['centroid_physical'] = [float(v) for v in origin + D @ (sp * ci[::-1])]
            for i, c in enumerate(chans):
                e['intensity'][c] = {'min': float(raw['min'][j, i]), 'max': float(raw['max'][j, i]), 'mean': float(raw['mean'][j, i]),
                                     'std': float(raw['std'][j, i])}
                if qs:
                    e['intensity'][c]['percentile'] = {percentile_key(q): float(pct['percentile'][j, i, p]) for p, q in enumerate(qs)}
        out[name] = e
    return out


def dump_statistics(stats: dict, path: str) -> str:
    """``json.dump`` with sorted keys; Python floats, so the file reads back to the dict (None is ``null``)."""
    with open(path, 'w') as f:
        json.dump(stats, f, sort_keys=True, indent=1)
        f.write('\n')
    return path
