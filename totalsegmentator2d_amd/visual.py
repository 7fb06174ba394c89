"""PNG visuals: ``create_visual`` (reference ``ts2d/core/util/image.py:383-453``) as a numpy float64 STATEMENT, and the device route behind it.

SimpleITK is not installed here, so ITK's bytes cannot be pinned; as with ``image.project`` and ``postprocess.keep_largest_components_statement``
the functions of this module ARE the definition, and the device entries ``ts2d_visual_labels`` / ``ts2d_visual_grey`` (csrc/kernels_visual.h,
csrc/visual.hip, host tables in csrc/visual_plan.cpp) reproduce them byte for byte.  Where a step restates ITK from memory the docstring says
[UPSTREAM-RECALL].

Steps of :func:`create_visual`: reorient, collapse the unit axes, project while more than two axes are left, then
  labels:  flatten a multi-component image to 1 + the index of its LAST non-zero component (:func:`flatten_index`), nearest-neighbour resample to
           isotropic pixels (:func:`axis_table`), colour ``palette[v % len(palette)]``, 0 -> black (:func:`label_rgb`);
  grey:    resample (uint8: nearest; else the cubic B-spline of :func:`resample_cubic`, cast back to the pixel type), window to 0 ... 255
           (:func:`window_u8`).
"""
from __future__ import annotations

import math
import random
import warnings
from typing import Optional, Sequence

import numpy as np

from .nrrd import Image

POLE = float.fromhex('-0x1.126145e9ecd56p-2')          # the float64 nearest to sqrt(3) - 2 (preprocess.CUBIC_POLE)
GAIN = (1.0 - POLE) * (1.0 - 1.0 / POLE)
MAX_EXTENT = 8192                                       # per input axis of the device entries
MAX_OUT_EXTENT = 32768                                  # per output axis of the device entries
DEVICE_DTYPES = {'int16': 0, 'uint8': 1, 'float32': 2, 'uint16': 3, 'int32': 4}      # the dtype codes of ts2d_project_coronal
VISUAL_NONFINITE = 1                                    # TS2D_VISUAL_NONFINITE
# Size gates of the device route, from profiles/r27_visual_case.txt (a call costs about 0.15 ms of allocation, copies and synchronisation, a label
# call another 0.01 ms per plane uploaded).  Labels: the host wins at 53 x 133 with K = 117 (0.8 M plane samples, 0.4 - 0.6x) and K = 18, the device
# from 644 x 337 with K = 18 (3.9 M, 2.9 - 3.3x).  A grey plane that needs no resample is one multiply-add per sample on the host: it wins at 53 x 133
# (0.3x) and 320 x 320 (0.85 - 0.97x), the device from 644 x 337 (1.2 - 1.4x).  A grey plane that IS resampled won at every measured size (4.5x at 53 x 133).
LABELS_DEVICE_MIN = 1 << 21                             # K * H * W plane samples from which labels take the device route
GREY_UNIFORM_DEVICE_MIN = 1 << 17                       # H * W samples from which a grey plane without resample takes it

_BASE_COLORS = ((255, 0, 0), (0, 128, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255))      # matplotlib's red, green, blue, yellow, cyan, magenta
_NAMED = dict(zip(('red', 'green', 'blue', 'yellow', 'cyan', 'magenta'), _BASE_COLORS), white=(255, 255, 255), black=(0, 0, 0))


# ----------------------------------------------------------------------------- palette
def default_color(index: int) -> tuple:
    """Reference ``color.default_color``: six named colours, then ``random.Random(index)`` with three ``randint(32, 200)``."""
    assert index >= 0
    if index < len(_BASE_COLORS):
        return _BASE_COLORS[index]
    r = random.Random(index)
    return tuple(r.randint(32, 200) for _ in range(3))


def to_color(c) -> tuple:
    """Reference ``color.to_color``: an int is ``default_color``, a '#RRGGBB' string or one of the eight names above its bytes, an integer triple
    is clipped to 0 ... 255, a float triple becomes ``int(clip(v, 0, 1) * 255)`` per component."""
    if isinstance(c, (int, np.integer)):
        return default_color(int(c))
    if isinstance(c, str):
        s = c.strip().lower()
        if s in _NAMED:
            return _NAMED[s]
        h = s.lstrip('#')
        if len(h) != 6:
            raise ValueError(f"unsupported colour string: {c!r} (matplotlib is not used here: '#RRGGBB' or one of {sorted(_NAMED)})")
        return tuple(int(h[i:i + 2], 16) for i in (0, 2, 4))
    v = tuple(c)
    if len(v) != 3:
        raise RuntimeError(f"Color tuples need to be of length 3 (found: {len(v)})")
    if any(not isinstance(x, (int, np.integer)) for x in v):
        return tuple(int(min(max(float(x), 0.0), 1.0) * 255) for x in v)
    return tuple(min(max(int(x), 0), 255) for x in v)


def to_palette(v) -> list:
    """Reference ``color.to_palette``: a dict value -> colour becomes a list whose entry 0 is white and whose entry i is the given colour or
    ``default_color(i)``; a list is converted entry by entry."""
    if isinstance(v, dict):
        if any(not isinstance(k, (int, np.integer)) or k < 0 for k in v):
            raise RuntimeError("Dictionary palette must consist of non-negative integer keys!")
        lim = max(v) if v else 0
        return [(255, 255, 255)] + [to_color(v[i]) if v.get(i) is not None else default_color(i) for i in range(1, lim + 1)]
    return [to_color(c) for c in v]


# ----------------------------------------------------------------------------- flatten
def flatten_index(planes: np.ndarray) -> np.ndarray:
    """``image_vector_flatten_max(index=True)`` over planes ``[K, ...]``: per pixel 1 + the index of the LAST non-zero plane, 0 when all are
    zero, as uint8 - more than 255 planes raise (the reference's resample output is uint8)."""
    K = planes.shape[0]
    if K > 255:
        raise ValueError(f"flatten_index: {K} components do not fit the uint8 label map of the visual (at most 255)")
    out = np.zeros(planes.shape[1:], np.uint8)
    for k in range(K):
        out[planes[k] != 0] = k + 1
    return out


# ----------------------------------------------------------------------------- geometry
def _fold(i: np.ndarray, n: int) -> np.ndarray:
    """Mirror index folding (``... 2 1 0 1 2 ... n-1 n-2 ...``) of any integer onto 0 ... n-1."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i > n - 1, p - i, i)


def uniform_extent(N: int, s: float, m: float) -> int:
    """Samples of an axis of ``N`` samples at spacing ``s`` resampled to spacing ``m`` (``resample_filter``): ``int(0.5 + N*s/m)``."""
    return int(0.5 + N * float(s) / float(m))


def axis_table(N: int, s: float, m: float) -> dict:
    """One axis of ``resample_uniform`` (``resample_filter`` with the direction cancelled).  Output index j reads the continuous source index
    ``x_j = (N//2) + (j - M//2) * (m/s)`` - float64, in that order; it is inside iff ``-0.5 <= x < N - 0.5``.  Returns ``M``, ``x``,
    ``inside``, ``nearest`` = ``floor(x + 0.5)`` [UPSTREAM-RECALL: ITK's RoundHalfIntegerUp] (never above N - 1) or -1 outside, and the cubic taps: ``idx[M, 4]`` =
    ``floor(x) - 1 ... floor(x) + 2`` mirror-folded, ``w[M, 4]`` the cubic B-spline of ``y = x - floor(x)``, ``t = 1 - y``, one rounding per
    step: ``w1 = (y*y*(y-2)*3 + 4) / 6``, ``w2 = (t*t*(t-2)*3 + 4) / 6``, ``w0 = t*t*t / 6``, ``w3 = 1 - w0 - w1 - w2`` (scipy's order).  Outside
    entries have zero weights and indices.  csrc/visual_plan.cpp builds the same table."""
    N = int(N)
    M = uniform_extent(N, s, m)
    j = np.arange(M, dtype=np.int64) - (M // 2)
    x = np.float64(N // 2) + j.astype(np.float64) * (np.float64(m) / np.float64(s))
    inside = (x >= -0.5) & (x < np.float64(N) - 0.5)
    nearest = np.where(inside, np.minimum(np.floor(x + 0.5), np.float64(N - 1)), -1.0).astype(np.int64)
    f = np.floor(x)
    y = x - f
    t = 1.0 - y
    w = np.empty((M, 4), np.float64)
    w[:, 1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 2] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 0] = t * t * t / 6.0
    w[:, 3] = 1.0 - w[:, 0] - w[:, 1] - w[:, 2]
    idx = _fold(np.where(inside, f, 0.0).astype(np.int64)[:, None] + np.arange(-1, 3, dtype=np.int64)[None, :], N)
    idx[~inside] = 0
    w[~inside] = 0.0
    return {'M': M, 'x': x, 'inside': inside, 'nearest': nearest, 'idx': idx, 'w': w}


def is_uniform(spacing) -> bool:
    """``np.allclose(spacing, min(spacing))``: no resample at all, the plane passes through unchanged."""
    return bool(np.allclose(spacing, min(spacing)))


def resample_nearest(plane: np.ndarray, ty: dict, tx: dict) -> np.ndarray:
    """Nearest-neighbour gather through two :func:`axis_table` s; outside pixels are 0."""
    out = plane[np.clip(ty['nearest'], 0, None)[:, None], np.clip(tx['nearest'], 0, None)[None, :]]
    out[~(ty['inside'][:, None] & tx['inside'][None, :])] = 0
    return out


# ----------------------------------------------------------------------------- cubic B-spline
def spline_prefilter_axis0(c: np.ndarray) -> np.ndarray:
    """The cubic B-spline prefilter of ``scipy.ndimage.spline_filter(order=3, mode='mirror')`` along axis 0 of a float64 ``[n, m]`` array, in
    place, restated with one rounding per product and sum and no division inside the line (the two quotients are line-independent constants):
    the gain on every sample; ``acc = c[0] + z^(n-1) * c[n-1]``, for i = 1 ... n-2 ``acc += z_i * (c[i] + z^(n-1) * c[n-1-i])`` with the running
    product ``z_i`` (z, z*z, ...), ``c[0] = acc * (1 / (1 - z^(n-1) * z^(n-1)))``; ``c[i] += z * c[i-1]``;
    ``c[n-1] = (z * c[n-2] + c[n-1]) * (z / (z*z - 1))``; ``c[i] = z * (c[i+1] - c[i])``.  A line of one sample is left as it is."""
    n = c.shape[0]
    if n < 2:
        return c
    z = POLE
    c *= GAIN
    zn1 = math.pow(z, float(n - 1))
    acc = c[0] + zn1 * c[n - 1]
    z_i = z
    for i in range(1, n - 1):
        acc = acc + z_i * (c[i] + zn1 * c[n - 1 - i])
        z_i = z_i * z
    c[0] = acc * (1.0 / (1.0 - zn1 * zn1))
    for i in range(1, n):
        c[i] = c[i] + z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * (z / (z * z - 1.0))
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def spline_coefficients(plane: np.ndarray) -> np.ndarray:
    """float64 coefficients ``[H, W]`` of a plane: :func:`spline_prefilter_axis0` along axis 0, then along axis 1."""
    c = np.array(plane, dtype=np.float64, order='C')
    c = spline_prefilter_axis0(c)
    return np.ascontiguousarray(spline_prefilter_axis0(np.ascontiguousarray(c.T)).T)


def cast_to_pixel_type(r: np.ndarray, dtype) -> np.ndarray:
    """float64 -> the pixel type: float32 takes one rounding, float64 none; an integer type is clamped to its range and truncated toward zero
    [UPSTREAM-RECALL: ITK's ResampleImageFilter clamps, then ``static_cast``]."""
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        return r.astype(dtype)
    info = np.iinfo(dtype)
    return np.trunc(np.clip(r, float(info.min), float(info.max))).astype(dtype)


def resample_cubic(plane: np.ndarray, ty: dict, tx: dict) -> np.ndarray:
    """The order-3 resample of one plane in float64, cast back to its type: coefficients (:func:`spline_coefficients`), per output pixel 16 taps
    - row tap outer, column tap inner - each ``(c * wy) * wx``, summed in that order from 0, every product and sum rounded on its own; outside
    pixels are 0."""
    c = spline_coefficients(plane)
    r = np.zeros((ty['M'], tx['M']), np.float64)
    for a in range(4):
        rows = c[ty['idx'][:, a]]
        for b in range(4):
            r = r + (rows[:, tx['idx'][:, b]] * ty['w'][:, a, None]) * tx['w'][None, :, b]
    r[~(ty['inside'][:, None] & tx['inside'][None, :])] = 0.0
    return cast_to_pixel_type(r, plane.dtype)


# ----------------------------------------------------------------------------- window
def auto_window(res: np.ndarray, method) -> tuple:
    """Reference ``get_auto_window``: None / 'minmax' = min and max of the RESAMPLED plane (outside zeros included), 'pcN' = the N-th and
    (100-N)-th ``np.percentile``, 'pcA-B' the two given."""
    method = 'minmax' if method is None else str(method).lower()
    if method == 'minmax':
        return float(res.min()), float(res.max())
    if method.startswith('pc'):
        try:
            pc = tuple(float(a) for a in method[2:].split('-')) if '-' in method[2:] else (float(method[2:]), 100.0 - float(method[2:]))
        except ValueError:
            raise RuntimeError(f"Failed to parse percentile value from windowing method: {method}") from None
        if len(pc) != 2:
            raise RuntimeError(f"The percentile can only be a range value: found value {method}")
        lo, hi = np.percentile(res, pc)
        return float(lo), float(hi)
    raise RuntimeError(f"Unkown windowing method: {method}")


def resolve_window(res: np.ndarray, window) -> tuple:
    """(lo, hi) as float64: a method name through :func:`auto_window`, a pair as given with its None entries filled from min / max."""
    if window is None or isinstance(window, str):
        return auto_window(res, window)
    lo, hi = window
    return (float(res.min()) if lo is None else float(lo)), (float(res.max()) if hi is None else float(hi))


def window_u8(res: np.ndarray, lo: float, hi: float) -> np.ndarray:
    """``sitk.IntensityWindowing(img, lo, hi, 0, 255)`` then ``Cast(uint8)``, in float64: below ``lo`` 0, above ``hi`` 255, else
    ``x * scale + shift`` with ``scale = 255 / (hi - lo)``, ``shift = -lo * scale`` (product and sum rounded on their own); one rounding to the
    pixel type (an integer type truncates), then truncation to uint8 (kept inside 0 ... 255).  ``hi == lo`` gives an all-zero plane: our
    definition, ITK's is undefined."""
    lo, hi = float(lo), float(hi)
    if hi == lo:
        return np.zeros(res.shape, np.uint8)
    x = res.astype(np.float64)
    scale = 255.0 / (hi - lo)
    shift = -lo * scale
    v = x * scale + shift
    v = np.where(x < lo, 0.0, np.where(x > hi, 255.0, v))
    if res.dtype == np.float32:
        v = v.astype(np.float32).astype(np.float64)
    return np.clip(np.trunc(v), 0.0, 255.0).astype(np.uint8)


def label_rgb(index_map: np.ndarray, palette: Sequence) -> np.ndarray:
    """``sitk.LabelToRGB(img, 0, colormap)``: value v > 0 takes ``palette[v % len(palette)]``, 0 is black [UPSTREAM-RECALL: the LabelToRGB
    functor]."""
    lut = color_lut(palette)
    return lut[index_map]


def color_lut(palette: Sequence) -> np.ndarray:
    """uint8 ``[256, 3]``: the colour of every uint8 label value under :func:`label_rgb`."""
    pal = np.asarray([tuple(c) for c in palette], dtype=np.uint8).reshape(-1, 3)
    if len(pal) == 0:
        raise ValueError("label_rgb: the palette is empty")
    lut = pal[np.arange(256) % len(pal)]
    lut[0] = 0
    return lut


# ----------------------------------------------------------------------------- the statement and the device route
def _labels_statement(planes: np.ndarray, spacing_hw, pal) -> np.ndarray:
    idx = flatten_index(planes) if planes.shape[0] > 1 else planes[0]
    if not is_uniform(spacing_hw):
        m = min(spacing_hw)
        idx = resample_nearest(idx, axis_table(idx.shape[0], spacing_hw[0], m), axis_table(idx.shape[1], spacing_hw[1], m))
    return label_rgb(idx, pal)


def _grey_statement(plane: np.ndarray, spacing_hw, window) -> np.ndarray:
    res = plane
    if not is_uniform(spacing_hw):
        m = min(spacing_hw)
        ty, tx = axis_table(plane.shape[0], spacing_hw[0], m), axis_table(plane.shape[1], spacing_hw[1], m)
        if plane.dtype == np.uint8:
            warnings.warn("SimpleITK does not permit interpolation of UInt8 images, falling back to nearest neighbour.")
            res = resample_nearest(plane, ty, tx)
        else:
            res = resample_cubic(plane, ty, tx)
    lo, hi = resolve_window(res, window)
    return window_u8(res, lo, hi)


def _device_entries():
    from . import _lib, engine
    return _lib.load() if engine.has_entry('ts2d_visual_labels', 'ts2d_visual_grey') else None


def _device_geometry(shape, spacing_hw):
    """(spacing handed to the entry, (h, w)) when the entries serve the extents, else None.  A uniform plane is handed over with spacing
    (1, 1): x_j = j exactly, every pixel inside."""
    H, W = int(shape[0]), int(shape[1])
    sp = (1.0, 1.0) if is_uniform(spacing_hw) else (float(spacing_hw[0]), float(spacing_hw[1]))
    if not all(math.isfinite(s) and s > 0 for s in sp):
        return None
    m = min(sp)
    h, w = uniform_extent(H, sp[0], m), uniform_extent(W, sp[1], m)
    if not (1 <= H <= MAX_EXTENT and 1 <= W <= MAX_EXTENT and 1 <= h <= MAX_OUT_EXTENT and 1 <= w <= MAX_OUT_EXTENT and h * w <= 1 << 28):
        return None
    return sp, (h, w)


def _labels_device(planes: np.ndarray, spacing_hw, pal, device) -> Optional[np.ndarray]:
    from . import engine
    geo = _device_geometry(planes.shape[1:], spacing_hw)
    if device is None or _device_entries() is None or geo is None or planes.dtype != np.uint8 or not 1 <= planes.shape[0] <= 255 or len(pal) > 256:
        return None
    if planes.size < LABELS_DEVICE_MIN:
        return None                                              # the statement is faster (see the gates above)
    return engine.visual_labels(planes, geo[0], np.asarray(pal, np.uint8).reshape(-1, 3), geo[1], device)


def _grey_device(plane: np.ndarray, spacing_hw, window, device) -> Optional[np.ndarray]:
    from . import engine
    geo = _device_geometry(plane.shape, spacing_hw)
    if device is None or _device_entries() is None or geo is None or plane.dtype.name not in DEVICE_DTYPES:
        return None
    if isinstance(window, str) and window.lower() != 'minmax':
        return None                                              # the percentile windows are host-only
    lo, hi = (None, None) if window is None or isinstance(window, str) else window
    if any(v is not None and not math.isfinite(float(v)) for v in (lo, hi)):
        return None
    if is_uniform(spacing_hw) and plane.size < GREY_UNIFORM_DEVICE_MIN:
        return None                                              # the statement is faster (see the gates above)
    cubic = not is_uniform(spacing_hw) and plane.dtype != np.uint8
    if cubic and min(plane.shape) < 2:
        return None
    if plane.dtype == np.uint8 and not is_uniform(spacing_hw):
        warnings.warn("SimpleITK does not permit interpolation of UInt8 images, falling back to nearest neighbour.")
    got = engine.visual_grey(plane, geo[0], cubic, lo, hi, geo[1], device)
    return None if got is None else got[0]


def create_visual(img: Image, mode='max', axis=-1, window=None, labels=None, palette=None, device: Optional[int] = None) -> Image:
    """The reference's ``create_visual``: a 2-D uint8 image of ``img`` with uniform spacing - ``[h, w]`` grey, or ``[h, w, 3]``
    (``components=3``) for labels.  ``labels=None`` means "a palette is given, or the image carries ``Segment*`` metadata"; the palette then comes
    from ``get_annotation_labels`` (value -> colour).  ``window``: None / 'minmax', 'pcN', or a ``(lo, hi)`` pair whose None entries are filled
    from min / max.  A multi-component image that is no label image raises ``ValueError``, as do more than 255 components.

    ``device``: a device index takes the entries ``ts2d_visual_labels`` / ``ts2d_visual_grey`` where the library has them and the case is one they
    serve (uint8 planes for labels; uint8, int16, uint16, int32 or float32 for grey; no percentile window; extents up to 8192; above the size
    gates ``LABELS_DEVICE_MIN`` / ``GREY_UNIFORM_DEVICE_MIN``, below which the statement is faster) and the entry sets no status bit (a non-finite float sample does); otherwise, and with ``device=None``, the result is the statement's - the bytes are the same."""
    from . import image as I
    if labels is None:
        labels = bool(palette) or any(k.startswith('Segment') for k in img.meta)
    if labels and not palette:
        palette = {}
        try:
            for info in I.get_annotation_labels(img).values():
                if info.get('value') is not None and info.get('color') is not None:
                    palette[int(info['value'])] = info['color']
        except Exception as ex:                                   # (the reference warns and goes on with what it has)
            warnings.warn(f"Failed to extract palette from image metadata: {ex}")
    img = I.reorient_image(img)
    _axis = I.axis_name_to_index(axis) if isinstance(axis, str) else (-1 if axis is None else axis)
    while img.dimension > 2:
        img = I.reduce_dimensions(img)
        if img.dimension <= 2:
            break
        img = I.project(img, mode=mode, axis=-1 if abs(_axis) > img.dimension else _axis)
    if img.dimension != 2:
        raise ValueError(f"create_visual: the image collapses to {img.dimension} axes, two are needed")
    spacing_hw = (float(img.spacing[1]), float(img.spacing[0]))      # array axis 0 is the image's second axis
    arr = img.array
    if labels:
        pal = to_palette(palette)
        planes = np.moveaxis(arr, -1, 0) if img.components > 1 else arr[None]
        if planes.shape[0] > 255:
            raise ValueError(f"create_visual: {planes.shape[0]} components do not fit the uint8 label map of the visual (at most 255)")
        if planes.dtype != np.uint8:
            planes = planes.astype(np.uint8)                        # (the reference's label resample writes uint8)
        planes = np.ascontiguousarray(planes)
        out = _labels_device(planes, spacing_hw, pal, device)
        if out is None:
            out = _labels_statement(planes, spacing_hw, pal)
        comps = 3
    else:
        if img.components > 1:
            raise ValueError("create_visual: a multi-component image that is no label image has no visual here (the reference's VectorMagnitude)")
        plane = np.ascontiguousarray(arr)
        out = _grey_device(plane, spacing_hw, window, device)
        if out is None:
            out = _grey_statement(plane, spacing_hw, window)
        comps = 1
    m = min(img.spacing)
    D = np.asarray(img.direction, dtype=np.float64).reshape(2, 2)
    old = np.asarray([(n // 2) * s for n, s in zip(img.size, img.spacing)], dtype=np.float64)
    new = np.asarray([(n // 2) * m for n in (out.shape[1], out.shape[0])], dtype=np.float64)
    origin = np.asarray(img.origin, dtype=np.float64) + D @ old - D @ new
    if is_uniform(img.spacing):
        origin, sp = np.asarray(img.origin, dtype=np.float64), tuple(img.spacing)
    else:
        sp = (m, m)
    return Image(out, sp, tuple(float(o) for o in origin), img.direction, comps, {}, img.space)
