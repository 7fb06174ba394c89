"""Input side of the hot path: nnU-Net's ``DefaultPreprocessor.run_case`` for the 2-D multi-channel inputs ts2d feeds.

Reference call site: ``ts2d/core/inference/prediction_worker.py:194-199`` (``preprocessor.run_case(task.filenames, None,
plans_manager, configuration_manager, dataset_json)`` -> ``(data[C,1,H,W] float32, None, properties)``).  The
algorithm is third-party (nnunetv2ml==2.6.2): read -> float32 -> transpose_forward ->
crop_to_nonzero -> per-channel normalisation (channel names ``mean`` / ``max`` are not ``ct`` => ZScoreNormalization)
-> resample to the plan spacing when the rounded target shape differs.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import nrrd


def sitk_stuff(img, files=()) -> dict:
    """``properties['sitk_stuff']`` as upstream's ``SimpleITKIO.read_images`` fills it [UPSTREAM-RECALL]: the geometry of the
    FIRST input image in SimpleITK order (x, y[, z]; direction flattened row-major).  Upstream's ``SimpleITKIO.write_seg``
    reads exactly these three keys back when the reference's unchanged exporter (``export_prediction_from_logits``,
    ``ts2d/core/inference/prediction_worker.py:215-221``) writes the result of THIS preprocessor's properties (INTEGRATION.md
    section 1)."""
    return {'spacing': tuple(float(v) for v in img.spacing), 'origin': tuple(float(v) for v in img.origin),
            'direction': tuple(float(v) for v in img.direction), 'files': list(files)}


def image_to_array(img) -> Tuple[np.ndarray, dict]:
    """One in-memory image -> (``[c, z, y, x]`` float32, properties); 2-D images get a unit z axis and nnU-Net's
    ``999`` pseudo-spacing."""
    a = np.asarray(img.array)
    if img.dimension == 2:
        a = a[None] if img.components == 1 else np.moveaxis(a, -1, 0)
        a = a[:, None]
        sp = (999.0, float(img.spacing[1]), float(img.spacing[0]))
    elif img.dimension == 3:
        a = a[None] if img.components == 1 else np.moveaxis(a, -1, 0)
        sp = (float(img.spacing[2]), float(img.spacing[1]), float(img.spacing[0]))
    else:
        raise RuntimeError(f"unsupported image dimension {img.dimension}")
    return a.astype(np.float32), {'spacing': sp, 'sitk_stuff': sitk_stuff(img)}


def read_images(files: Sequence[str]) -> Tuple[np.ndarray, dict]:
    """The fork's reader for one multi-component 2-D file (reference ``ts2d/tool.py:160,170-172`` hands the model ONE
    vector image): ``[y, x, c]`` -> ``[c, 1, y, x]``; spacing reported nnU-Net style ``(999, sy, sx)`` for 2-D."""
    arrs, spacing, stuff = [], None, None
    for fp in files:
        img = nrrd.read(fp)
        a = np.asarray(img.array)
        if img.dimension == 2:
            a = a[None] if img.components == 1 else np.moveaxis(a, -1, 0)      # [c, y, x]
            a = a[:, None]                                                      # [c, 1, y, x]
            sp = (999.0, float(img.spacing[1]), float(img.spacing[0]))
        elif img.dimension == 3:
            a = a[None] if img.components == 1 else np.moveaxis(a, -1, 0)      # [c, z, y, x]
            sp = (float(img.spacing[2]), float(img.spacing[1]), float(img.spacing[0]))
        else:
            raise RuntimeError(f"unsupported image dimension {img.dimension} in {fp}")
        arrs.append(a)
        if stuff is None:                       # upstream keeps the first image's geometry (and checks the others against it)
            spacing, stuff = sp, sitk_stuff(img, files)
    data = np.concatenate(arrs, 0).astype(np.float32)
    return data, {'spacing': spacing, 'sitk_stuff': stuff}


def crop_to_nonzero(data: np.ndarray, return_mask: bool = False):
    """``crop_to_nonzero``: bounding box of voxels that are non-zero in ANY channel.  ``return_mask``: also the non-zero mask inside
    the box - upstream writes it into the segmentation (``seg = where(nonzero_mask, 0, -1)``) and the masked normalisers use
    ``seg >= 0``.  Upstream fills the holes of the mask (``create_nonzero_mask``: ``binary_fill_holes`` on the [Z, H, W] mask, default
    3-D structure) - a no-op for the [C, 1, H, W] inputs of the 2-D path (with Z = 1 every voxel lies on the array's border, so no
    background region is enclosed), applied here for Z > 1 so that a volume input is masked like upstream masks it [UPSTREAM-RECALL]."""
    nz = np.any(data != 0, axis=0)
    if nz.ndim == 3 and nz.shape[0] > 1:
        from scipy.ndimage import binary_fill_holes
        nz = binary_fill_holes(nz)
    if not nz.any():
        bbox = [[0, s] for s in data.shape[1:]]
    else:
        bbox = []
        for ax in range(nz.ndim):
            other = tuple(i for i in range(nz.ndim) if i != ax)
            idx = np.where(nz.any(axis=other))[0]
            bbox.append([int(idx[0]), int(idx[-1]) + 1])
    sl = (slice(None),) + tuple(slice(b[0], b[1]) for b in bbox)
    if return_mask:
        return data[sl], bbox, nz[sl[1:]]
    return data[sl], bbox


def zscore(img: np.ndarray) -> np.ndarray:
    """``ZScoreNormalization.run`` (no mask): float32, ``(x - mean) / max(std, 1e-8)``."""
    img = img.astype(np.float32, copy=True)
    mean, std = img.mean(), img.std()
    img -= mean
    img /= max(std, 1e-8)
    return img


def normalize_channel(img: np.ndarray, scheme: str, use_mask: bool, mask: Optional[np.ndarray], props: Optional[dict]) -> np.ndarray:
    """nnU-Net ``default_normalization_schemes`` [UPSTREAM-RECALL nnunetv2 2.6], float32 like upstream's ``target_dtype``:
    ZScoreNormalization (optionally inside the non-zero mask only: outside stays 0), CTNormalization (clip to the dataset's
    0.5 / 99.5 percentiles, then the dataset's mean / std: ``plans['foreground_intensity_properties_per_channel'][str(c)]``),
    NoNormalization, RescaleTo01Normalization, RGBTo01Normalization."""
    img = img.astype(np.float32, copy=True)
    if scheme == 'ZScoreNormalization':
        if use_mask:
            if mask is None:
                raise RuntimeError("masked ZScoreNormalization needs the non-zero mask")
            m = mask.astype(bool)
            mean, std = img[m].mean(), img[m].std()
            img[m] = (img[m] - mean) / max(std, 1e-8)
            return img
        return zscore(img)
    if scheme == 'CTNormalization':
        if not props:
            raise RuntimeError("CTNormalization needs plans['foreground_intensity_properties_per_channel']")
        lo, hi = props['percentile_00_5'], props['percentile_99_5']
        np.clip(img, lo, hi, out=img)
        img -= np.float32(props['mean'])
        img /= np.float32(max(props['std'], 1e-8))
        return img
    if scheme == 'NoNormalization':
        return img
    if scheme == 'RescaleTo01Normalization':
        img -= img.min()
        img /= np.clip(img.max(), a_min=1e-8, a_max=None)
        return img
    if scheme == 'RGBTo01Normalization':
        if img.min() < 0 or img.max() > 255:
            raise RuntimeError("RGB images are uint 8, for whatever reason I found pixel values outside [0, 255]")
        return img / np.float32(255.0)
    raise NotImplementedError(f"normalization scheme {scheme} is not implemented")


def resize_like_skimage(img2d: np.ndarray, new_shape, order: int) -> np.ndarray:
    """``skimage.transform.resize(img, new_shape, order, mode='edge', anti_aliasing=False)`` of scikit-image >= 0.19 (nnU-Net's
    resampling primitive) restated with scipy, which is what skimage calls itself on this path [UPSTREAM-RECALL]:
    ``ndi.zoom(img, out / in, order, mode='nearest', grid_mode=True)`` followed by a clip to the input's value range
    (``clip=True``).  skimage is not installed here."""
    from scipy import ndimage as ndi
    img2d = np.asarray(img2d)
    if tuple(img2d.shape) == tuple(new_shape):
        return img2d
    zoom = [n / o for n, o in zip(new_shape, img2d.shape)]
    out = ndi.zoom(img2d, zoom, order=order, mode='nearest', grid_mode=True)
    if order > 0 and out.size:
        np.clip(out, img2d.min(), img2d.max(), out=out)
    return out.astype(img2d.dtype, copy=False)


def linear_axis_taps(n_in: int, n_out: int):
    """Taps of one axis of :func:`resize_linear_f64` (``n_in`` -> ``n_out`` samples), all in float64: the two source indices and their
    weights per output sample, ``(i0, i1, w0, w1)``.  As scipy does it for ``mode='nearest'``: the coordinate is NOT clamped - the array
    is extended by its edge samples, so the tap INDICES are clamped and a coordinate outside the array weighs the same edge sample twice.
    The C entry ts2d_engine_predict_tiled_export computes the same table on the host."""
    cc = (np.arange(n_out, dtype=np.float64) + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5
    f = np.floor(cc)
    w1 = cc - f
    i0 = f.astype(np.int64)
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), 1.0 - w1, w1


def resize_linear_f64(img2d: np.ndarray, new_shape) -> np.ndarray:
    """:func:`resize_like_skimage` with ``order=1`` as a closed form in float64, bit for bit what scipy returns (tests/test_resample_cpu.py:
    every float32 value, half-valued and full float32 input, and the same non-finite outputs for +-inf samples): four taps in the order
    (y0,x0), (y0,x1), (y1,x0), (y1,x1), each sample multiplied by its row weight and then by its column weight, the four products summed
    left to right, every product and sum rounded to float64 (no FMA), ONE rounding to the input's dtype.  The clip to the input's
    value range that follows in ``resize_like_skimage`` never changes an order-1 result (a convex combination, rounded once).  A zero
    weight on an infinite sample gives NaN, as in scipy.  This is the statement the device kernel ``sw_resample_threshold``
    (csrc/kernels_resample.h) reproduces bit for bit."""
    img2d = np.asarray(img2d)
    y0, y1, wy0, wy1 = linear_axis_taps(img2d.shape[0], int(new_shape[0]))
    x0, x1, wx0, wx1 = linear_axis_taps(img2d.shape[1], int(new_shape[1]))
    a = img2d.astype(np.float64)
    wy0, wy1, wx0, wx1 = wy0[:, None], wy1[:, None], wx0[None], wx1[None]
    with np.errstate(invalid='ignore'):                                   # (0 x inf = NaN is the pinned result, not a warning)
        r = (a[y0][:, x0] * wy0) * wx0
        r = r + (a[y0][:, x1] * wy0) * wx1
        r = r + (a[y1][:, x0] * wy1) * wx0
        r = r + (a[y1][:, x1] * wy1) * wx1
    return r.astype(img2d.dtype)


CUBIC_PAD = 12                                         # scipy's _prepad_for_spline_filter: edge samples per side for mode='nearest'
CUBIC_POLE = float.fromhex('-0x1.126145e9ecd56p-2')    # the float64 nearest to sqrt(3) - 2 (see resize_cubic_f64: NOT math.sqrt(3.0) - 2.0)
CUBIC_GAIN = (1.0 - CUBIC_POLE) * (1.0 - 1.0 / CUBIC_POLE)
CUBIC_MAX_EXTENT = 8192                                # per axis, input and output: the device entry's index arithmetic is sized for it


class CubicResampleLimit(ValueError):
    """A plane :func:`resize_cubic_f64` (and the device entry ts2d_resample_cubic) does not compute: the callers keep the scipy route."""


def cubic_axis_taps(n_in: int, n_out: int):
    """Taps of one axis of :func:`resize_cubic_f64` (``n_in`` -> ``n_out`` samples), all in float64: per output sample the index of
    the first of four consecutive samples of the PADDED line (``n_in + 2 * CUBIC_PAD`` coefficients) and their four weights,
    ``(start[n_out] int64, w[n_out, 4] float64)``.  As scipy's NI_ZoomShift does it for ``grid_mode=True``, ``mode='nearest'``, order 3, one
    rounding per step: ``cc = ((o + 0.5) * (n_in / n_out) - 0.5) + 12``, clamped to the padded extent, ``start = floor(cc) - 1``, and with
    ``y = cc - floor(cc)``, ``t = 1 - y``: ``w1 = (y*y*(y-2)*3 + 4) / 6``, ``w2 = (t*t*(t-2)*3 + 4) / 6``, ``w0 = t*t*t / 6``, ``w3 = 1 - w0 - w1 - w2``.
    With this map ``cc`` lies in ``[11.5, n_in + 11.5]`` for every pair of extents, so the four taps stay inside the padded line and scipy's
    re-mapping of edge taps never runs; that is checked all the same (:class:`CubicResampleLimit`), as are the extents (2 ... CUBIC_MAX_EXTENT).
    The C entry ts2d_resample_cubic computes the same table on the host."""
    n_in, n_out = int(n_in), int(n_out)
    if min(n_in, n_out) < 2 or max(n_in, n_out) > CUBIC_MAX_EXTENT:
        raise CubicResampleLimit(f"cubic_axis_taps: extent {n_in} -> {n_out} outside 2 ... {CUBIC_MAX_EXTENT}")
    n_pad = n_in + 2 * CUBIC_PAD
    cc = np.arange(n_out, dtype=np.float64) + 0.5
    cc = cc * (np.float64(n_in) / np.float64(n_out))
    cc = cc - 0.5
    cc = cc + np.float64(CUBIC_PAD)
    cc = np.clip(cc, 0.0, np.float64(n_pad - 1))
    f = np.floor(cc)
    start = f.astype(np.int64) - 1
    if start.min() < 0 or start.max() + 3 > n_pad - 1:
        raise CubicResampleLimit(f"cubic_axis_taps: zoom {n_in} -> {n_out} puts a tap outside the padded line")
    y = cc - f
    t = 1.0 - y
    w = np.empty((n_out, 4), np.float64)
    w[:, 1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 2] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 0] = t * t * t / 6.0
    w[:, 3] = 1.0 - w[:, 0] - w[:, 1] - w[:, 2]
    return start, w


def cubic_prefilter_axis0(c: np.ndarray) -> np.ndarray:
    """scipy's cubic B-spline prefilter (``ni_splines.c: apply_filter``, the initialisation of modes 'nearest' / 'reflect') along axis 0
    of a float64 ``[n, m]`` array, in place and bit for bit, one rounding per product / sum / quotient:
    the gain on every sample; ``c[0]``: ``acc = c[0] + z^n * c[n-1]``, then for i = 1 ... n-1 ``acc += z_i * (c[i] + z^n * c[n-1-i])`` with the
    running product ``z_i`` (``z, z*z, ...``), ``c[0] = acc * (z / (1 - z^n * z^n)) + c[0]``; ``c[i] += z * c[i-1]``; ``c[n-1] *= z / (z - 1)``;
    ``c[i] = z * (c[i+1] - c[i])``.  scipy accumulates ``acc`` IN ``c[0]``, so the last term of the sum (i = n-1, which reads ``c[0]``) sees the
    accumulator and not the sample: that is reproduced here, it is worth 6e-4 of an impulse on a line of 2 and 6e-7 on a padded line of 26."""
    n = c.shape[0]
    z = CUBIC_POLE
    c *= CUBIC_GAIN
    z_n = math.pow(z, float(n))
    c0 = c[0].copy()
    acc = c[0] + z_n * c[n - 1]
    z_i = z
    for i in range(1, n):
        acc = acc + z_i * (c[i] + z_n * (acc if i == n - 1 else c[n - 1 - i]))
        z_i = z_i * z
    c[0] = acc * (z / (1.0 - z_n * z_n)) + c0
    for i in range(1, n):
        c[i] = c[i] + z * c[i - 1]
    c[n - 1] = c[n - 1] * (z / (z - 1.0))
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def cubic_coefficients_f64(img2d: np.ndarray) -> np.ndarray:
    """The float64 B-spline coefficients ``[H + 24, W + 24]`` scipy's zoom interpolates: the plane padded by its edge samples, filtered
    along axis 0 and then along axis 1 (``ndi.spline_filter(np.pad(a, 12, 'edge'), 3, output=float64, mode='nearest')``, bit for bit)."""
    c = np.pad(np.asarray(img2d), CUBIC_PAD, mode='edge').astype(np.float64)
    c = cubic_prefilter_axis0(c)
    return np.ascontiguousarray(cubic_prefilter_axis0(np.ascontiguousarray(c.T)).T)


def resize_cubic_f64(img2d: np.ndarray, new_shape) -> np.ndarray:
    """:func:`resize_like_skimage` with ``order=3`` as a closed form in float64 - nnU-Net's input resample for one float32 plane: pad by 12 edge
    samples, prefilter both axes (:func:`cubic_coefficients_f64`), per output pixel 16 taps in row-major order (row tap outer, column tap
    inner), each ``(c * wy) * wx``, summed left to right from 0, every product and sum rounded to float64 (no FMA), ONE rounding to float32,
    then the clip to the plane's float32 ``[min, max]``.  This is the statement the device entry ts2d_resample_cubic
    (csrc/kernels_resample_in.h) reproduces bit for bit.

    Compared with scipy 1.15.3 (tests/test_resample_cubic_cpu.py: seeded shapes from 8 x 8 to 1000 x 512, up- and down-sampling, N(0,1),
    integer-valued, high-dynamic-range and constant planes): every float32 result is equal bit for bit.  Two things had to be found for
    that, both in the prefilter.  The pole: scipy's binary holds ``sqrt(3.0) - 2.0`` folded by its compiler in extended precision, the
    float64 nearest to the real number, which is two units in the last place away from Python's ``math.sqrt(3.0) - 2.0``.  And the
    boundary sum accumulates in ``c[0]`` (:func:`cubic_prefilter_axis0`).  A scipy built by a compiler that folds the constant differently
    would differ by about one float32 ulp on a few pixels in a million; the CPU test would show it.

    Limits, raised as :class:`CubicResampleLimit`: an extent below 2 or above CUBIC_MAX_EXTENT, a plane with a non-finite sample (scipy
    computes NaN-polluted lines there; the callers hand such a plane to scipy), a tap outside the padded plane (unreachable, see
    :func:`cubic_axis_taps`)."""
    img2d = np.asarray(img2d)
    if img2d.ndim != 2:
        raise CubicResampleLimit(f"resize_cubic_f64: a 2-D plane is needed, got {img2d.ndim} axes")
    sy, wy = cubic_axis_taps(img2d.shape[0], int(new_shape[0]))
    sx, wx = cubic_axis_taps(img2d.shape[1], int(new_shape[1]))
    if not np.isfinite(img2d).all():
        raise CubicResampleLimit("resize_cubic_f64: the plane has a non-finite sample")
    c = cubic_coefficients_f64(img2d)
    r = np.zeros((len(sy), len(sx)), np.float64)
    for i in range(4):
        rows = c[sy + i]
        for j in range(4):
            r = r + (rows[:, sx + j] * wy[:, i, None]) * wx[None, :, j]
    out = r.astype(img2d.dtype)
    lo, hi = img2d.min(), img2d.max()
    out[out < lo] = lo                      # numpy's clip spelled out: a result equal to a bound keeps its own sign of zero
    out[out > hi] = hi
    return out


def cubic_device_entry():
    """``ts2d_resample_cubic`` of the engine library, or None where there is none to call (no library built, or one built before the
    entry existed): the callers then keep the host route, silently - the result is the same."""
    from . import _lib
    try:
        lib = _lib.load()
    except _lib.EngineLibraryError:
        return None
    return getattr(lib, 'ts2d_resample_cubic', None)


def resample_planes_cubic_device(data: np.ndarray, new_hw, device: int) -> Optional[np.ndarray]:
    """All (channel, slice) planes of ``data`` [C, Z, H, W] float32 through ONE ``ts2d_resample_cubic`` call on ``device``: bit for bit
    :func:`resize_cubic_f64`, hence scipy, per plane.  ``data`` may be a :class:`DevicePlanes` that :meth:`DevicePlanes.crop_zscore` or
    :meth:`DevicePlanes.crop_normalize` has normalised: its planes are resampled where they lie.  None when this is no case for the entry - no entry, not float32, an extent outside
    2 ... CUBIC_MAX_EXTENT, a plane with a non-finite sample (its min / max say so) - and the caller runs scipy.  A call that FAILS raises."""
    from . import _lib
    c, z, h, w = data.shape
    oh, ow = int(new_hw[0]), int(new_hw[1])
    if isinstance(data, DevicePlanes):          # normalised on the device: resampled there, with the clip bounds it kept, and downloaded once
        if min(h, w, oh, ow) < 2 or max(h, w, oh, ow) > CUBIC_MAX_EXTENT or c * z * (h + 2 * CUBIC_PAD) * (w + 2 * CUBIC_PAD) > 1 << 28 or c * z * oh * ow > 1 << 28:
            return None
        return data.resample((oh, ow)).download()
    entry = cubic_device_entry()
    if entry is None or data.dtype != np.float32 or c * z < 1 or min(h, w, oh, ow) < 2 or max(h, w, oh, ow) > CUBIC_MAX_EXTENT:
        return None
    if c * z * (h + 2 * CUBIC_PAD) * (w + 2 * CUBIC_PAD) > 1 << 28 or c * z * oh * ow > 1 << 28:
        return None
    src = np.ascontiguousarray(data).reshape(c * z, h, w)
    lo_hi = np.stack([src.min(axis=(1, 2)), src.max(axis=(1, 2))], axis=1).astype(np.float32)
    if not np.isfinite(lo_hi).all():
        return None
    out = np.empty((c, z, oh, ow), np.float32)
    _lib.check(entry(int(device), src.ctypes.data, c * z, h, w, oh, ow, lo_hi.ctypes.data, out.ctypes.data), 'ts2d_resample_cubic')
    return out


def resample_data_to_shape(data: np.ndarray, new_shape, order: int = 3, device: Optional[int] = None) -> np.ndarray:
    """``resample_data_or_seg_to_shape(data, new_shape, current_spacing, new_spacing, is_seg=False, order=3, order_z=0)`` for the
    2-D configurations ts2d uses ([C, 1, H, W] with the 999 pseudo-spacing): upstream finds the 999 axis anisotropic and
    resamples every (channel, slice) in-plane with ``resize``; the slice count does not change [UPSTREAM-RECALL].
    ``device``: index of the GPU that resamples order 3 (:func:`resample_planes_cubic_device`, the same float32 values bit for bit);
    None, another order or a plane outside that entry's limits: scipy on the host."""
    new_shape = tuple(int(v) for v in new_shape)
    if tuple(data.shape[1:]) == new_shape:
        return data
    if data.shape[1] != new_shape[0]:
        raise NotImplementedError(f"resampling along the slice axis ({data.shape[1]} -> {new_shape[0]} slices) is not implemented (2-D configurations only)")
    if device is not None and order == 3:
        out = resample_planes_cubic_device(data, new_shape[1:], device)
        if out is not None:
            return out
    if isinstance(data, DevicePlanes):
        data = data.download()
    out = np.empty((data.shape[0],) + new_shape, dtype=data.dtype)
    for c in range(data.shape[0]):
        for z in range(data.shape[1]):
            out[c, z] = resize_like_skimage(data[c, z], new_shape[1:], order)
    return out


SUM_CHUNK = 8192             # numpy's default buffer size in elements (np.getbufsize()): the run add.reduce hands to its pairwise sum
SUM_LEAF = 128               # numpy's PW_BLOCKSIZE: the longest run summed in eight strided accumulators
PLANES_MAX_SAMPLES = 1 << 28  # samples one device handle takes (ts2d_planes_create)
PLANES_MAX_PLANES = 65535     # ... and planes: the channels x slices of a stack (ts2d_planes_create_stack)


def pairwise_leaves(n: int):
    """The leaves of numpy's pairwise sum over a run of ``n`` elements, ``(offset, length)`` in the order the recursion visits them: a run of
    at most SUM_LEAF elements is a leaf, a longer one splits at ``n2 = n // 2 - (n // 2) % 8``.  The C entry ts2d_planes_crop_zscore walks
    the same recursion for the partial chunk of a plane."""
    out = []

    def walk(off, n):
        if n <= SUM_LEAF:
            out.append((off, n))
        else:
            n2 = n // 2
            n2 -= n2 % 8
            walk(off, n2)
            walk(off + n2, n - n2)
    walk(0, int(n))
    return out


def _leaf_sums_f32(a: np.ndarray, offs: np.ndarray, length: int) -> np.ndarray:
    """The float32 sums of the leaves ``a[o : o + length]``, all of one length: fewer than 8 elements one by one from +0, else eight strided
    accumulators combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the ``length % 8`` last elements one by one."""
    blk = a[offs[:, None] + np.arange(length)[None]]
    if length < 8:
        r = np.zeros(len(offs), np.float32)
        for i in range(length):
            r = r + blk[:, i]
        return r
    m = length - length % 8
    r8 = blk[:, :8].copy()
    for i in range(8, m, 8):
        r8 = r8 + blk[:, i:i + 8]
    r = ((r8[:, 0] + r8[:, 1]) + (r8[:, 2] + r8[:, 3])) + ((r8[:, 4] + r8[:, 5]) + (r8[:, 6] + r8[:, 7]))
    for i in range(m, length):
        r = r + blk[:, i]
    return r


def sum_f32_statement(a: np.ndarray) -> np.float32:
    """``a.sum()`` of a C-contiguous float32 array as numpy 2.2 computes it, written out: the flattened array goes to add.reduce's inner loop in
    chunks of SUM_CHUNK elements; the result starts at +0 (so a sum of -0.0 alone is +0.0) and receives the PAIRWISE sum of each chunk in
    index order (:func:`pairwise_leaves`, the leaves' sums added along the recursion's tree).  A full chunk is 64 leaves of 128 under a
    perfect binary tree.  Every addition is rounded to float32."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    n_full, tail = divmod(a.size, SUM_CHUNK)
    acc = np.float32(0.0)
    with np.errstate(over='ignore', invalid='ignore'):
        if n_full:
            lv = _leaf_sums_f32(a, np.arange(n_full * (SUM_CHUNK // SUM_LEAF), dtype=np.int64) * SUM_LEAF, SUM_LEAF).reshape(n_full, -1)
            while lv.shape[1] > 1:
                lv = lv[:, 0::2] + lv[:, 1::2]
            for v in lv[:, 0]:
                acc = np.float32(acc + v)
        if tail:
            leaves = pairwise_leaves(tail)
            offs = np.array([o for o, _ in leaves], np.int64) + n_full * SUM_CHUNK
            lens = np.array([l for _, l in leaves], np.int64)
            sums = np.empty(len(leaves), np.float32)
            for length in np.unique(lens):
                sel = lens == length
                sums[sel] = _leaf_sums_f32(a, offs[sel], int(length))
            it = iter(sums)

            def fold(n):
                if n <= SUM_LEAF:
                    return next(it)
                n2 = n // 2
                n2 -= n2 % 8
                left = fold(n2)
                return np.float32(left + fold(n - n2))
            acc = np.float32(acc + fold(tail))
    return acc


def zscore_stats_f32_statement(plane: np.ndarray):
    """``(mean, std, divisor)`` of :func:`zscore_f32_statement`, each a float32."""
    x = np.ascontiguousarray(plane, np.float32)
    n = np.float64(x.size)
    with np.errstate(over='ignore', invalid='ignore'):
        mean = np.float32(np.float64(sum_f32_statement(x)) / n)         # numpy: float32 sum / intp count, in float64, rounded once
        d = x - mean
        var = np.float32(np.float64(sum_f32_statement(d * d)) / n)
        std = np.sqrt(var)
    return mean, std, (np.float32(1e-8) if 1e-8 > std else std)         # max(std, 1e-8): the divisor is std unless 1e-8 > std


def zscore_f32_statement(plane: np.ndarray) -> np.ndarray:
    """:func:`zscore` (nnU-Net's ``ZScoreNormalization.run`` without mask) of one C-contiguous float32 plane with numpy's reductions written out,
    bit for bit what numpy 2.2 returns (tests/test_prep_cpu.py: every float32 value over run lengths that cross every branch, N(0,1),
    integer-valued, constant, all-zero and high-dynamic-range planes): ``sum`` = :func:`sum_f32_statement`; ``mean = fl32(f64(sum) / n)``;
    ``d = fl32(x - mean)``; the second sum runs over ``fl32(d * d)``; ``var = fl32(f64(sum) / n)``; ``std = sqrt(var)`` in float32; per element
    ``fl32(d / div)`` with ``div = std`` unless ``1e-8 > std``, then ``float32(1e-8)``.  For n below 2^24 the two float64 quotients equal the
    float32 ones.  What had to be found: numpy sums in chunks of its buffer size, so the pairwise tree never spans more than 8192 elements
    and the chunk sums are added one after the other; and the reduction starts from +0, not from the first element.  This is the statement
    the device entry ts2d_planes_crop_zscore (csrc/kernels_prep.h) reproduces bit for bit."""
    x = np.ascontiguousarray(plane, np.float32)
    mean, _, div = zscore_stats_f32_statement(x)
    with np.errstate(over='ignore', invalid='ignore'):
        return (x - mean) / div


def crop_box_statement(data: np.ndarray):
    """:func:`crop_to_nonzero`'s box for ``[C, 1, H, W]`` data: ``[[0, 1], [r0, r1], [c0, c1]]``, half open, over the pixels that are non-zero in
    any channel; an all-zero image keeps its whole extent.  The device entry ts2d_planes_crop_zscore returns ``(r0, r1, c0, c1)``."""
    c, z, h, w = data.shape
    if z != 1:
        raise ValueError(f"crop_box_statement: one slice per channel is needed, got {z}")
    nz = (data[:, 0] != 0).any(axis=0)
    rows, cols = np.flatnonzero(nz.any(axis=1)), np.flatnonzero(nz.any(axis=0))
    if not len(rows):
        return [[0, 1], [0, h], [0, w]]
    return [[0, 1], [int(rows[0]), int(rows[-1]) + 1], [int(cols[0]), int(cols[-1]) + 1]]


def crop_box3_statement(data: np.ndarray):
    """:func:`crop_to_nonzero`'s box for a stack ``[C, Z, H, W]``: ``[[z0, z1], [r0, r1], [c0, c1]]``, half open, over the voxels that are non-zero in
    any channel (``!= 0``: a NaN counts, ``-0.0`` does not); an all-zero volume keeps its whole extent.  Upstream fills the holes of the mask before it
    takes the box; a hole is enclosed by the mask, so the box of the filled mask is that of the raw one and no filling is needed for it
    (tests/test_stack_cpu.py).  The device entry ts2d_planes_crop_normalize_stack returns ``(z0, z1, r0, r1, c0, c1)``."""
    nz = (np.asarray(data) != 0).any(axis=0)
    if nz.ndim != 3:
        raise ValueError(f"crop_box3_statement: [C, Z, H, W] is needed, got {np.shape(data)}")
    box = []
    for ax in range(3):
        idx = np.flatnonzero(nz.any(axis=tuple(i for i in range(3) if i != ax)))
        box.append([int(idx[0]), int(idx[-1]) + 1] if len(idx) else [0, int(nz.shape[ax])])
    return box


# nnU-Net's default_normalization_schemes -> the TS2D_NORM_* of include/ts2d_engine.h, and the TS2D_PLANES_* status bits of ts2d_planes_crop_normalize
NORM_SCHEME_IDS = {'ZScoreNormalization': 0, 'CTNormalization': 1, 'RescaleTo01Normalization': 2, 'RGBTo01Normalization': 3, 'NoNormalization': 4}
PLANES_NONFINITE, PLANES_RGB_RANGE, PLANES_EMPTY_MASK, PLANES_ZERO_SIGN = 1, 2, 4, 8
PLANES_FILL_ROUNDS = 16      # ts2d_planes_crop_normalize_stack_masked: the hole filling was still adding voxels after FILL_MAX_ROUNDS rounds
FILL_MAX_ROUNDS = 64         # kPrepFillMaxRounds of csrc/kernels_prep_fill.h
RGB_RANGE_MESSAGE = "RGB images are uint 8, for whatever reason I found pixel values outside [0, 255]"


def ct_f32_parameters(props: dict) -> np.ndarray:
    """``(mean, divisor, lower bound, upper bound)`` of :func:`ct_f32_statement`, four float32, from one entry of the plan's
    ``foreground_intensity_properties_per_channel``: ``float32(mean)``; ``float32(max(std, 1e-8))``, the ``max`` taken in double and rounded once;
    the two percentiles as numpy 2.2's ``clip`` converts a Python float or int for a float32 array (NEP 50: to float32, round to nearest) - found
    by letting ``clip`` itself convert them.  A bound float32 cannot hold becomes an infinity (numpy warns of the overflow; silenced here)."""
    with np.errstate(over='ignore'):
        lo = np.clip(np.array([-np.inf], np.float32), props['percentile_00_5'], None)[0]
        hi = np.clip(np.array([np.inf], np.float32), None, props['percentile_99_5'])[0]
        return np.array([np.float32(props['mean']), np.float32(max(props['std'], 1e-8)), lo, hi], np.float32)


def ct_f32_statement(plane: np.ndarray, props: dict) -> np.ndarray:
    """``CTNormalization.run`` (:func:`normalize_channel`) of one float32 plane with numpy's clip written out, bit for bit what numpy 2.2 returns
    (tests/test_prep_schemes_cpu.py): with the parameters of :func:`ct_f32_parameters`, ``x < lo ? lo : x``, then ``x > hi ? hi : x``, then
    ``fl32(fl32(x - mean) / divisor)``.  What clip does at the edges: a NaN SAMPLE stays NaN (both comparisons are false); a sample EQUAL to a
    bound keeps its own bits, so ``-0.0`` against a bound of ``0.0`` stays ``-0.0`` and only a sample really below ``0.0`` becomes ``+0.0`` (``-0.0`` as the
    bound gives ``-0.0``); bounds in the wrong order give the upper one everywhere.  A bound that is not finite in float32: an infinity clips
    nothing on its side, a NaN bound makes every sample NaN (that is the one thing the comparisons do not say: numpy's clip propagates a NaN
    bound).  The device entry ts2d_planes_crop_normalize takes finite parameters only; the caller keeps the host route for the rest."""
    x = np.ascontiguousarray(plane, np.float32)
    mean, div, lo, hi = ct_f32_parameters(props)
    with np.errstate(over='ignore', invalid='ignore'):
        if np.isnan(lo) or np.isnan(hi):
            v = np.full(x.shape, np.nan, np.float32)
        else:
            v = np.where(x < lo, lo, x)
            v = np.where(v > hi, hi, v)
        return (v - mean) / div


def rescale01_f32_statement(plane: np.ndarray) -> np.ndarray:
    """``RescaleTo01Normalization.run`` of one C-contiguous float32 plane, bit for bit numpy 2.2: ``d = fl32(x - min)``, then ``fl32(d / div)`` with
    ``div = max(d)`` unless that is below ``float32(1e-8)``, then ``float32(1e-8)`` (``np.clip`` of a float32 scalar with a Python float bound stays
    float32).  ``x -> fl32(x - min)`` is monotone, so ``max(d) = fl32(max(x) - min(x))``: the device derives the divisor from the plane's two bounds
    and needs no second pass.  A constant plane gives ``d = +0`` everywhere, the divisor 1e-8 and zeros.  ``min`` and ``max`` are exact, but for one
    thing: of a plane whose smallest value is zero and that holds zeros of both signs, numpy's ``min()`` returns ``-0.0`` or ``+0.0`` depending on where
    they lie and how its vector loop runs over them, and ``fl32(-0.0 - min)`` is ``+0.0`` for the one and ``-0.0`` for the other.  This statement takes
    what numpy returns; the device entry reports a minimum of ``-0.0`` (PLANES_ZERO_SIGN) and leaves such a plane to numpy."""
    x = np.ascontiguousarray(plane, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        d = x - x.min()
        mx, lo = d.max(), np.float32(1e-8)
        return d / (lo if mx < lo else mx)


def rgb01_f32_statement(plane: np.ndarray) -> np.ndarray:
    """``RGBTo01Normalization.run`` of one float32 plane: upstream's range check (``min() < 0 or max() > 255`` raises; a NaN passes it, a ``-0.0`` too),
    then ``fl32(x / float32(255))``."""
    x = np.ascontiguousarray(plane, np.float32)
    if x.min() < 0 or x.max() > 255:
        raise RuntimeError(RGB_RANGE_MESSAGE)
    with np.errstate(invalid='ignore'):
        return x / np.float32(255.0)


def masked_zscore_f32_statement(plane: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """``ZScoreNormalization.run`` with ``use_mask_for_norm`` of one float32 plane, bit for bit numpy 2.2: ``img[m]`` is a compact 1-D copy of the
    masked samples in row-major order, so ``img[m].mean()`` and ``img[m].std()`` are :func:`zscore_stats_f32_statement` of a run of ``n_m`` elements
    (chunks of 8192, the pairwise tree of the last ``n_m % 8192``); inside the mask ``fl32(fl32(x - mean) / max(std, 1e-8))``, outside it the sample
    itself.  For the single-slice inputs of the device path the mask is "non-zero in ANY channel" inside the crop box (:func:`crop_to_nonzero`).
    An empty mask (an image of zeros) has no mean: numpy warns and fills NaN; it is no case of this statement, nor of the device."""
    x = np.ascontiguousarray(plane, np.float32).copy()
    m = np.asarray(mask).astype(bool)
    sel = x[m]
    if not sel.size:
        raise ValueError("masked_zscore_f32_statement: the mask is empty")
    mean, _, div = zscore_stats_f32_statement(sel)
    with np.errstate(over='ignore', invalid='ignore'):
        x[m] = (sel - mean) / div
    return x


def fill_holes_sweeps_statement(mask: np.ndarray):
    """``scipy.ndimage.binary_fill_holes(mask)`` (default cross structure) of a boolean volume ``[Z, H, W]`` as the device computes it
    (csrc/kernels_prep_fill.h), ``(filled, rounds)``: ``bg = ~mask``; ``out`` starts as the background voxels on the six faces; a ROUND is six
    directional sweeps in fixed order - z up, z down, y up, y down, x up, x down - each ``out[i] |= bg[i] & out[i -+ 1]`` walked along its axis, each
    seeing the one before; a round that adds nothing ends the loop and is counted.  ``filled = ~out``.  The result does not depend on the order: a
    background voxel stays outside the mask iff it is 6-connected through background to a face, which is scipy's definition, so the bytes are
    scipy's (tests/test_stack_masked_cpu.py) - only ``rounds`` belongs to this order, and they are the device's rounds: 2 ... 7 on head-like masks,
    ``(H - 1) // 2 + 1`` on a one-voxel serpentine corridor of height H.  Applied to the mask INSIDE crop_to_nonzero's box it gives the filled mask of the
    whole array, cropped: every voxel outside the box is background and reaches the array's border in a straight line."""
    mask = np.asarray(mask).astype(bool)
    if mask.ndim != 3:
        raise ValueError(f"fill_holes_sweeps_statement: [Z, H, W] is needed, got {mask.shape}")
    bg = ~mask
    out = np.zeros_like(bg)
    for ax in range(3):
        for at in (0, -1):
            sl = [slice(None)] * 3
            sl[ax] = at
            out[tuple(sl)] = bg[tuple(sl)]
    o, b = [np.moveaxis(out, ax, 0) for ax in range(3)], [np.moveaxis(bg, ax, 0) for ax in range(3)]     # views: axis `ax` first
    rounds = 0
    while True:
        rounds += 1
        before = int(out.sum())
        for ax in range(3):
            n = mask.shape[ax]
            for i in range(1, n):                       # up
                o[ax][i] |= b[ax][i] & o[ax][i - 1]
            for i in range(n - 2, -1, -1):              # down
                o[ax][i] |= b[ax][i] & o[ax][i + 1]
        if int(out.sum()) == before:
            return ~out, rounds


def masked_zscore_stack_statement(vol: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """``ZScoreNormalization.run`` with ``use_mask_for_norm`` of one channel's cropped volume ``[Z, h, w]``: :func:`masked_zscore_f32_statement` over the
    flattened, C-ordered channel - ``img[mask]`` is ONE run of the masked samples in index order, so numpy's chunks of 8192 cross the slices.
    ``mask``: the volume's hole-filled non-zero mask (:func:`fill_holes_sweeps_statement` inside the crop box = :func:`crop_to_nonzero`'s).  This is
    the statement the device entry ts2d_planes_crop_normalize_stack_masked reproduces bit for bit."""
    flat = np.ascontiguousarray(vol, np.float32).reshape(1, -1)
    return masked_zscore_f32_statement(flat, np.asarray(mask).reshape(1, -1)).reshape(np.shape(vol))


def planes_device_entries():
    """The engine library when it has the ``ts2d_planes_*`` entries, or None (no library built, or one built before they existed): the callers
    then keep the host route, silently - the result is the same."""
    from . import _lib
    try:
        lib = _lib.load()
    except _lib.EngineLibraryError:
        return None
    return lib if hasattr(lib, 'ts2d_planes_create') else None


class DevicePlanes:
    """The planes ``[C, 1, h, w]`` float32 of one native 2-D case - with ``stack``, the slices ``[C, Z, h, w]`` of a volume that a 2-D plan takes slice
    by slice (:meth:`crop_normalize_stack`, or :meth:`crop_normalize_stack_masked` with a masked z-score channel, is then the crop entry) - on the device, behind a ``ts2d_planes`` handle: uploaded once here, cropped
    and normalised (:meth:`crop_zscore`, or :meth:`crop_normalize` for the other schemes) and resampled (:meth:`resample`) where they lie, downloaded once (:meth:`download`).  Every float32
    that comes back is the host route's, bit for bit (:func:`zscore_f32_statement` and the statements of the other schemes, :func:`resize_cubic_f64`).  A context manager;
    :meth:`close` destroys the handle and may be called twice."""

    def __init__(self, data: np.ndarray, device: int, lib=None, stack: bool = False):
        import ctypes
        self._lib = lib if lib is not None else planes_device_entries()
        if self._lib is None:
            raise RuntimeError("DevicePlanes: the engine library has no ts2d_planes_* entries")
        data = np.asarray(data)
        if data.ndim != 4 or (data.shape[1] != 1 and not stack) or data.dtype != np.float32:
            raise ValueError(f"DevicePlanes: float32 [C, 1, H, W] is needed, got {data.dtype} {data.shape}")
        src = np.ascontiguousarray(data)
        self.device, self.channels = int(device), int(data.shape[0])
        self.slices = int(data.shape[1])                    # 1, or the slices per channel of a stack (crop_normalize_stack may drop some)
        self.stats = None                                   # [C, 2] float32 (mean, std) after crop_zscore; what crop_normalize used per channel
        self.status = 0                                     # PLANES_* bits of the last crop_normalize
        self._h = ctypes.c_void_p()
        if stack:
            self._check(self._lib.ts2d_planes_create_stack(self.device, src.ctypes.data, self.channels, self.slices, int(data.shape[2]), int(data.shape[3]),
                                                           ctypes.byref(self._h)), 'ts2d_planes_create_stack')
            return
        self._check(self._lib.ts2d_planes_create(self.device, src.ctypes.data, self.channels, int(data.shape[2]), int(data.shape[3]),
                                                 ctypes.byref(self._h)), 'ts2d_planes_create')

    @staticmethod
    def _check(rc, what):
        from . import _lib
        _lib.check(rc, what)

    @property
    def shape(self):
        import ctypes
        h, w = ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.ts2d_planes_extent(self._h, ctypes.byref(h), ctypes.byref(w)), 'ts2d_planes_extent')
        return (self.channels, self.slices, h.value, w.value)

    def crop_zscore(self):
        """crop_to_nonzero and the per-channel z-score on the device.  Returns the box ``[[0, 1], [r0, r1], [c0, c1]]`` the planes now span, or None
        when the device met a non-finite mean, variance or result: nothing usable was normalised and the caller takes the host route."""
        import ctypes
        box, bad = (ctypes.c_int32 * 4)(), ctypes.c_int(0)
        stats = np.zeros((self.channels, 2), np.float32)
        self._check(self._lib.ts2d_planes_crop_zscore(self._h, ctypes.byref(box), stats.ctypes.data, ctypes.byref(bad)), 'ts2d_planes_crop_zscore')
        if bad.value:
            return None
        self.stats = stats
        return [[0, 1], [int(box[0]), int(box[1])], [int(box[2]), int(box[3])]]

    def crop_normalize(self, schemes, use_mask, fip):
        """crop_to_nonzero and each channel's own scheme on the device (ts2d_planes_crop_normalize): ``schemes`` the plan's names, ``use_mask`` its
        ``use_mask_for_norm``, ``fip`` its ``foreground_intensity_properties_per_channel`` (read for the CT channels).  Returns the box like
        :meth:`crop_zscore`, or None with the PLANES_* bits in ``self.status``: nothing usable was normalised and the caller takes the host route."""
        import ctypes
        ids = np.array([NORM_SCHEME_IDS[s] for s in schemes[:self.channels]], np.int32)
        params = np.zeros((self.channels, 4), np.float32)
        for c in np.flatnonzero(ids == NORM_SCHEME_IDS['CTNormalization']):
            params[c] = ct_f32_parameters(fip[str(c)])
        masked = np.array([bool(c < len(use_mask) and use_mask[c]) for c in range(self.channels)], np.uint8)
        box, status = (ctypes.c_int32 * 4)(), ctypes.c_int(0)
        stats = np.zeros((self.channels, 2), np.float32)
        self._check(self._lib.ts2d_planes_crop_normalize(self._h, ids.ctypes.data, params.ctypes.data, masked.ctypes.data, ctypes.byref(box),
                                                         stats.ctypes.data, ctypes.byref(status)), 'ts2d_planes_crop_normalize')
        self.status = int(status.value)
        if self.status:
            return None
        self.stats = stats
        return [[0, 1], [int(box[0]), int(box[1])], [int(box[2]), int(box[3])]]

    def crop_normalize_stack(self, schemes, use_mask, fip, entry='ts2d_planes_crop_normalize_stack'):
        """:meth:`crop_normalize` for a stack (ts2d_planes_crop_normalize_stack): the box over all three axes, each channel normalised with the
        parameters of its WHOLE cropped volume, no masked scheme.  Returns the box ``[[z0, z1], [r0, r1], [c0, c1]]`` the slices now span, or None with
        the PLANES_* bits in ``self.status``.  ``entry``: the symbol to call - :meth:`crop_normalize_stack_masked` passes its own, same arguments."""
        import ctypes
        ids = np.array([NORM_SCHEME_IDS[s] for s in schemes[:self.channels]], np.int32)
        params = np.zeros((self.channels, 4), np.float32)
        for c in np.flatnonzero(ids == NORM_SCHEME_IDS['CTNormalization']):
            params[c] = ct_f32_parameters(fip[str(c)])
        masked = np.array([bool(c < len(use_mask) and use_mask[c]) for c in range(self.channels)], np.uint8)
        box, status = (ctypes.c_int32 * 6)(), ctypes.c_int(0)
        stats = np.zeros((self.channels, 2), np.float32)
        self._check(getattr(self._lib, entry)(self._h, ids.ctypes.data, params.ctypes.data, masked.ctypes.data, ctypes.byref(box),
                                              stats.ctypes.data, ctypes.byref(status)), entry)
        self.status = int(status.value)
        if self.status:
            return None
        self.stats, self.slices = stats, int(box[1]) - int(box[0])
        return [[int(box[0]), int(box[1])], [int(box[2]), int(box[3])], [int(box[4]), int(box[5])]]

    def crop_normalize_stack_masked(self, schemes, use_mask, fip):
        """:meth:`crop_normalize_stack` that takes a masked z-score channel (ts2d_planes_crop_normalize_stack_masked): the non-zero mask of the cropped
        volume is hole-filled in 3-D on the device (:func:`fill_holes_sweeps_statement`) and the channel normalised inside it with the statistics of its
        masked samples (:func:`masked_zscore_stack_statement`).  None with the PLANES_* bits in ``self.status`` - PLANES_EMPTY_MASK and
        PLANES_FILL_ROUNDS among them - as there."""
        return self.crop_normalize_stack(schemes, use_mask, fip, entry='ts2d_planes_crop_normalize_stack_masked')

    def resample(self, hw):
        """Order-3 resample of every plane to ``hw`` on the device, clipped to the bounds :meth:`crop_zscore` left."""
        self._check(self._lib.ts2d_planes_resample_cubic(self._h, int(hw[0]), int(hw[1])), 'ts2d_planes_resample_cubic')
        return self

    def download(self) -> np.ndarray:
        out = np.empty(self.shape, np.float32)
        self._check(self._lib.ts2d_planes_download(self._h, out.ctypes.data), 'ts2d_planes_download')
        return out

    def close(self):
        h, self._h = self._h, None
        if h is not None and h.value is not None:
            self._lib.ts2d_planes_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# C * H * W from which the device route of run_case_npy is taken.  Below it the handle's fixed cost (three allocations, a dozen small copies
# and synchronisations: 0.25 ms) is more than numpy's passes over the planes; measured on two-channel square planes the routes cross between
# 2 x 128^2 (0.89x) and 2 x 192^2 (1.34x) samples (profiles/r12_native2d_case.txt).  The other schemes
# (DevicePlanes.crop_normalize) cross between the same two sizes - 0.78 ... 0.98x and 1.23 ... 1.65x, quartiles within 3 % of the medians
# (profiles/r16_normalize_schemes_case.txt) - so this one gate serves them all.
DEVICE_NORMALIZE_MIN_SAMPLES = 1 << 16


def _device_normalize_applies(data, tf, schemes, use_mask, dz) -> bool:
    """The handle computes nnU-Net's result only for the plain case: identity transpose, one slice per channel, ZScoreNormalization without
    mask on every channel, no z-score from the projection, extents and sample count inside the handle's limits (and above the size from
    which it pays), the entries present."""
    c, z, h, w = data.shape
    return (list(tf) == [0, 1, 2] and z == 1 and c >= 1 and dz is None
            and all(s == 'ZScoreNormalization' for s in schemes[:c]) and len(schemes) >= c and not any(use_mask[:c])
            and 1 <= min(h, w) and max(h, w) <= CUBIC_MAX_EXTENT and DEVICE_NORMALIZE_MIN_SAMPLES <= c * h * w <= PLANES_MAX_SAMPLES
            and planes_device_entries() is not None)


def _ct_parameters_usable(schemes, fip, c) -> bool:
    """Are the plan's intensity properties there for every CT channel of the first ``c``, as Python numbers that are finite in float32?"""
    for i in range(c):
        if schemes[i] == 'CTNormalization':
            props = (fip or {}).get(str(i))
            keys = ('mean', 'std', 'percentile_00_5', 'percentile_99_5')
            if not props or not all(type(props.get(k)) in (int, float) for k in keys):
                return False
            try:
                if not np.isfinite(ct_f32_parameters(props)).all():
                    return False
            except OverflowError:
                return False
    return True


def _device_stack_applies(data, tf, schemes, use_mask, fip) -> bool:
    """The cases ts2d_planes_crop_normalize_stack computes: a stack (more than one slice per channel) under the identity transpose, every scheme one of
    nnU-Net's five and none of them masked (the mask of a volume is hole-filled in 3-D: :func:`_device_stack_masked_applies` and its entry take that), usable CT parameters, extents,
    plane and sample counts inside the handle's limits (and above the size from which it pays), the two stack entries present."""
    c, z, h, w = data.shape
    if not (list(tf) == [0, 1, 2] and z > 1 and c >= 1 and len(schemes) >= c and all(s in NORM_SCHEME_IDS for s in schemes[:c])):
        return False
    if any(schemes[i] == 'ZScoreNormalization' and i < len(use_mask) and use_mask[i] for i in range(c)):
        return False
    if not _ct_parameters_usable(schemes, fip, c):
        return False
    lib = planes_device_entries()
    return (1 <= min(h, w) and max(h, w) <= CUBIC_MAX_EXTENT and c * z <= PLANES_MAX_PLANES
            and DEVICE_NORMALIZE_MIN_SAMPLES <= c * z * h * w <= PLANES_MAX_SAMPLES
            and lib is not None and hasattr(lib, 'ts2d_planes_create_stack') and hasattr(lib, 'ts2d_planes_crop_normalize_stack'))


def _device_stack_masked_applies(data, tf, schemes, use_mask, fip) -> bool:
    """The cases :func:`_device_stack_applies` refuses for a masked channel and ts2d_planes_crop_normalize_stack_masked computes: its other conditions,
    at least one ZScoreNormalization channel with ``use_mask_for_norm``, and that entry present.  Ungated beyond DEVICE_NORMALIZE_MIN_SAMPLES: the
    device route wins at every size measured, 16 x 128 x 128 included (profiles/r22_stack_masked_case.txt)."""
    c, z, h, w = data.shape
    if not (list(tf) == [0, 1, 2] and z > 1 and c >= 1 and len(schemes) >= c and all(s in NORM_SCHEME_IDS for s in schemes[:c])):
        return False
    if not any(schemes[i] == 'ZScoreNormalization' and i < len(use_mask) and use_mask[i] for i in range(c)):
        return False
    if not _ct_parameters_usable(schemes, fip, c):
        return False
    lib = planes_device_entries()
    return (1 <= min(h, w) and max(h, w) <= CUBIC_MAX_EXTENT and c * z <= PLANES_MAX_PLANES
            and DEVICE_NORMALIZE_MIN_SAMPLES <= c * z * h * w <= PLANES_MAX_SAMPLES
            and lib is not None and hasattr(lib, 'ts2d_planes_create_stack') and hasattr(lib, 'ts2d_planes_crop_normalize_stack_masked'))


def _device_schemes_apply(data, tf, schemes, use_mask, fip) -> bool:
    """The cases :func:`_device_normalize_applies` refuses for their schemes and ts2d_planes_crop_normalize computes: identity transpose, one slice
    per channel, every scheme one of nnU-Net's five and not all of them the plain z-score (that case belongs to the other predicate, its z-score
    from the projection included - which can never apply here, so it does not bar this route), the plan's intensity properties there for every CT
    channel as Python numbers that are finite in float32, extents and sample count inside the handle's limits (and above the size from which it
    pays), the entry present."""
    c, z, h, w = data.shape
    if not (list(tf) == [0, 1, 2] and z == 1 and c >= 1 and len(schemes) >= c and all(s in NORM_SCHEME_IDS for s in schemes[:c])):
        return False
    masked = [bool(i < len(use_mask) and use_mask[i]) for i in range(c)]
    if all(s == 'ZScoreNormalization' for s in schemes[:c]) and not any(masked):
        return False
    if not _ct_parameters_usable(schemes, fip, c):
        return False
    lib = planes_device_entries()
    return (1 <= min(h, w) and max(h, w) <= CUBIC_MAX_EXTENT and DEVICE_NORMALIZE_MIN_SAMPLES <= c * h * w <= PLANES_MAX_SAMPLES
            and lib is not None and hasattr(lib, 'ts2d_planes_crop_normalize'))


def _device_zscore_applies(dz, data, bbox, tf, schemes, use_mask) -> bool:
    """The device result is nnU-Net's result only if nothing sits between projection and normalisation: identity transpose,
    crop-to-nonzero = whole image (checked on both sides: the device's non-zero box and the host's bbox), plain z-score on
    every channel, one channel per projection."""
    nz, nx = dz['shape']
    return (list(tf) == [0, 1, 2] and data.shape[1:] == (1, nz, nx) and len(dz['order']) == data.shape[0]
            and tuple(dz['box']) == (0, nz - 1, 0, nx - 1) and [list(b) for b in bbox] == [[0, 1], [0, nz], [0, nx]]
            and all(s == 'ZScoreNormalization' for s in schemes[:data.shape[0]]) and not any(use_mask[:data.shape[0]]))


class DefaultPreprocessor:
    def __init__(self, verbose: bool = True):
        self.verbose = verbose

    def run_case_npy(self, data: np.ndarray, seg, properties: dict, plans_manager, configuration_manager, dataset_json):
        data = data.astype(np.float32)
        tf = list(getattr(plans_manager, 'transpose_forward', [0, 1, 2]))
        data = data.transpose([0] + [i + 1 for i in tf])
        original_spacing = [properties['spacing'][i] for i in tf]
        properties['shape_before_cropping'] = data.shape[1:]
        schemes = getattr(configuration_manager, 'normalization_schemes', None) or ['ZScoreNormalization'] * data.shape[0]
        use_mask = getattr(configuration_manager, 'use_mask_for_norm', None) or [False] * data.shape[0]
        dz = properties.pop('device_zscore', None)
        device_resample = properties.pop('device_resample', None)     # GPU index for the order-3 resample below (HIPModel sets it), None: host
        device_normalize = properties.pop('device_normalize', None)   # GPU index for crop box + z-score (+ that resample) on device-resident planes
        device_schemes = properties.pop('device_normalize_schemes', None)   # the same for the cases that route refuses for their schemes: masked z-score, CT, Rescale, RGB, none
        device_stack = properties.pop('device_normalize_stack', None)       # the same for a stack [C, Z, H, W], Z > 1, under a 2-D plan: box over three axes, statistics of the whole volume, no masked scheme
        device_stack_masked = properties.pop('device_normalize_stack_masked', None)   # ... and for a stack with a masked z-score channel: the 3-D hole filling of the mask, the statistics of the masked samples
        target_spacing = list(configuration_manager.spacing)
        if len(target_spacing) < len(data.shape[1:]):
            target_spacing = [original_spacing[0]] + target_spacing
        fip = (getattr(plans_manager, 'plans', None) or {}).get('foreground_intensity_properties_per_channel', {})
        planes_device = None
        if device_normalize is not None and _device_normalize_applies(data, tf, schemes, use_mask, dz):
            planes_device, plain = device_normalize, True
        elif device_schemes is not None and _device_schemes_apply(data, tf, schemes, use_mask, fip):
            planes_device, plain = device_schemes, False
        stack_device = None
        if device_stack is not None and len(configuration_manager.spacing) == 2 and _device_stack_applies(data, tf, schemes, use_mask, fip):
            stack_device, stack_masked = device_stack, False
        elif device_stack_masked is not None and len(configuration_manager.spacing) == 2 and _device_stack_masked_applies(data, tf, schemes, use_mask, fip):
            stack_device, stack_masked = device_stack_masked, True
        if stack_device is not None:
            with DevicePlanes(data, stack_device, stack=True) as planes:
                bbox = planes.crop_normalize_stack_masked(schemes, use_mask, fip) if stack_masked else planes.crop_normalize_stack(schemes, use_mask, fip)
                if bbox is not None:            # (None: a status bit - numpy below computes, or raises, what numpy does)
                    properties['bbox_used_for_cropping'] = bbox
                    shape = properties['shape_after_cropping_and_before_resampling'] = planes.shape[1:]
                    new_shape = [int(round(i / j * k)) for i, j, k in zip(original_spacing, target_spacing, shape)]
                    if list(new_shape) != list(shape):
                        return resample_data_to_shape(planes, new_shape, order=3, device=device_resample), None, properties
                    return planes.download(), None, properties
        if planes_device is not None:
            with DevicePlanes(data, planes_device) as planes:
                bbox = planes.crop_zscore() if plain else planes.crop_normalize(schemes, use_mask, fip)
                if bbox is not None:            # (None: a non-finite sample or sum, an RGB sample out of range, an empty mask - numpy below computes, or raises, what numpy does)
                    properties['bbox_used_for_cropping'] = bbox
                    shape = properties['shape_after_cropping_and_before_resampling'] = planes.shape[1:]
                    new_shape = [int(round(i / j * k)) for i, j, k in zip(original_spacing, target_spacing, shape)]
                    if list(new_shape) != list(shape):
                        return resample_data_to_shape(planes, new_shape, order=3, device=device_resample), None, properties
                    return planes.download(), None, properties
        data, bbox, nzmask = crop_to_nonzero(data, return_mask=True)
        properties['bbox_used_for_cropping'] = bbox
        properties['shape_after_cropping_and_before_resampling'] = data.shape[1:]
        new_shape = [int(round(i / j * k)) for i, j, k in zip(original_spacing, target_spacing, data.shape[1:])]
        if dz is not None and not _device_zscore_applies(dz, data, bbox, tf, schemes, use_mask):
            dz = None
        for c in range(data.shape[0]):
            if dz is not None:          # normalised on the device behind the projection (ts2d_project_coronal_zscore): no host pass
                data[c, 0] = dz['norm'][dz['order'][c]]
                continue
            data[c] = normalize_channel(data[c], schemes[c], bool(c < len(use_mask) and use_mask[c]), nzmask, fip.get(str(c)))
        if list(new_shape) != list(data.shape[1:]):       # the plan's spacing differs from the image's: resample (order 3), AFTER normalising
            data = resample_data_to_shape(data, new_shape, order=3, device=device_resample)
        return data, None, properties

    def run_case(self, image_files: List[str], seg_file: Optional[str], plans_manager, configuration_manager, dataset_json):
        if isinstance(image_files, str):
            image_files = [image_files]
        data, props = read_images(image_files)
        return self.run_case_npy(data, None, props, plans_manager, configuration_manager, dataset_json)
