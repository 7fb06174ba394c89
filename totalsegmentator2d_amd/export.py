"""Output side of the hot path: logits -> segmentation image.

Reference: ``export_prediction_from_logits(prediction, data_properties, configuration_manager, plans_manager, dataset_json,
ofile_truncated, save_probabilities)`` called at ``ts2d/core/inference/prediction_worker.py:215-221`` (third-party
nnunetv2ml fork: multilabel => ``sigmoid(logits.float()) > 0.5`` per channel), followed by the metadata restamp
``set_annotation_meta(img, labels, colors)`` at ``prediction_worker.py:226-240``.  Here both happen in memory; the
file is written once.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import nrrd
from .image import set_annotation_meta

SIGMOID_HALF_THRESHOLD = np.float32(1.5 * 2.0 ** -24)     # sigmoid(float32 x) > 0.5  <=>  x > 1.5 * 2^-24 (tests/test_oracle.py)


def needs_logits(properties: dict, shape_khw) -> bool:
    """Does the export resample the prediction back to another shape (then it needs logits, not a thresholded segmentation)?"""
    return tuple(properties.get('shape_after_cropping_and_before_resampling', tuple(shape_khw))) != tuple(shape_khw)


def labelmap_statement(logits_f16, rect, out_hw) -> np.ndarray:
    """The numpy statement of the device label-map export (csrc/kernels_labelmap.h; C-ABI ts2d_ensemble_predict_tiled_labelmap and
    ts2d_labelmap_from_logits): the rectangle ``rect = (y, x, h, w)`` of the aggregated half logits [K, Hp, Wp] widened to float32,
    every plane resampled to ``out_hw`` by :func:`preprocess.resize_linear_f64` (bit for bit scipy's order-1 zoom, the export's
    ``resampling_fn_probabilities``) - NOT where ``out_hw == (h, w)``: the host route does not resample there, so an infinite logit stays
    infinite instead of meeting a zero weight - and numpy's argmax over the heads: the first index of the maximum, +0 == -0, the first
    NaN wins.  uint8 [out_h, out_w].  It is the host route of the export byte for byte (tests/test_labelmap_cpu.py) wherever no SOURCE sample
    is NaN: skimage's clip to the plane's [min, max] makes such a plane NaN as a whole there; the engine refuses NaN logits long before
    the export (ts2d_engine_check), so that no such plane arrives."""
    from .preprocess import resize_linear_f64
    y, x, h, w = (int(v) for v in rect)
    out_hw = tuple(int(v) for v in out_hw)
    lg = np.asarray(logits_f16)[:, y:y + h, x:x + w].astype(np.float32)
    if out_hw != (h, w):
        lg = np.stack([resize_linear_f64(pl, out_hw) for pl in lg])
    return lg.argmax(0).astype(np.uint8)


def paint_regions(above, class_order) -> np.ndarray:
    """nnU-Net's ``convert_probabilities_to_segmentation`` of a region-based model [UPSTREAM-RECALL], on the thresholded heads
    ``above`` [K, ...] (bool: ``sigmoid(logit) > 0.5``): ``seg = 0; for i, c in enumerate(regions_class_order): seg[above[i]] = c`` -
    the highest head above one half decides a pixel; class values may repeat and may be 0.  uint8 [...]."""
    above = np.asarray(above)
    if len(class_order) != above.shape[0]:
        raise ValueError(f"regions_class_order has {len(class_order)} entries, the prediction {above.shape[0]} heads")
    seg = np.zeros(above.shape[1:], dtype=np.uint8)
    for i, c in enumerate(class_order):
        seg[above[i]] = c
    return seg


def regions_statement(logits_f16, rect, out_hw, class_order) -> np.ndarray:
    """The numpy statement of the device export of a REGION-BASED model (csrc/kernels_regions.h; C-ABI
    ts2d_ensemble_predict_tiled_regions and ts2d_regions_from_logits): the rectangle ``rect = (y, x, h, w)`` of the aggregated half
    logits [K, Hp, Wp] widened to float32, every plane resampled to ``out_hw`` by :func:`preprocess.resize_linear_f64` - NOT where
    ``out_hw == (h, w)``, as in :func:`labelmap_statement` - then the export's predicate ``sigmoid(float32 v) > 0.5``, that is
    ``v > SIGMOID_HALF_THRESHOLD`` (NaN is not above it, +inf is), and :func:`paint_regions` in ``class_order``.  uint8 [out_h, out_w]."""
    from .preprocess import resize_linear_f64
    y, x, h, w = (int(v) for v in rect)
    out_hw = tuple(int(v) for v in out_hw)
    lg = np.asarray(logits_f16)[:, y:y + h, x:x + w].astype(np.float32)
    if out_hw != (h, w):
        with np.errstate(invalid='ignore'):          # (a zero weight on an infinite sample: NaN, not painted)
            lg = np.stack([resize_linear_f64(pl, out_hw) for pl in lg])
    return paint_regions(lg > SIGMOID_HALF_THRESHOLD, class_order)


PROBABILITY_MODES = ('multilabel', 'labelmap', 'regions')      # in the order of TS2D_PROB_* (include/ts2d_engine.h)


def inference_nonlinearity(lg32, softmax: bool) -> np.ndarray:
    """nnU-Net's inference non-linearity on float32 logits [K, ...] [UPSTREAM-RECALL: LabelManager.apply_inference_nonlin on
    ``logits.float()``]: the softmax over the heads for a label-map model, else the sigmoid per head, in float32 numpy.  A NaN logit
    gives NaN; the softmax of a pixel with a +inf or NaN head is NaN in every head (inf - inf) and a -inf head gives 0 - what
    ``torch.softmax`` does on the CPU.  Every sum, difference and quotient is float32; ``exp`` is the float64 function rounded once to
    float32, as on the device (csrc/kernels_prob.h: pr_exp): numpy's own float32 ``exp`` is a whole unit off on some arguments, enough
    for ``sigmoid(2^-23) > 0.5`` to come out false, and the probabilities must never contradict the segmentation decided on the logit."""
    v = np.asarray(lg32, dtype=np.float32)

    def exp32(x):
        return np.exp(x.astype(np.float64)).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        if softmax:
            e = exp32(v - v.max(0, keepdims=True))
            return (e / e.sum(0, keepdims=True, dtype=np.float32)).astype(np.float32)
        return (np.float32(1) / (np.float32(1) + exp32(-v))).astype(np.float32)


def fill_probabilities(prob, full_shape, slices, softmax: bool) -> np.ndarray:
    """Upstream's ``revert_cropping_on_probabilities`` [UPSTREAM-RECALL]: ``prob`` [K, ...] placed at ``slices`` of a float32
    [K, *full_shape] whose rest is 0 - except head 0 of a label-map model (``softmax``), which is 1: background is certain there."""
    out = np.zeros((prob.shape[0],) + tuple(int(v) for v in full_shape), dtype=np.float32)
    if softmax:
        out[0] = 1
    out[(slice(None),) + tuple(slices)] = prob
    return out


def probabilities_statement(logits_f16, rect, out_hw, full_hw, box_yx, mode) -> np.ndarray:
    """The numpy statement of the device's probabilities (csrc/kernels_prob.h; C-ABI ts2d_ensemble_predict_tiled_probabilities and
    ts2d_probabilities_from_logits): the rectangle ``rect = (y, x, h, w)`` of the aggregated half logits [K, Hp, Wp] widened to float32,
    every plane resampled to ``out_hw`` by :func:`preprocess.resize_linear_f64` - NOT where ``out_hw == (h, w)``, as in
    :func:`labelmap_statement` - then :func:`inference_nonlinearity` (``mode`` of :data:`PROBABILITY_MODES`: the softmax for 'labelmap',
    else the sigmoid) and :func:`fill_probabilities` into ``full_hw`` with the rectangle at ``box_yx``.  float32 [K, full_h, full_w].
    The resampled logits are the device's bit for bit; the probabilities are not (another ``exp``): both lie within a few float32 units
    of the exact value (tests/test_probabilities_cpu.py, tests/test_gpu_probabilities.py)."""
    from .preprocess import resize_linear_f64
    if mode not in PROBABILITY_MODES:
        raise ValueError(f"mode must be one of {PROBABILITY_MODES}, found {mode!r}")
    y, x, h, w = (int(v) for v in rect)
    out_hw = tuple(int(v) for v in out_hw)
    by, bx = (int(v) for v in box_yx)
    lg = np.asarray(logits_f16)[:, y:y + h, x:x + w].astype(np.float32)
    if out_hw != (h, w):
        with np.errstate(invalid='ignore'):          # (a zero weight on an infinite sample: NaN)
            lg = np.stack([resize_linear_f64(pl, out_hw) for pl in lg])
    softmax = mode == 'labelmap'
    return fill_probabilities(inference_nonlinearity(lg, softmax), full_hw, (slice(by, by + out_hw[0]), slice(bx, bx + out_hw[1])), softmax)


def stack_probabilities_statement(logits_f16, rect, out_hw, full_shape, box, mode) -> np.ndarray:
    """The numpy statement of the device's probabilities of a SLICE STACK (C-ABI ts2d_ensemble_predict_tiled_probabilities_stack under
    HIPnnUNetPredictor.predict_stack_probabilities_from_preprocessed_data): ``logits_f16`` [K, Z, Hp, Wp], :func:`probabilities_statement`
    of every slice - ``rect``, ``out_hw`` and the in-plane part of ``full_shape`` = (Z0, H0, W0) and ``box`` = (z0, y0, x0) are the same
    for all of them - placed at slice ``z0 + z`` of a float32 [K, Z0, H0, W0] whose other slices hold the fill of
    :func:`fill_probabilities`.  Bit for bit the host route of a stack (``convert_...(return_probabilities=True)``, which resamples per
    slice: tests/test_stack_probabilities_cpu.py)."""
    lg = np.asarray(logits_f16)
    Z0, z0 = int(full_shape[0]), int(box[0])
    planes = np.stack([probabilities_statement(lg[:, z], rect, out_hw, full_shape[1:], box[1:], mode) for z in range(lg.shape[1])], axis=1)
    return fill_probabilities(planes, (Z0,) + planes.shape[2:], (slice(z0, z0 + lg.shape[1]), slice(None), slice(None)), mode == 'labelmap')


def convert_predicted_logits_to_segmentation_with_correct_shape(logits, properties: dict, multilabel: bool = True,
                                                                transpose_backward=(0, 1, 2), regions=None,
                                                                return_probabilities: bool = False, probabilities=None):
    """[K, Z, H, W] logits (any float dtype) -> uint8 segmentation in the ORIGINAL (pre-crop) array shape:
    multilabel: [K, Z0, H0, W0] of {0,1}; otherwise a label map [Z0, H0, W0] - the argmax over the heads or, with ``regions`` (the
    ``regions_class_order`` of a region-based model, one class value per head), ``sigmoid > 0.5`` per head painted in that order.
    Upstream first resamples the logits back to
    ``properties['shape_after_cropping_and_before_resampling']`` (``resampling_fn_probabilities``: order 1, per slice for the 2-D
    configurations [UPSTREAM-RECALL]) - a no-op when the plan's spacing is the image's.
    ``return_probabilities``: ``(segmentation, probabilities)`` - the host route of ``save_probabilities``: the inference non-linearity
    in float32 on the resampled logits (:func:`inference_nonlinearity`: sigmoid, or softmax for a label-map model), the crop reverted
    on them (:func:`fill_probabilities`) and ``transpose_backward`` applied: float32 [K, Z0, H0, W0] [UPSTREAM-RECALL].  It needs the
    logits; the segmentation is decided on them exactly as without the flag.
    ``probabilities`` (with ``return_probabilities``): the device has done all of it (HIPnnUNetPredictor.
    predict_probabilities_from_preprocessed_data) - ``logits`` is then its decided uint8 map and ``probabilities`` its float32
    [K, Z0, H0, W0], both already in the PRE-CROP shape: only ``transpose_backward`` is left."""
    lg = np.asarray(logits)
    if probabilities is not None:
        if not return_probabilities or lg.dtype != np.uint8:
            raise ValueError("device probabilities come with return_probabilities and the decided uint8 map")
        seg = lg if multilabel else lg[0]
        tb = list(transpose_backward)
        return ((seg.transpose([0] + [i + 1 for i in tb]) if multilabel else seg.transpose(tb)),
                np.asarray(probabilities, dtype=np.float32).transpose([0] + [i + 1 for i in tb]))
    if return_probabilities and lg.dtype == np.uint8:
        raise ValueError("probabilities need the logits, found an already decided uint8 prediction")
    tgt = tuple(properties.get('shape_after_cropping_and_before_resampling', lg.shape[1:]))
    if tuple(lg.shape[1:]) != tgt:
        from .preprocess import resample_data_to_shape
        lg = resample_data_to_shape(lg.astype(np.float32), tgt, order=1)
    shape0 = tuple(properties['shape_before_cropping'])
    bbox = properties['bbox_used_for_cropping']
    sl = tuple(slice(b[0], b[1]) for b in bbox)
    if multilabel:
        if lg.dtype == np.uint8:
            seg = lg          # already thresholded on the device (HIPnnUNetPredictor.predict_segmentation_from_preprocessed_data): same predicate
        elif lg.dtype == np.float16:
            # float32(x) > 1.5 * 2^-24 on the fp16 bit pattern: positive, at least the SECOND subnormal (the first, 2^-24, is
            # below the threshold), +inf included, NaN excluded - the same predicate without a float32 copy of the array
            v = np.ascontiguousarray(lg).view(np.uint16)
            seg = ((v >= np.uint16(2)) & (v <= np.uint16(0x7C00))).view(np.uint8)
        else:
            seg = (lg.astype(np.float32) > SIGMOID_HALF_THRESHOLD).astype(np.uint8)
        out = np.zeros((lg.shape[0],) + shape0, dtype=np.uint8)
        out[(slice(None),) + sl] = seg
        out = out.transpose([0] + [i + 1 for i in transpose_backward])
        return (out, _host_probabilities(lg, shape0, sl, False, transpose_backward)) if return_probabilities else out
    if lg.dtype == np.uint8:
        # already resampled and decided on the device (HIPnnUNetPredictor.predict_labelmap_from_preprocessed_data): ONE plane of labels,
        # the argmax of a label-map model or the painted regions of a region-based one
        if lg.shape[0] != 1:
            raise ValueError(f"a uint8 prediction of a label-map model is one plane of labels, found {lg.shape[0]}")
        seg = lg[0]
    elif regions is not None:
        # [UPSTREAM-RECALL] the sigmoid in float32, > 0.5, the painting loop: on the host for whatever the device did not decide
        seg = paint_regions(lg.astype(np.float32) > SIGMOID_HALF_THRESHOLD, regions)
    else:
        seg = lg.astype(np.float32).argmax(0).astype(np.uint8)
    out = np.zeros(shape0, dtype=np.uint8)
    out[sl] = seg
    out = out.transpose(list(transpose_backward))
    return (out, _host_probabilities(lg, shape0, sl, regions is None, transpose_backward)) if return_probabilities else out


def _host_probabilities(lg, shape0, sl, softmax: bool, transpose_backward) -> np.ndarray:
    """The probabilities of the host route: the (resampled) logits ``lg`` [K, Z, H, W] in float32 through the non-linearity, the crop
    reverted, ``transpose_backward`` applied."""
    prob = fill_probabilities(inference_nonlinearity(lg.astype(np.float32), softmax), shape0, sl, softmax)
    return prob.transpose([0] + [i + 1 for i in transpose_backward])


def segmentation_to_image(seg: np.ndarray, ref: nrrd.Image, multilabel: bool, labels: Optional[Dict[int, str]] = None,
                          colors: Optional[dict] = None) -> nrrd.Image:
    """uint8 array from :func:`convert_...` -> image with the geometry of the (2-D) input image `ref` and Slicer metadata."""
    if multilabel:
        arr = np.moveaxis(seg, 0, -1)                  # [Z, H, W, K]
        if ref.dimension == 2:
            arr = arr[0]                               # [H, W, K]
        # (the interleaved [.., K] VIEW of the plane-major array: scattering K x H x W bytes at stride K costs 3 ms per sub-model of a
        #  644 x 337 case; consumers index it like sitk's vector image, nrrd.write serialises the logical order)
        img = nrrd.Image(arr, ref.spacing, ref.origin, ref.direction, seg.shape[0], {}, ref.space)
    else:
        arr = seg[0] if ref.dimension == 2 else seg
        img = nrrd.Image(np.ascontiguousarray(arr), ref.spacing, ref.origin, ref.direction, 1, {}, ref.space)
    if labels or colors:
        set_annotation_meta(img, {int(k): v for k, v in (labels or {}).items()}, colors)
    return img


def export_prediction_from_logits(logits, properties: dict, configuration_manager, plans_manager, dataset_json: dict,
                                  ofile_truncated: str, save_probabilities: bool = False, ref_image: Optional[nrrd.Image] = None,
                                  labels: Optional[Dict[int, str]] = None, colors: Optional[dict] = None,
                                  probabilities=None, postprocess=None) -> nrrd.Image:
    """``postprocess``: None, or a callable ``seg -> (seg, stats, route)`` (a closure over ``postprocess.apply_postprocessing``, HIPModel._run)
    applied to the decided label map in its ORIGINAL extent, after the crop has been reverted and ``transpose_backward`` applied and before it
    becomes an image [UPSTREAM-RECALL: the stored postprocessing runs on the written label maps]; the probabilities stay as they are.  The
    returned image then carries ``img.postprocessing = {'route': ..., 'stats': ..., 'seconds': the span of the step alone}``.  A multilabel model has no such step (ValueError).
    ``save_probabilities`` [UPSTREAM-RECALL: export_prediction_from_logits]: beside the segmentation ``<ofile>.npz``
    (``np.savez_compressed``, key ``probabilities``: float32 [K, *original shape]) and ``<ofile>.pkl`` (the case's properties) are
    written; the returned image carries the array as ``img.probabilities`` (the one thing a caller without an output file gets).
    ``probabilities``: the device's array, ``logits`` then being its decided map (see :func:`convert_...`)."""
    from .labels import label_convention
    conv = label_convention(dataset_json)
    multilabel = conv.kind == 'multilabel'
    tb = getattr(plans_manager, 'transpose_backward', [0, 1, 2])
    prob = None
    if save_probabilities:
        seg, prob = convert_predicted_logits_to_segmentation_with_correct_shape(logits, properties, multilabel, tb, regions=conv.class_order,
                                                                                return_probabilities=True, probabilities=probabilities)
    else:
        seg = convert_predicted_logits_to_segmentation_with_correct_shape(logits, properties, multilabel, tb, regions=conv.class_order)
    post = None
    if postprocess is not None:
        if multilabel:
            raise ValueError("postprocessing is defined for label-map and region-based models, not for a multilabel model")
        import time
        t0 = time.perf_counter()
        seg, stats, route = postprocess(seg)
        post = {'route': route, 'stats': stats, 'seconds': time.perf_counter() - t0}
    if ref_image is None:
        ref_image = nrrd.read(properties['sitk_stuff']['files'][0])
    img = segmentation_to_image(seg, ref_image, multilabel, labels, colors)
    if prob is not None:
        img.probabilities = prob
    if post is not None:
        img.postprocessing = post
    if ofile_truncated:
        nrrd.write(img, ofile_truncated + dataset_json.get('file_ending', '.nrrd'), True)
        if prob is not None:
            import pickle
            np.savez_compressed(ofile_truncated + '.npz', probabilities=prob)
            with open(ofile_truncated + '.pkl', 'wb') as f:
                pickle.dump(properties, f)
    return img
