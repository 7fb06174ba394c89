"""``HIPnnUNetPredictor`` - the drop-in for the duck-typed predictor the reference worker consumes.

The reference accepts any object whose type name contains ``nnUNetPredictor`` (or a zero-argument callable returning
one): ``ts2d/core/inference/prediction_worker.py:103-114``.  The members it touches are mirrored here with the same
names and argument meaning:

* ``.configuration_manager.patch_size`` / ``.spacing`` / ``.preprocessor_class(verbose=)``  (prediction_worker.py:76-77,194)
* ``.dataset_json`` (``channel_names``, ``file_ending``, ``labels``)                           (prediction_worker.py:78,180,230)
* ``.plans_manager``, ``.verbose``, ``.device.type``                                         (prediction_worker.py:194-207)
* ``.predict_logits_from_preprocessed_data(data[C,1,H,W]) -> Tensor[K,1,H,W]`` with ``.cpu()`` (prediction_worker.py:206-209)
* ``initialize_from_trained_model_folder(model_dir, folds, checkpoint_name)``                (nnu.py:165)
* ctor kwargs ``tile_step_size, use_mirroring, verbose, allow_tqdm, device, perform_everything_on_device`` (nnu.py:152-163)

What changes underneath: ``network(x)`` is the HIP engine (C-ABI, include/ts2d_engine.h); all tiles x mirror variants
of a case are submitted as ONE batch instead of B=1 calls; the Gaussian/fp16 aggregation follows upstream bit for
bit (float16 accumulators) so that end-of-pipeline logits are comparable with the reference's.
"""
from __future__ import annotations

import json
import os
import re
from types import SimpleNamespace
from typing import List, Optional, Sequence

import numpy as np

from . import sliding_window as sw
from .arch import UNetArch


def fold_mean_f16(folds) -> np.ndarray:
    """The fold ensemble's mean as upstream's ``predict_logits_from_preprocessed_data`` takes it (``prediction += fold`` per fold, then
    ``prediction /= n`` when n > 1), in the float16 of the aggregated logits: numpy's half ``+`` and ``/`` are the fp32 operation
    rounded to nearest even - what the device kernel sw_fold_mean computes, bit for bit (csrc/kernels_fold.h)."""
    folds = [np.asarray(f, dtype=np.float16) for f in folds]
    pred = folds[0]
    for p in folds[1:]:
        pred = pred + p
    if len(folds) > 1:
        pred = pred / np.float16(len(folds))
    return pred


def _to_numpy(data) -> np.ndarray:
    """torch tensor or array-like in -> float32 numpy."""
    return np.asarray(data.detach().cpu().numpy() if hasattr(data, 'detach') else data, dtype=np.float32)


def _to_torch(a: np.ndarray):
    """numpy out -> torch CPU tensor when torch is importable (so that the caller's ``.cpu()`` works), else the array."""
    try:
        import torch
        return torch.from_numpy(np.ascontiguousarray(a))
    except ImportError:
        return a


class _Device:
    """``torch.device``-like (``.type``) without importing torch."""
    def __init__(self, index: int):
        self.type, self.index = 'cuda', index

    def __repr__(self):
        return f"device(type='cuda', index={self.index})"


class HIPnnUNetPredictor:
    def __init__(self, tile_step_size: float = 0.5, use_gaussian: bool = True, use_mirroring: bool = True,
                 perform_everything_on_device: bool = True, device=None, verbose: bool = False,
                 verbose_preprocessing: bool = False, allow_tqdm: bool = True, max_batch: int = 64, precision: str = 'split',
                 tile_dtype: Optional[str] = None):
        """``tile_dtype``: dtype of a tile prediction when it is blended into upstream's float16 buffers - 'float' (the
        reference's CPU path, taken when ``torch.cuda.is_available()`` is false, ``nnu.py:161-163``: fp32 tile x half gaussian in
        fp32, ONE rounding per ``logits[sl] += p``) or 'half' (the reference's CUDA path under fp16 autocast: the tile is half, the
        product and the sum each round to half).  Default (None): the blend order of the reference path the chosen arithmetic
        mirrors - 'float' for the fp32-parity modes ('split', 'exact': BASELINE.json compares with the CPU path), 'half' for
        ``precision='f16'`` (the autocast-like mode).
        (The network is always the HIP engine: the numpy restatement of the tiling / aggregation that the CPU tests use lives in
        tests/host_predictor.py, a subclass - nothing in this module can route around the engine.)"""
        self.tile_step_size = tile_step_size
        self.use_gaussian = use_gaussian
        self.use_mirroring = use_mirroring
        self.perform_everything_on_device = perform_everything_on_device
        self.verbose = verbose
        self.verbose_preprocessing = verbose_preprocessing
        self.allow_tqdm = allow_tqdm
        self.max_batch = int(max_batch)
        if precision not in ('split', 'exact', 'f16'):
            raise ValueError("precision must be 'split' (fp32-equivalent, default), 'exact' (fp32 MFMA) or 'f16' (like the reference's CUDA autocast path)")
        self.precision = precision
        if tile_dtype is None:
            tile_dtype = 'half' if precision == 'f16' else 'float'
        if tile_dtype not in ('float', 'half'):
            raise ValueError("tile_dtype must be 'float' (reference CPU path), 'half' (CUDA autocast path) or None (by precision)")
        self.tile_dtype = tile_dtype
        idx = 0
        if device is not None:
            idx = getattr(device, 'index', device)
            idx = 0 if idx is None else int(idx)
            if getattr(device, 'type', 'cuda') != 'cuda':
                raise RuntimeError("HIPnnUNetPredictor runs on an MI355X only; there is no CPU fallback")
        self.device = _Device(idx)
        self.engines: list = []
        self.arch: Optional[UNetArch] = None
        self.plans_manager = None
        self.configuration_manager = None
        self.dataset_json = None
        self.allowed_mirroring_axes = None
        self.list_of_parameters: List[np.ndarray] = []
        self.label_manager = None
        self.regions_class_order = None      # a region-based model (labels.label_convention): the class value each head paints; else None

    # ------------------------------------------------------------------ initialisation
    def manual_initialization(self, arch: UNetArch, fold_blobs: Sequence[np.ndarray], patch_size: Sequence[int],
                              spacing: Sequence[float] = (1.5, 1.5), dataset_json: Optional[dict] = None,
                              plans: Optional[dict] = None, configuration: str = '2d',
                              inference_allowed_mirroring_axes: Optional[Sequence[int]] = (0, 1)):
        from .preprocess import DefaultPreprocessor
        self.arch = arch
        self.list_of_parameters = [np.ascontiguousarray(b, dtype=np.float32) for b in fold_blobs]
        self.allowed_mirroring_axes = tuple(inference_allowed_mirroring_axes) if inference_allowed_mirroring_axes else None
        self.dataset_json = dataset_json or {
            'channel_names': {str(i): f'ch{i}' for i in range(arch.input_channels)},
            'labels': {'background': 0, **{f'label{i + 1}': i + 1 for i in range(arch.num_classes)}},
            'file_ending': '.nrrd', 'multilabel': True}
        from .labels import label_convention
        self.regions_class_order = label_convention(self.dataset_json).class_order
        self.plans_manager = SimpleNamespace(plans=plans or {}, transpose_forward=[0, 1, 2], transpose_backward=[0, 1, 2])
        self.configuration_manager = SimpleNamespace(
            patch_size=list(patch_size), spacing=list(spacing), preprocessor_class=DefaultPreprocessor,
            normalization_schemes=['ZScoreNormalization'] * arch.input_channels,
            use_mask_for_norm=[False] * arch.input_channels, configuration=configuration)
        self._create_engines()

    def initialize_from_trained_model_folder(self, model_training_output_dir: str, use_folds, checkpoint_name: str = 'checkpoint_final.pth'):
        """Reads ``dataset.json`` / ``plans.json`` / ``fold_X/<checkpoint_name>`` exactly where upstream does."""
        from . import weights as W
        with open(os.path.join(model_training_output_dir, 'dataset.json')) as f:
            dataset_json = json.load(f)
        with open(os.path.join(model_training_output_dir, 'plans.json')) as f:
            plans = json.load(f)
        if use_folds is None or use_folds == 'auto':
            use_folds = sorted(int(m.group(1)) for m in (re.match(r'fold_(\d+)$', d) for d in os.listdir(model_training_output_dir)) if m)
        if isinstance(use_folds, (str, int)):
            use_folds = [use_folds]
        blobs, mirror, configuration = [], None, None
        n_in = len(dataset_json['channel_names'])
        from .labels import label_convention
        n_heads = label_convention(dataset_json).n_heads      # (a region-based model: one head per foreground region)
        for i, f in enumerate(use_folds):
            f = int(f) if f != 'all' else f
            sd, mirror_axes, init_args = W.load_checkpoint(os.path.join(model_training_output_dir, f'fold_{f}', checkpoint_name))
            if i == 0:
                configuration = init_args.get('configuration', '2d')
                mirror = mirror_axes
                arch = UNetArch.from_plans(plans, configuration, n_in, n_heads)
            blobs.append(W.pack_blob(arch, sd))
        cfg = plans['configurations'][configuration]
        self.manual_initialization(arch, blobs, cfg['patch_size'], cfg.get('spacing', (1.0, 1.0)), dataset_json, plans,
                                   configuration, mirror)
        self.plans_manager.transpose_forward = plans.get('transpose_forward', [0, 1, 2])
        self.plans_manager.transpose_backward = plans.get('transpose_backward', [0, 1, 2])
        self.configuration_manager.normalization_schemes = cfg.get('normalization_schemes', self.configuration_manager.normalization_schemes)
        self.configuration_manager.use_mask_for_norm = cfg.get('use_mask_for_norm', self.configuration_manager.use_mask_for_norm)

    def _create_engines(self):
        from .engine import Engine, set_precision_opted_in            # raises loudly if libts2d_engine.so is missing - no fallback
        for e in self.engines:
            e.close()
        self.engines = [Engine(self.arch, blob, self.device.index) for blob in self.list_of_parameters]
        for e in self.engines:
            set_precision_opted_in(e, self.precision)      # (precision='f16' on a ResidualEncoderUNet: the user has named the mode)
            e.set_tile_dtype(self.tile_dtype)

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []

    # ------------------------------------------------------------------ inference
    _INF_MESSAGE = ('Encountered inf in predicted array. Aborting... If this problem persists, reduce '
                    'value_scaling_factor in compute_gaussian or increase the dtype of predicted_logits to fp32')

    def _sliding_window_batch(self, list_of_data, fold: Optional[int] = 0, want_seg: bool = False, one_call: bool = True, out_shapes=None,
                              labelmap: bool = False, regions=None, probabilities=None):
        """One fold, N inputs [C,Z,H,W]: pad, tile, tiles x mirror variants through the engine, upstream's fp16 Gaussian aggregation
        on the device.  Every z slice of every input is one image.  ``one_call``: all images in ONE engine call (C-ABI
        ts2d_engine_predict_tiled_batch: the network takes the full-batch dispatch, an input's bytes do not depend on its batch-mates,
        an error names the input); otherwise one ts2d_engine_predict_tiled call per image (size-dependent dispatch).  Returns one
        array per input in the input's geometry: float16 [K,Z,H,W] logits, or the device-thresholded uint8 segmentation when ``want_seg``.
        A single case is a batch of one: the single-case methods below are this method on ``[data]`` with ``one_call=False``.
        ``out_shapes`` (with ``want_seg``, Z = 1): one in-plane extent ``(h, w)`` or None per input - the device resamples every input's
        logits (order 1) to its extent, None = the input's own, and thresholds them there (C-ABI ts2d_engine_predict_tiled_export, the
        export's ``resampling_fn_probabilities`` + threshold): uint8 [K,1,h,w] per input.
        ``fold`` None: EVERY fold, single-slice inputs [C,1,H,W], ONE engine call (C-ABI ts2d_ensemble_predict_tiled_export): per fold
        the same sliding window, the mean of the folds' float16 logits on the device (:func:`fold_mean_f16`, bit for bit), and every
        output is that of the mean; ``want_seg`` always goes through the export (at an input's own extent the taps are 1 / 0).
        ``one_call`` False there: the size-dependent dispatch, so the bytes are those of :meth:`predict_logits_from_preprocessed_data`.
        ``labelmap`` (a label-map model; single-slice inputs): ONE engine call (C-ABI ts2d_ensemble_predict_tiled_labelmap) over fold
        ``fold`` or, with None, every fold and their mean; the device resamples every input's logits to its extent of ``out_shapes``
        (None = its own: no resampling) and takes the argmax over the heads there (:func:`export.labelmap_statement`, byte for byte):
        uint8 [1,1,h,w] per input.
        ``regions`` (a region-based model: its ``regions_class_order``, one class value per head; single-slice inputs): the same call
        shape through C-ABI ts2d_ensemble_predict_tiled_regions - the device resamples as for ``labelmap``, thresholds every head with the
        export's predicate and paints the regions in that order (:func:`export.regions_statement`, byte for byte): uint8 [1,1,h,w] per input.
        ``probabilities`` (single-slice inputs): one ``((full_h, full_w), (box_y, box_x))`` per input - the extent the case had before
        cropping and where its rectangle sits in it.  ONE engine call (C-ABI ts2d_ensemble_predict_tiled_probabilities) over fold ``fold``
        or every fold and their mean: the device resamples as above, applies the inference non-linearity of the model's convention
        (``labelmap``: softmax; ``regions`` or neither: sigmoid), writes the float32 planes of the full extent with upstream's fill around
        the rectangle and decides the map on the logits in the same pass (csrc/kernels_prob.h; :func:`export.probabilities_statement`):
        ``(uint8 [1,1,full_h,full_w] - multilabel [K,1,full_h,full_w] -, float32 [K,1,full_h,full_w])`` per input.
        (The one method that touches the engine, under the name the test infrastructure overrides: tests/batch_util.py replaces it, and
        tests/host_predictor.py predict_sliding_window_return_logits, with the host restatement.)"""
        ensemble, n = fold is None, len(list_of_data)
        w = self._window(list_of_data, single_slice=ensemble or labelmap or regions is not None or probabilities is not None)
        patch, images, tiles, axes, g = w.patch, w.images, w.tiles, w.axes, w.g
        e = None if ensemble else self.engines[fold]
        engines = self.engines if ensemble else [e]
        per_image = [range(len(images))] if one_call else [[j] for j in range(len(images))]
        if probabilities is not None or labelmap or regions is not None:
            if probabilities is not None and len(probabilities) != n:
                raise AssertionError('probabilities needs one (full extent, box origin) per input')
            rects = self._export_rects(list_of_data, w.reverts, w.shapes, out_shapes if out_shapes is not None else [None] * n, True)
            decision = {'regions': tuple(regions)} if regions is not None else {'labelmap': True} if labelmap else {}
            if probabilities is None:
                entry = self._decided_entry(decision)
                planes = self._calls(w, per_image, one_call, lambda im, tl, grp: entry(engines, im, patch, tl, [rects[j] for j in grp], axes, g, one_call), engines[0])
                return [p[None, None] for p in planes]
            from .engine import predict_tiled_probabilities_ensemble
            rects = [r + tuple(int(v) for v in full) + tuple(int(v) for v in box) for r, (full, box) in zip(rects, probabilities)]
            mode = 'regions' if regions is not None else 'labelmap' if labelmap else 'multilabel'

            def call(im, tl, grp):
                pr, dc, _ = predict_tiled_probabilities_ensemble(engines, im, patch, tl, [rects[j] for j in grp], mode, regions, axes, g, full_batch=one_call)
                return list(zip(dc, pr))
            return [((d[None, None] if d.ndim == 2 else d[:, None]), pr[:, None]) for d, pr in self._calls(w, per_image, one_call, call, engines[0])]
        if ensemble and want_seg and out_shapes is None:
            out_shapes = [None] * n
        exports = None if out_shapes is None else self._export_rects(list_of_data, w.reverts, w.shapes, out_shapes, want_seg)
        want = dict(want_logits=not want_seg, want_seg=want_seg)
        if ensemble:
            from .engine import predict_tiled_export_ensemble
            planes = self._calls(w, [range(len(images))], one_call, lambda im, tl, grp: predict_tiled_export_ensemble(
                self.engines, im, patch, tl, exports, axes, g, **want, full_batch=one_call)[0 if want_seg else 2])
        elif exports is not None:
            planes = self._calls(w, per_image, one_call, lambda im, tl, grp: e.predict_tiled_export(
                im, patch, tl, [exports[j] for j in grp], axes, g, full_batch=one_call)[0], e)
        elif one_call:
            planes = self._calls(w, per_image, one_call, lambda im, tl, grp: e.predict_tiled_batch(im, patch, tl, axes, g, **want)[want_seg], e)
        else:
            planes = self._calls(w, per_image, one_call, lambda im, tl, grp: [e.predict_tiled(im[0], patch, tl[0], axes, g, **want)[want_seg]], e,
                                 flags=lambda: [e.last_tiled_inf])
        if exports is not None:              # resampled on the device: already the case's own rectangle, one plane per input
            return [p[:, None] for p in planes]
        results, j = [], 0
        for (Z, H, W), revert in zip(w.shapes, w.reverts):
            full = np.stack(planes[j:j + Z], axis=1) if Z != 1 else planes[j][:, None]
            j += Z
            results.append(full[(slice(None),) + revert[1:]])
        return results

    def _window(self, list_of_data, single_slice: bool):
        """The set-up every sliding window shares: the padded images with their tiles (:meth:`_pad_and_tile`), the mirror assertion, the gaussian
        and the mirror axes - as one namespace ``patch, images, tiles, owner, reverts, shapes, g, axes``."""
        patch = tuple(self.configuration_manager.patch_size)
        images, tiles, owner, reverts, shapes = self._pad_and_tile(list_of_data, patch, single_slice=single_slice)
        if self.use_mirroring and self.allowed_mirroring_axes and max(self.allowed_mirroring_axes) > 1:
            raise AssertionError('mirror_axes does not match the dimension of the input!')
        return SimpleNamespace(patch=patch, images=images, tiles=tiles, owner=owner, reverts=reverts, shapes=shapes,
                               g=sw.compute_gaussian(patch) if self.use_gaussian else None,
                               axes=self.allowed_mirroring_axes if self.use_mirroring else None)

    def _calls(self, w, groups, named: bool, call, engine=None, flags=None):
        """One engine call per group of images of the window ``w``: ``call(images, tiles, group)`` returns one result per image; they are
        collected in image order with the inf flags each call left (``flags()``; else the per-image flags of ``engine``, else of the first
        engine), and :meth:`_raise_on_inf` is applied (``named``: the calls carry several inputs)."""
        engine = self.engines[0] if engine is None else engine
        out, inf = [], []
        for grp in groups:
            out += call([w.images[j] for j in grp], [w.tiles[j] for j in grp], grp)
            inf += flags() if flags else engine.last_tiled_inf_per_image
        self._raise_on_inf(inf, w.owner, named)
        return out

    def _decided_entry(self, decision: dict):
        """The engine function that decides the maps of a model by its convention (``decision``: :meth:`_decision`, or {} for a multilabel model),
        as ``(engines, images, patch, tiles, rects, axes, g, full_batch) -> one uint8 array per image``."""
        from .engine import predict_tiled_export_ensemble, predict_tiled_labelmap_ensemble, predict_tiled_regions_ensemble
        if 'regions' in decision:
            return lambda eng, im, patch, tl, rc, axes, g, full: predict_tiled_regions_ensemble(eng, im, patch, tl, rc, decision['regions'], axes, g, full_batch=full)[0]
        if decision:
            return lambda eng, im, patch, tl, rc, axes, g, full: predict_tiled_labelmap_ensemble(eng, im, patch, tl, rc, axes, g, full_batch=full)[0]
        return lambda eng, im, patch, tl, rc, axes, g, full: predict_tiled_export_ensemble(eng, im, patch, tl, rc, axes, g, want_seg=True, full_batch=full)[0]

    def _pad_and_tile(self, list_of_data, patch, single_slice: bool):
        """Inputs [C,Z,H,W] -> every z slice of every input, padded up to the patch, as one image with its tile list (upstream order),
        the input that owns it, and per input the slicer that undoes the padding and the padded ``(Z, H, W)``."""
        images, tiles, owner, reverts, shapes = [], [], [], [], []
        for i, data in enumerate(list_of_data):
            data = np.asarray(data, dtype=np.float32)
            if single_slice and (data.ndim != 4 or data.shape[1] != 1):
                raise AssertionError('the fold ensemble on the device takes single-slice inputs (c, 1, y, z)')
            if data.ndim != 4:
                raise AssertionError('input_image must be a 4D np.ndarray or torch.Tensor (c, x, y, z)')
            padded, revert = sw.pad_nd_image(data, patch)
            C, Z, H, W = padded.shape
            slicers = sw.tile_slicers((H, W), patch, self.tile_step_size, Z)
            for d in range(Z):
                images.append(padded[:, d])
                tiles.append([(sx, sy) for (dd, sx, sy) in slicers if dd == d])
                owner.append(i)
            reverts.append(revert)
            shapes.append((Z, H, W))
        return images, tiles, owner, reverts, shapes

    @staticmethod
    def _export_rects(list_of_data, reverts, shapes, out_shapes, want_seg):
        """One ``(src_y, src_x, src_h, src_w, out_h, out_w)`` per input: the rectangle of the padded prediction that is the case, and
        the extent it is resampled to (None: its own)."""
        if not want_seg or len(out_shapes) != len(list_of_data) or any(Z != 1 for Z, _, _ in shapes):
            raise AssertionError('out_shapes needs want_seg, one extent (or None) per input and single-slice inputs')
        exports = []
        for data, revert, hw in zip(list_of_data, reverts, out_shapes):
            H, W = np.shape(data)[2:]
            exports.append((revert[2].start, revert[3].start, H, W) + (tuple(int(v) for v in hw) if hw is not None else (H, W)))
        return exports

    def _raise_on_inf(self, inf, owner, one_call):
        """Upstream's inf check on the flags of the device, one per image; a call that carries several inputs names the first bad one."""
        bad = sorted({owner[j] for j, f in enumerate(inf) if f})
        if bad:
            raise RuntimeError((f'input {bad[0]}: ' if one_call else '') + self._INF_MESSAGE)

    def _device_ensemble(self) -> bool:
        """Is this a fold ensemble whose folds are all real engines?  (The host doubles of the tests have none: they keep the logits route.)"""
        from .engine import Engine
        return len(self.engines) == len(self.list_of_parameters) > 1 and all(isinstance(e, Engine) for e in self.engines)

    def predict_sliding_window_return_logits(self, data: np.ndarray, fold: int = 0) -> np.ndarray:
        """One fold: tiles x mirror variants -> one engine batch per z slice -> upstream's fp16 Gaussian aggregation.
        data [C,Z,H,W] float32 -> float16 [K,Z,H,W]."""
        return self._sliding_window_batch([data], fold, one_call=False)[0]

    @staticmethod
    def _in_plane(out_shape, data):
        """``out_shape`` of the fast-path methods -> in-plane ``(h, w)``, None (no resampling) or False (not a case for the device export).
        Accepts (h, w) or, as ``properties['shape_after_cropping_and_before_resampling']`` holds it, (1, h, w)."""
        if out_shape is None:
            return None
        hw = tuple(int(v) for v in out_shape)
        if len(hw) == 3 and hw[0] == 1:
            hw = hw[1:]
        if len(hw) != 2 or min(hw) < 1:
            return False
        return None if hw == tuple(data.shape[2:]) else hw

    def predict_segmentation_from_preprocessed_data(self, data, out_shape=None):
        """Fast path of the product surface (not part of the reference's duck-typed seam): the multilabel segmentation
        ``sigmoid(float(half logits)) > 0.5`` thresholded ON THE DEVICE by the aggregation kernel (kernels_sw.h: the same predicate as
        export.py's bit-pattern test, verified on all 65 536 half values), so that K uint8 planes travel to the host instead of K float16
        ones and the host never thresholds.  One z-slice (the 2-D models of ts2d); returns uint8 [K, 1, H, W] in the
        preprocessed geometry, or None when the case needs the logits (3-D stacks; a predictor without engines).  A fold ensemble runs
        every fold in one engine call and the device takes the mean of the folds' logits in front of the threshold
        (:meth:`_sliding_window_batch` with ``fold=None``): the bytes are those of :meth:`predict_logits_from_preprocessed_data` + the host export.
        ``out_shape`` (the case's ``shape_after_cropping_and_before_resampling``, (h, w) or (1, h, w)): the export's order-1
        resample-back runs on the device in front of the threshold (kernels_resample.h; bit for bit the host route's
        ``resample_data_to_shape(order=1)`` + threshold) and the result is uint8 [K, 1, h, w] in THAT extent."""
        out = self._segmentation([data], None if out_shape is None else [out_shape], one_call=False, compare_engines=True)
        return None if out is None else out[0]

    def _fast_inputs(self, list_of_data, per_input, stack: bool = False, probe=None, compare_engines: bool = True, convert_first: bool = False):
        """THE guard of the fast-path methods: the inputs as float32 arrays and the in-plane extent each is resampled to (None: its own),
        ``(datas, hws)`` - or ``[]`` for no inputs, or None where the predictor keeps the logits route.  ``per_input``: the per-input
        lists of the method, ``out_shapes`` first, each None or of one entry per input.  ``stack``: the stack methods (:meth:`_serves_stacks`,
        any Z, ``out_shapes`` of ``(Z, h, w)``, and a list of the wrong length is refused before an empty call is answered); else the
        single-slice methods: a device ensemble, or one fold on - ``compare_engines`` - one engine.  ``probe``: the ``engine.has_*`` of an
        optional entry.  ``convert_first`` (the segmentation methods): the entries of ``out_shapes`` are converted, as far as the inputs go,
        before the length of the list is looked at - a malformed entry raises even in a list of the wrong length."""
        datas = [_to_numpy(d) for d in list_of_data]
        n = len(datas)
        lengths = all(v is None or len(v) == n for v in per_input)
        if stack:
            if not self._serves_stacks() or any(d.ndim != 4 for d in datas) or not lengths:
                return None
        elif not (self._device_ensemble() or (len(self.list_of_parameters) == 1 and (len(self.engines) == 1 or not compare_engines))) \
                or any(d.ndim != 4 or d.shape[1] != 1 for d in datas):
            return None
        if probe is not None and not probe():
            return None
        if not datas:
            return []
        if not lengths and not convert_first:
            return None
        extent = self._stack_extent if stack else self._in_plane
        hws = [extent(s, d) for s, d in zip(per_input[0] if per_input[0] is not None else [None] * n, datas)]
        return None if not lengths or any(hw is False for hw in hws) else (datas, hws)

    @staticmethod
    def _per_image(one_call: bool) -> dict:
        """``one_call`` as a keyword of :meth:`_sliding_window_batch` only where it is not the default: the doubles of the tests that override
        the method for the batch route need not know it."""
        return {} if one_call else {'one_call': False}

    def _fold(self):
        """The ``fold`` of :meth:`_sliding_window_batch` for the fast paths: every fold of a device ensemble, else the one there is."""
        return None if self._device_ensemble() else 0

    def _decision(self) -> dict:
        """The keyword of :meth:`_sliding_window_batch` that decides the map of this model: ``labelmap`` (argmax over the heads) or, for a
        region-based model, ``regions`` (its class order)."""
        order = getattr(self, 'regions_class_order', None)
        return {'labelmap': True} if order is None else {'regions': tuple(order)}

    def predict_labelmap_from_preprocessed_data(self, data, out_shape=None):
        """The twin of :meth:`predict_segmentation_from_preprocessed_data` for a LABEL-MAP model (the ordinary nnU-Net head: one head per
        label, background at 0): the export's order-1 resample-back and the argmax over the heads ON THE DEVICE (kernels_labelmap.h), so
        that ONE uint8 plane travels to the host instead of K float16 ones.  One z-slice; returns uint8 [1, 1, h, w] - the labels in the
        extent of ``out_shape`` (the case's ``shape_after_cropping_and_before_resampling``, (h, w) or (1, h, w); None: the preprocessed
        geometry) - or None when the case keeps the logits route (3-D stacks; a predictor without engines; a bad ``out_shape``).  A fold
        ensemble runs every fold in one engine call, the mean of the folds in front of the argmax.  The bytes are those of
        :meth:`predict_logits_from_preprocessed_data` + the host export (``resample_data_to_shape(order=1)`` + ``argmax``).
        A REGION-BASED model (``regions_class_order`` is set) takes the same route with its own decision: the sigmoid's predicate per
        head and the painting in class order (kernels_regions.h) in the place of the argmax - the decided map of whatever non-multilabel
        convention the model has."""
        out = self._labelmaps([data], None if out_shape is None else [out_shape], one_call=False)
        return None if out is None else out[0]

    def predict_labelmap_from_preprocessed_data_batch(self, list_of_data, out_shapes=None):
        """:meth:`predict_labelmap_from_preprocessed_data` for a list of inputs: uint8 [1,1,h,w] per input from ONE engine call (every
        fold of an ensemble in it), or None when the predictor keeps the logits route (a fold ensemble without engines), an input is no
        single z slice or an ``out_shapes`` entry is bad.  ``out_shapes``: one ``out_shape`` (or None) per input."""
        return self._labelmaps(list_of_data, out_shapes, one_call=True)

    def _labelmaps(self, list_of_data, out_shapes, one_call: bool):
        ok = self._fast_inputs(list_of_data, (out_shapes,))
        return ok if not ok else self._sliding_window_batch(ok[0], self._fold(), out_shapes=ok[1], **self._per_image(one_call), **self._decision())

    def _probability_mode(self) -> dict:
        """The keyword of :meth:`_sliding_window_batch` for this model's convention, as :meth:`_decision` - nothing for a multilabel model."""
        from .labels import label_convention
        return {} if label_convention(self.dataset_json).kind == 'multilabel' else self._decision()

    @staticmethod
    def _full_and_box(hw, data, full_shape, box):
        """``full_shape`` ((h, w) or (1, h, w); None: the output extent) and ``box`` ((y, x) or (0, y, x); None: the origin) of the
        probabilities methods -> ``((full_h, full_w), (box_y, box_x))``, or None where they describe no 2-D placement of the output."""
        out = tuple(int(v) for v in (hw if hw is not None else data.shape[2:]))
        full = out if full_shape is None else tuple(int(v) for v in full_shape)
        at = (0, 0) if box is None else tuple(int(v) for v in box)
        if len(full) == 3 and full[0] == 1:
            full = full[1:]
        if len(at) == 3 and at[0] == 0:
            at = at[1:]
        if len(full) != 2 or len(at) != 2 or min(at) < 0 or any(o + a > f for o, a, f in zip(out, at, full)):
            return None
        return full, at

    def predict_probabilities_from_preprocessed_data(self, data, out_shape=None, full_shape=None, box=None):
        """The export's PROBABILITIES from the device (``save_probabilities`` of the reference's predictor, predictor.py:99-111): the
        twin of :meth:`predict_segmentation_from_preprocessed_data` / :meth:`predict_labelmap_from_preprocessed_data` that also returns
        what the export computes in front of the decision.  ``out_shape`` as there; ``full_shape`` ((h, w) or (1, h, w)): the case's
        ``shape_before_cropping``, ``box`` ((y, x) or (0, y, x)): where the crop box begins in it (None, None: the output is the whole).
        Returns ``(decided uint8, float32 [K,1,full_h,full_w])`` - the decided map [1,1,full_h,full_w] of a label-map or region-based
        model or the thresholded planes [K,1,full_h,full_w] of a multilabel one, in the PRE-CROP extent, 0 outside the box, inside it the
        bytes of the sibling methods; the probabilities with upstream's fill (0; 1 in head 0 of a label-map model) - or None wherever the
        siblings return None, and with a library built before the entry."""
        out = self.predict_probabilities_from_preprocessed_data_batch([data], None if out_shape is None else [out_shape], [full_shape], [box],
                                                                      one_call=False)
        return None if out is None else out[0]

    def predict_probabilities_from_preprocessed_data_batch(self, list_of_data, out_shapes=None, full_shapes=None, boxes=None, one_call: bool = True):
        """:meth:`predict_probabilities_from_preprocessed_data` for a list of inputs: ``(decided, probabilities)`` per input from ONE
        engine call (every fold of an ensemble in it), or None.  ``out_shapes`` / ``full_shapes`` / ``boxes``: one entry (or None) per input."""
        from .engine import has_probabilities
        ok = self._fast_inputs(list_of_data, (out_shapes, full_shapes, boxes), probe=has_probabilities)
        if not ok:
            return ok
        (datas, hws), n = ok, len(ok[0])
        place = [self._full_and_box(hw, d, f, b) for hw, d, f, b in zip(hws, datas, full_shapes or [None] * n, boxes or [None] * n)]
        if any(pl is None for pl in place):
            return None
        return self._sliding_window_batch(datas, self._fold(), one_call=one_call, out_shapes=hws, probabilities=place, **self._probability_mode())

    # ------------------------------------------------------------------ stacks: a 3-D volume through a 2-D model, slice by slice
    stack_call_bytes = 1 << 30       # device bytes of inputs and outputs one engine call of the stack batch method may hold (see _stack_calls)

    @staticmethod
    def _stack_extent(out_shape, data):
        """``out_shape`` of the stack methods, ``(Z, h, w)`` with the stack's own Z -> the in-plane ``(h, w)`` every slice is resampled to (None: the
        slices' own), or False where it describes no such extent."""
        if out_shape is None:
            return tuple(int(v) for v in data.shape[2:])
        s = tuple(int(v) for v in out_shape)
        if len(s) != 3 or s[0] != data.shape[1] or min(s) < 1:
            return False
        return s[1:]

    @staticmethod
    def _stack_rects(datas, reverts, hws):
        """One ``(src_y, src_x, src_h, src_w, out_h, out_w)`` per SLICE of every input, in image order: the rectangle of the padded prediction that
        is the slice - the same for all slices of an input - and the extent it is resampled to."""
        rects = []
        for data, revert, hw in zip(datas, reverts, hws):
            H, W = data.shape[2:]
            rects += [(revert[2].start, revert[3].start, H, W, int(hw[0]), int(hw[1]))] * data.shape[1]
        return rects

    def _stack_calls(self, images, rects, multilabel: bool, fulls=None):
        """The images of the stack batch method split into engine calls, in order, by a byte budget (``stack_call_bytes``) on what the header's
        scratch formula sums over the images of a call: the inputs C x Hp x Wp x 4, the half outputs folds x K x Hp x Wp x 2, the export's outputs
        out_h x out_w (x K for a multilabel model).  At least one image per call.  Where the calls split does not show in the bytes: inside a
        full-batch call an image's result does not depend on its call-mates.  ``fulls`` (the probabilities of stacks): one ``(full_h, full_w)`` per
        image - its outputs are then the planes of that extent, K x full_h x full_w x 4 of probabilities and the decided planes beside them."""
        K, F, budget = self.arch.num_classes, max(1, len(self.engines)), int(self.stack_call_bytes)
        calls, used = [[]], 0
        for j, (image, r) in enumerate(zip(images, rects)):
            C, Hp, Wp = image.shape
            need = C * Hp * Wp * 4 + F * K * Hp * Wp * 2 + r[4] * r[5] * (K if multilabel else 1)
            if fulls is not None:
                need = C * Hp * Wp * 4 + F * K * Hp * Wp * 2 + fulls[j][0] * fulls[j][1] * (K * 4 + (K if multilabel else 1))
            if calls[-1] and used + need > budget:
                calls.append([])
                used = 0
            calls[-1].append(j)
            used += need
        return calls

    def _stack_window(self, datas, hws, full_batch: bool):
        """Inputs [C,Z,H,W] -> the decided uint8 maps of every slice from the device, stacked per input: [1,Z,h,w] of a label-map or region-based
        model, [K,Z,h,w] of a multilabel one.  Every slice is one image of the ensemble entries (ts2d_ensemble_predict_tiled_labelmap / _regions /
        _export: one engine is the single-model case), with its input's tile list, rectangle and out extent.  ``full_batch`` False: one call per
        slice with the size-dependent dispatch - the bytes of :meth:`predict_logits_from_preprocessed_data` + the host export; True: calls of
        :meth:`_stack_calls` with the full-batch dispatch - the bytes of :meth:`predict_logits_from_preprocessed_data_batch` + the host export."""
        from .labels import label_convention
        w = self._window(datas, single_slice=False)
        rects = self._stack_rects(datas, w.reverts, hws)
        multilabel = label_convention(self.dataset_json).kind == 'multilabel'
        entry = self._decided_entry({} if multilabel else self._decision())
        groups = self._stack_calls(w.images, rects, multilabel) if full_batch else [[j] for j in range(len(w.images))]
        planes = self._calls(w, groups, full_batch, lambda im, tl, grp: entry(self.engines, im, w.patch, tl, [rects[j] for j in grp], w.axes, w.g, full_batch))
        out, j = [], 0
        for data in datas:
            Z = data.shape[1]
            out.append(np.stack(planes[j:j + Z], axis=1) if multilabel else np.stack(planes[j:j + Z])[None])
            j += Z
        return out

    def _serves_stacks(self) -> bool:
        """Can the device decide the maps?  One real engine per fold (the host doubles of the tests have none: they keep the logits route) and a 2-D plan."""
        from .engine import Engine
        return len(self.engines) == len(self.list_of_parameters) >= 1 and all(isinstance(e, Engine) for e in self.engines) \
            and len(self.configuration_manager.patch_size) == 2

    def predict_stack_from_preprocessed_data(self, data, out_shape=None):
        """The decided map of a STACK [C,Z,H,W] - a 3-D volume that this 2-D model takes slice by slice - from the device, in the model's own
        convention: uint8 [1,Z,h,w] of a label-map model (argmax) or a region-based one (painted regions), uint8 [K,Z,h,w] of a multilabel one
        (thresholded heads).  ``out_shape``: the case's ``shape_after_cropping_and_before_resampling`` ``(Z, h, w)`` - Z the stack's own, (h, w) the
        extent every slice is resampled back to (order 1) in front of the decision; None: the preprocessed geometry.  One engine call per slice with
        the size-dependent dispatch, every fold of an ensemble in it: the bytes are those of :meth:`predict_logits_from_preprocessed_data` + the host
        export.  None where the device cannot serve (a predictor without engines, a 3-D plan, a bad ``out_shape``): the caller keeps the logits."""
        out = self._stacks([data], None if out_shape is None else [out_shape], full_batch=False)
        return None if out is None else out[0]

    def predict_stack_from_preprocessed_data_batch(self, list_of_data, out_shapes=None):
        """:meth:`predict_stack_from_preprocessed_data` for a list of inputs - stacks and single-slice cases may be mixed: the slices of all inputs packed
        into engine calls with the full-batch dispatch, as many per call as ``stack_call_bytes`` allows, so that a stack's bytes depend neither on that
        budget nor on its batch-mates; they are those of :meth:`predict_logits_from_preprocessed_data_batch` + the host export.  ``out_shapes``: one
        ``out_shape`` (or None) per input.  None where the single-case method returns None for some input."""
        return self._stacks(list_of_data, out_shapes, full_batch=True)

    def _stacks(self, list_of_data, out_shapes, full_batch: bool):
        ok = self._fast_inputs(list_of_data, (out_shapes,), stack=True)
        return ok if not ok else self._stack_window(*ok, full_batch=full_batch)

    # ------------------------------------------------------------------ ... and their probabilities: one strided volume per stack
    @staticmethod
    def _stack_place(hw, data, full_shape, box):
        """``full_shape`` ((Z0, H0, W0); None: the output's own extent) and ``box`` ((z0, y0, x0); None: the origin) of the stack probabilities
        methods -> ``((Z0, H0, W0), (z0, y0, x0))``, or None where the [Z, h, w] output does not lie inside that extent at that place."""
        out = (int(data.shape[1]),) + tuple(int(v) for v in hw)
        full = out if full_shape is None else tuple(int(v) for v in full_shape)
        at = (0, 0, 0) if box is None else tuple(int(v) for v in box)
        if len(full) != 3 or len(at) != 3 or min(at) < 0 or any(o + a > f for o, a, f in zip(out, at, full)):
            return None
        return full, at

    @staticmethod
    def _stack_runs(grp, owner, first_image, rects, places, probs, decs, multilabel: bool):
        """The run descriptors of ONE engine call of the stack probabilities (``engine.predict_tiled_probabilities_stack_ensemble``).  ``grp``: the
        call's images, consecutive indices into the image list; ``owner[j]`` the input of image j, ``first_image[i]`` the index of input i's first
        slice.  Consecutive images of one input are one run ``(first image in the call, n_slices, the ten numbers, probabilities view, decided
        view)``: the views are slices ``[z0 + s, z0 + s + n_slices)`` along axis 1 of that input's arrays - [K, Z0, H0, W0] float32 and
        [K or 1, Z0, H0, W0] uint8 (the one plane per slice of a non-multilabel model is passed without its leading axis) - so a volume that a call
        boundary splits contributes one run to each call, at different slice offsets of the same arrays."""
        runs, a = [], 0
        while a < len(grp):
            i = owner[grp[a]]
            b = a
            while b < len(grp) and owner[grp[b]] == i:
                b += 1
            (full, at), n = places[i], b - a
            z = at[0] + grp[a] - first_image[i]
            dec = decs[i][:, z:z + n] if multilabel else decs[i][0, z:z + n]
            runs.append((a, n, tuple(rects[grp[a]]) + tuple(full[1:]) + tuple(at[1:]), probs[i][:, z:z + n], dec))
            a = b
        return runs

    def _stack_probabilities_window(self, datas, hws, places, full_batch: bool):
        """:meth:`_stack_window` with the export's probabilities: per input ``(decided uint8 [1 or K, Z0, H0, W0], float32 [K, Z0, H0, W0])``, both
        allocated ONCE in their final layout.  The slabs outside the z range of the box are filled here with upstream's fill (0; 1 in head 0 of a
        label-map model); every slice inside it - its in-plane fill included - is written in place by the engine, a run of slices per call and input
        (C-ABI ts2d_ensemble_predict_tiled_probabilities_stack).  ``full_batch`` as in :meth:`_stack_window`."""
        from .engine import predict_tiled_probabilities_stack_ensemble
        from .labels import label_convention
        w = self._window(datas, single_slice=False)
        images, owner = w.images, w.owner
        rects = self._stack_rects(datas, w.reverts, hws)
        kind = label_convention(self.dataset_json).kind
        multilabel = kind == 'multilabel'
        mode = 'multilabel' if multilabel else 'regions' if 'regions' in self._decision() else 'labelmap'
        K = self.arch.num_classes
        probs, decs, first_image = [], [], []
        for data, (full, at) in zip(datas, places):
            first_image.append(sum(d.shape[1] for d in datas[:len(first_image)]))
            prob, dec = np.empty((K,) + full, dtype=np.float32), np.empty((K if multilabel else 1,) + full, dtype=np.uint8)
            for slab in (slice(0, at[0]), slice(at[0] + data.shape[1], full[0])):
                prob[:, slab] = 0
                if mode == 'labelmap':
                    prob[0, slab] = 1
                dec[:, slab] = 0
            probs.append(prob)
            decs.append(dec)
        fulls = [places[i][0][1:] for i in owner]

        def call(im, tl, grp):
            runs = self._stack_runs(grp, owner, first_image, rects, places, probs, decs, multilabel)
            predict_tiled_probabilities_stack_ensemble(self.engines, im, w.patch, tl, runs, mode, self._decision().get('regions'), w.axes, w.g,
                                                       full_batch=full_batch)
            return []
        self._calls(w, self._stack_calls(images, rects, multilabel, fulls) if full_batch else [[j] for j in range(len(images))], full_batch, call)
        return list(zip(decs, probs))

    def predict_stack_probabilities_from_preprocessed_data(self, data, out_shape=None, full_shape=None, box=None):
        """:meth:`predict_stack_from_preprocessed_data` with the export's PROBABILITIES (``save_probabilities`` for a 3-D volume under a 2-D plan):
        ``data`` [C,Z,H,W], ``out_shape`` ``(Z, h, w)`` as there, ``full_shape`` ``(Z0, H0, W0)`` the case's ``shape_before_cropping`` and ``box``
        ``(z0, y0, x0)`` where the crop box begins in it (None, None: the output is the whole).  Returns ``(decided uint8, float32 [K,Z0,H0,W0])`` -
        the decided map [1,Z0,H0,W0] of a label-map or region-based model, [K,Z0,H0,W0] of a multilabel one, 0 outside the box and inside it the
        bytes of :meth:`predict_stack_from_preprocessed_data`; the probabilities of :meth:`predict_probabilities_from_preprocessed_data` per slice
        with upstream's fill (0; 1 in head 0 of a label-map model) everywhere else, the slices outside the box along z included.  One engine call
        per slice with the size-dependent dispatch.  None where the stack methods or the probabilities methods return None: a predictor without
        engines, a 3-D plan, a bad shape, a box that leaves the full extent, a library built before the entry."""
        out = self._stack_probabilities([data], None if out_shape is None else [out_shape], [full_shape], [box], full_batch=False)
        return None if out is None else out[0]

    def predict_stack_probabilities_from_preprocessed_data_batch(self, list_of_data, out_shapes=None, full_shapes=None, boxes=None):
        """:meth:`predict_stack_probabilities_from_preprocessed_data` for a list of inputs - stacks and single-slice cases may be mixed: the slices of
        all inputs packed into full-batch engine calls by ``stack_call_bytes`` (:meth:`_stack_calls`; a call boundary may fall inside a volume), so
        that the bytes depend neither on that budget nor on the batch-mates: every slice has those of
        :meth:`predict_probabilities_from_preprocessed_data_batch`.  One entry (or None) per input in each list.  None where the single-case
        method returns None for some input."""
        return self._stack_probabilities(list_of_data, out_shapes, full_shapes, boxes, full_batch=True)

    def _stack_probabilities(self, list_of_data, out_shapes, full_shapes, boxes, full_batch: bool):
        from .engine import has_stack_probabilities
        ok = self._fast_inputs(list_of_data, (out_shapes, full_shapes, boxes), stack=True, probe=has_stack_probabilities)
        if not ok:
            return ok
        (datas, hws), n = ok, len(ok[0])
        places = [self._stack_place(hw, d, f, b) for hw, d, f, b in zip(hws, datas, full_shapes or [None] * n, boxes or [None] * n)]
        if any(pl is None for pl in places):
            return None
        return self._stack_probabilities_window(datas, hws, places, full_batch)

    def predict_logits_from_preprocessed_data(self, data):
        """Fold ensemble (upstream: sum over ``list_of_parameters`` then ``/= n``).  Accepts numpy or torch [C,1,H,W];
        returns a torch CPU tensor (float16) when torch is importable so that the caller's ``.cpu()`` works."""
        data, n = _to_numpy(data), max(1, len(self.list_of_parameters))
        return _to_torch(fold_mean_f16([self.predict_sliding_window_return_logits(data, f) for f in range(n)]))

    # ------------------------------------------------------------------ batched inference (N cases, one engine batch per fold)
    def predict_logits_from_preprocessed_data_batch(self, list_of_data):
        """:meth:`predict_logits_from_preprocessed_data` for a list of inputs: one batched engine call per fold (a [C,Z,H,W] input
        contributes Z images - a z-stack is one engine call, not Z), folds averaged as there.  Returns a list (torch CPU tensors when
        torch is importable)."""
        datas = [_to_numpy(d) for d in list_of_data]
        if not datas:
            return []
        n = max(1, len(self.list_of_parameters))
        per_fold = [self._sliding_window_batch(datas, f) for f in range(n)]
        return [_to_torch(fold_mean_f16(folds)) for folds in zip(*per_fold)]

    def predict_segmentation_from_preprocessed_data_batch(self, list_of_data, out_shapes=None):
        """:meth:`predict_segmentation_from_preprocessed_data` for a list of inputs: uint8 [K,1,H,W] per input from ONE engine call,
        or None when the predictor needs the logits (a fold ensemble without engines) or an input is no single z slice.  ``out_shapes``:
        one ``out_shape`` (or None) per input; inputs that resample and inputs that do not travel in the same call.  A fold ensemble:
        every fold and every input in ONE engine call, the mean of the folds on the device (:meth:`_sliding_window_batch` with ``fold=None``)."""
        return self._segmentation(list_of_data, out_shapes, one_call=True, compare_engines=False)

    def _segmentation(self, list_of_data, out_shapes, one_call: bool, compare_engines: bool):
        """The two segmentation methods.  ``compare_engines``: the single-case method wants its one fold on ONE engine; the batch method
        does not look (and goes through the export entry only where some input resamples)."""
        ok = self._fast_inputs(list_of_data, (out_shapes,), compare_engines=compare_engines, convert_first=True)
        if not ok:
            return ok
        kw = {} if all(hw is None for hw in ok[1]) else {'out_shapes': ok[1]}
        return self._sliding_window_batch(ok[0], self._fold(), want_seg=True, **self._per_image(one_call), **kw)
