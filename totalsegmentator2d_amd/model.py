"""In-process model handle: the replacement of the reference's ``NNUProcessModel`` (``ts2d/core/inference/nnu.py:98-241``)
and its ``ParallelPredictor`` worker pool (``ts2d/core/inference/predictor.py``).  Same surface - ``start / await_startup /
apply / stop``, ``channels``, ``multilabel``, ``revision`` - but no worker process, no Manager queue, no temp NRRD files:
``apply`` runs preprocess -> HIP engine -> export in the caller's process and reports per-stage timestamps like
``PredictTask.timestamps`` (``prediction_worker.py:57-58``).
"""
from __future__ import annotations

import inspect
import json
import os
import re
import time
from typing import Dict, List, Optional, Union

import numpy as np

from . import nrrd
from .export import export_prediction_from_logits, needs_logits
from .labels import label_convention
from .predictor import HIPnnUNetPredictor


def parse_int(v):
    try:
        return int(v)
    except (TypeError, ValueError):
        return v


class HIPModel:
    def __init__(self, config: dict):
        """config keys (reference ``model.json`` + loader additions): ``root``, ``model``, ``revision``, ``folds``, ``param``
        (``nnu.*`` dotted keys, reference wrapper.py:53-71), or ``synthetic`` = dict(arch, blobs, patch_size, dataset_json)."""
        self._config = dict(config)
        self._param = dict(config.get('param', {}))
        self._predictor: Optional[HIPnnUNetPredictor] = None
        self.timestamps: Dict[str, float] = {}
        self.labels: Optional[Dict[int, str]] = None
        self.colors = self._param.get('nnu.result.colors')
        self._dataset_json: Optional[dict] = None
        self.device_threshold = True     # thresholded segmentation straight from the device where the export needs no logits (_run)
        self.device_labelmap = True      # a label-map (non-multilabel) model: resample-back and argmax on the device, ONE uint8 plane to the host (_run); the host route's bytes
        self.device_regions = True       # a region-based model (label values are lists + regions_class_order): resample-back, sigmoid predicate and painting in class order on the device, ONE uint8 plane to the host (_run); the host route's bytes
        self.device_probabilities = True  # save_probabilities: resample-back, sigmoid / softmax, the fill around the crop box and the decision in one kernel, float32 planes of the pre-crop extent to the host (_run); the host route's segmentation bytes, its probabilities to a few float32 units
        self.device_input_resample = True   # order-3 resample of an off-spacing case's input on the device: the same float32 values as scipy, bit for bit (preprocess.resize_cubic_f64)
        self.device_input_normalize = True  # crop box, z-score (and that resample) of a native 2-D input on device-resident planes: the same float32 values as numpy, bit for bit (preprocess.zscore_f32_statement)
        self.device_input_normalize_schemes = True  # the same for every other nnU-Net scheme (masked z-score, CT, Rescale, RGB, none): the cases device_input_normalize leaves to numpy, the same bits (preprocess.*_f32_statement)
        self.device_input_stack = True   # a stack [C, Z, H, W] under a 2-D plan: crop box over three axes, unmasked normalisation with the statistics of the whole volume (and the per-slice resample) on device-resident planes; numpy's bits (preprocess.crop_box3_statement and the *_f32_statement of the flattened channel)
        self.device_input_stack_masked = True   # ... and a stack whose plan has use_mask_for_norm on a z-score channel (the MR plans): the 3-D hole filling of the non-zero mask, the statistics of the masked samples and the normalisation inside the mask on those planes; numpy's and scipy's bits (preprocess.fill_holes_sweeps_statement, masked_zscore_stack_statement)
        self.device_stack = True         # ... and its decided map from the device, every slice one image of the convention's own entry (_run; needs that convention's switch too); the host route's bytes
        self.device_stack_probabilities = True   # ... and, with save_probabilities, its probabilities: every slice through the kernel of device_probabilities, written in place into ONE float32 [K, Z0, H0, W0] (_run; needs device_stack and the convention's switch, and an untransposed plan); the host route's segmentation bytes, its probabilities to a few float32 units
        self.device_postprocessing = True   # a model with a postprocessing plan (set_postprocessing): 26-connected labelling of the final uint8 map, component sizes and the removal of all but the largest on the device, every step of the plan between one upload and one download (_run); the host route's bytes (postprocess.keep_largest_components_statement)
        self._postprocessing = None      # the plan (postprocess.PostprocessingPlan); None - the default - leaves the export exactly as it is
        self._discover()
        plan = self._param.get('nnu.postprocessing')               # a postprocessing.json or a folder that holds one; True: the model's own folder
        if plan is None or plan is False:
            plan = (self._config.get('synthetic') or {}).get('postprocessing')      # ... or a plan list stated beside synthetic weights
        elif plan is True:
            if self._data_dir is None:
                raise ValueError("nnu.postprocessing = True looks in the trained-model folder; a synthetic model has none")
            plan = self._data_dir
        self.set_postprocessing(plan)

    def set_postprocessing(self, plan):
        """The model's postprocessing plan: None (none), a ``postprocess.PostprocessingPlan``, a list of ``(labels_or_regions,
        background_label)`` steps, or the path of a ``postprocessing.json`` / of a trained-model folder (``postprocess.load_postprocessing``).
        Defined for label-map and region-based models; a multilabel model is refused here."""
        if plan is None:
            self._postprocessing = None
            return
        kind = label_convention(self._dataset_json).kind
        if kind == 'multilabel':
            raise ValueError(f"a postprocessing plan was given for the {kind} model {self.name!r}: the largest-component step is defined for "
                             "label-map and region-based models only")
        from .postprocess import load_postprocessing
        self._postprocessing = load_postprocessing(plan)

    @property
    def postprocessing(self):
        return self._postprocessing

    # ------------------------------------------------------------------ configuration (reference wrapper.py:113-162)
    def _discover(self):
        syn = self._config.get('synthetic')
        if syn is not None:
            self._dataset_json = syn['dataset_json']
            self._data_dir = None
        else:
            root = self._config['root']
            task = next((d for d in sorted(os.listdir(root)) if re.match(r'Dataset\d+_', d)), None)
            if task is None:
                raise RuntimeError(f"no nnU-Net v2 'Dataset###_*' directory found in {root}")
            trainer = '__'.join([self._param.get('nnu.trainer', 'nnUNetTrainer'), self._param.get('nnu.plans', 'nnUNetPlans'),
                                 self._param.get('nnu.configuration', '3d_fullres')])
            self._data_dir = os.path.join(root, task, trainer)
            with open(os.path.join(self._data_dir, 'dataset.json')) as f:
                self._dataset_json = json.load(f)
        self.labels = label_convention(self._dataset_json).names      # (a region-based model: {class value: region name})

    @property
    def name(self):
        return self._config.get('model', 'model')

    @property
    def revision(self):
        r = self._config.get('revision', 0)
        return f'r{r:03d}' if isinstance(r, int) else r

    @property
    def folds(self):
        f = self._param.get('nnu.folds', self._config.get('folds'))
        return tuple(f) if f else (0,)

    @property
    def channels(self) -> Dict[int, str]:
        return {int(k): v for k, v in self._dataset_json['channel_names'].items()}

    @property
    def multilabel(self) -> bool:
        return bool(self._dataset_json.get('multilabel', self._dataset_json.get('multiclass', False)))

    # ------------------------------------------------------------------ lifetime (reference nnu.py:118-137)
    def start(self, wait: bool = True):
        p = self._param
        kw = {}
        if p.get('nnu.predict.stepsize') is not None:
            kw['tile_step_size'] = float(p['nnu.predict.stepsize'])
        kw['use_mirroring'] = bool(p.get('nnu.predict.augment', True))        # reference default: True (wrapper.py:65)
        kw['verbose'] = bool(p.get('nnu.verbose', False))
        kw['device'] = self._config.get('device')
        kw['precision'] = p.get('hip.precision', self._config.get('precision', 'split'))     # engine arithmetic mode (include/ts2d_engine.h)
        pred = self._make_predictor(kw)
        syn = self._config.get('synthetic')
        if syn is not None:
            pred.manual_initialization(syn['arch'], syn['blobs'], syn['patch_size'], syn.get('spacing', (1.5, 1.5)),
                                       syn['dataset_json'], inference_allowed_mirroring_axes=syn.get('mirror_axes', (0, 1)))
        else:
            ck = p.get('nnu.predict.checkpoint', 'final')
            pred.initialize_from_trained_model_folder(self._data_dir, self.folds, f'checkpoint_{ck}.pth')
        self._predictor = pred
        if wait:
            self.await_startup()

    def _make_predictor(self, kw: dict):
        """The predictor object behind this model: always the HIP one (the CPU surface tests subclass the model, tests/surface_util.py)."""
        return HIPnnUNetPredictor(**kw)

    def await_startup(self):
        """Warm-up on a zero patch (reference prediction_worker.py:74-96): allocates the workspace, loads the kernels."""
        p = self._predictor
        ps = tuple(p.configuration_manager.patch_size)
        p.predict_logits_from_preprocessed_data(np.zeros((len(self.channels), 1) + ps, np.float32))

    def stop(self):
        if self._predictor is not None:
            self._predictor.close()
            self._predictor = None

    # ------------------------------------------------------------------ apply (reference nnu.py:169-241)
    def apply(self, inputs: Union[str, nrrd.Image, List, Dict], result_dir: Optional[str] = None, override: bool = True,
              save_probabilities: bool = False):
        """``save_probabilities`` (reference: ``ParallelPredictor.predict(..., save_probabilities=True)``, ts2d/core/inference/predictor.py:99-111):
        with a ``result_dir`` ``<name>.npz`` (key ``probabilities``: float32 [K, *original shape]) and ``<name>.pkl`` (the case's
        properties) appear beside ``<name>.nrrd``; without one the returned image carries the array as ``img.probabilities``.  The
        segmentation is byte for byte that of the same call without the flag."""
        if self._predictor is None:
            raise RuntimeError("model is not started")
        single = isinstance(inputs, (str, nrrd.Image))
        if single:
            inputs = [inputs]
        if isinstance(inputs, (list, tuple)):
            inputs = {f'image{i + 1}': img for i, img in enumerate(inputs)}
        results = {}
        for name, img in inputs.items():          # one input at a time through all four stages, as the reference's worker
            try:
                results.update(self._run({name: img}, result_dir, override, batched=False, stamps={}, save_probabilities=save_probabilities))
            except Exception as ex:
                raise RuntimeError(f"Prediction failed for: {name}: {ex}") from ex
        return next(iter(results.values())) if single else results

    @staticmethod
    def _preprocess_key(p, props) -> str:
        """Everything DefaultPreprocessor.run_case_npy reads besides the image itself: two sub-models with the same key preprocess identically."""
        cm, pm = p.configuration_manager, p.plans_manager
        dz = props.get('device_zscore')
        return repr((props.get('device_resample'), props.get('device_normalize'), props.get('device_normalize_schemes'), props.get('device_normalize_stack'), props.get('device_normalize_stack_masked')) + (list(getattr(pm, 'transpose_forward', [0, 1, 2])), list(cm.spacing), list(getattr(cm, 'normalization_schemes', None) or []),
                     list(getattr(cm, 'use_mask_for_norm', None) or []), sorted((p.dataset_json.get('channel_names') or {}).items()),
                     (getattr(pm, 'plans', None) or {}).get('foreground_intensity_properties_per_channel', {}),
                     None if dz is None else tuple(dz.get('order', ()))))

    def _input_device(self, switch: bool) -> Optional[int]:
        """GPU index for a device stage of the input side: the device of the predictor's engines.  None - the host route - with the stage's switch
        off and for a predictor that holds no engine of this library (a foreign or host-only predictor: there may be no GPU at all)."""
        from .engine import Engine
        engines = getattr(self._predictor, 'engines', None) or []
        if not switch or not engines or not isinstance(engines[0], Engine):
            return None
        return int(engines[0].device)

    def _resample_device(self) -> Optional[int]:
        """GPU index for the input resample (``device_input_resample``), or None: the host route."""
        return self._input_device(self.device_input_resample)

    def _normalize_device(self) -> Optional[int]:
        """GPU index for crop box and z-score of a native 2-D input (``device_input_normalize``), or None: the host route."""
        return self._input_device(getattr(self, 'device_input_normalize', False))

    def _preprocess_input(self, img):
        """Stage 1 of :meth:`_run`: read, to array, preprocess (the case's shared ``preprocess_cache`` is honoured).
        Returns (reference image, preprocessed data, properties)."""
        p = self._predictor
        ref = nrrd.read(img) if isinstance(img, str) else img
        from .preprocess import image_to_array
        data, props = image_to_array(ref)
        if getattr(ref, 'device_zscore', None) is not None:
            props['device_zscore'] = ref.device_zscore      # z-score done on the device behind the projection (image.py)
        if self._resample_device() is not None:
            props['device_resample'] = self._resample_device()   # an off-spacing case is resampled to the plan spacing on the device (preprocess.py)
        if self._normalize_device() is not None:
            props['device_normalize'] = self._normalize_device()  # a native 2-D input is cropped and z-scored on the device, on planes that stay there for the resample (preprocess.py)
        if self._input_device(getattr(self, 'device_input_normalize_schemes', False)) is not None:
            props['device_normalize_schemes'] = self._input_device(self.device_input_normalize_schemes)   # ... and normalised there by any other scheme of the plan
        if self._input_device(getattr(self, 'device_input_stack', False)) is not None:
            props['device_normalize_stack'] = self._input_device(self.device_input_stack)   # ... and a stack of slices under a 2-D plan is cropped and normalised there as a volume
        if self._input_device(getattr(self, 'device_input_stack_masked', False)) is not None:
            props['device_normalize_stack_masked'] = self._input_device(self.device_input_stack_masked)   # ... with the 3-D hole filling of the mask where a channel is normalised inside it
        pre = p.configuration_manager.preprocessor_class(verbose=p.verbose)
        shared = getattr(ref, 'preprocess_cache', None)      # set by TS2D.predict: the sub-models of one case mostly share channels and plan
        if shared is None:
            data, _, props = pre.run_case_npy(data, None, props, p.plans_manager, p.configuration_manager, p.dataset_json)
        else:
            key = self._preprocess_key(p, props)
            with shared['lock']:                             # (the first sub-model computes, its siblings wait for the result instead of repeating it)
                hit = shared['items'].get(key)
                if hit is None:
                    d2, _, p2 = pre.run_case_npy(data, None, props, p.plans_manager, p.configuration_manager, p.dataset_json)
                    d2.setflags(write=False)
                    hit = shared['items'][key] = (d2, p2)
            data, props = hit[0], dict(hit[1])
        return ref, data, props

    @staticmethod
    def _takes(fn, name: str) -> bool:
        """Does callable `fn` accept the keyword `name`?"""
        try:
            params = inspect.signature(fn).parameters
        except (TypeError, ValueError):
            return False
        return name in params or any(q.kind is q.VAR_KEYWORD for q in params.values())

    def _predict(self, datas, use_seg: bool, batched: bool, out_shapes=None, fast: str = 'predict_segmentation_from_preprocessed_data'):
        """Stage 2 of :meth:`_run`, the one stage that differs between :meth:`apply` and :meth:`apply_batch`: ONE predictor batch call
        over ``datas``, or the predictor's single-case methods per input - the reference's duck-typed seam
        (``predict_logits_from_preprocessed_data``, prediction_worker.py:206-209), which a foreign predictor without the batch methods
        serves too.  ``use_seg``: ask for the device-thresholded segmentation first (it answers None when the case needs the logits);
        ``out_shapes``: per input the extent its export resamples to, or None - passed on only when some input has one.  ``fast``: the
        name of that fast-path method - the segmentation of a multilabel model or the label map of an ordinary one."""
        p = self._predictor
        shapes = out_shapes if out_shapes is not None and any(s is not None for s in out_shapes) else None
        if batched:
            out = getattr(p, fast + '_batch')(datas, **({} if shapes is None else {'out_shapes': shapes})) if use_seg else None
            if out is None:
                out = p.predict_logits_from_preprocessed_data_batch(datas)
        else:
            out = [getattr(p, fast)(d, **({} if shapes is None or s is None else {'out_shape': s})) if use_seg else None
                   for d, s in zip(datas, shapes or [None] * len(datas))]
            out = [p.predict_logits_from_preprocessed_data(d) if o is None else o for d, o in zip(datas, out)]
        return [o.cpu().numpy() if hasattr(o, 'cpu') else o for o in out]

    def _predict_device(self, group, batched: bool, name: str, placed: bool):
        """Stage 2 of :meth:`_run` for cases whose map the device decides beyond :meth:`_predict`'s reach: per case what the predictor's method
        ``name`` answers - the decided map of a stack (``predict_stack_...``), or ``(decided map, probabilities)`` (``predict_probabilities_...``,
        ``predict_stack_probabilities_...``) - or, where it answers None, the logits (:meth:`_predict`): the export then takes the host route.
        The extent before resampling goes with each case and, with ``placed``, the extent before cropping and the origin of the crop box."""
        p = self._predictor
        datas = [t[3] for t in group]
        kw = {'out_shape': [tuple(t[4].get('shape_after_cropping_and_before_resampling', np.asarray(t[3]).shape[1:])) for t in group]}
        if placed:
            kw['full_shape'] = [tuple(t[4]['shape_before_cropping']) for t in group]
            kw['box'] = [tuple(int(b[0]) for b in t[4]['bbox_used_for_cropping']) for t in group]
        if batched:
            out = getattr(p, name + '_batch')(datas, **{'boxes' if k == 'box' else k + 's': v for k, v in kw.items()})
            out = list(out) if out is not None else [None] * len(group)
        else:
            out = [getattr(p, name)(d, **{k: v[i] for k, v in kw.items()}) for i, d in enumerate(datas)]
        rest = [i for i, o in enumerate(out) if o is None]
        for i, lg in zip(rest, self._predict([datas[i] for i in rest], False, batched) if rest else []):
            out[i] = lg
        return out

    def _routes(self, todo, batched: bool, save_probabilities: bool):
        """The route decision of :meth:`_run`: the preprocessed cases ``todo`` in at most three groups - stacks, fast, rest - each with the call
        that predicts it, ``[(group, predict), ...]``; ``predict()`` returns one result per case of its group."""
        p = self._predictor
        method = lambda name: getattr(p, name + ('_batch' if batched else ''), None)
        window_takes = lambda keyword: not hasattr(p, '_sliding_window_batch') or self._takes(p._sliding_window_batch, keyword)
        # product fast path: a multilabel 2-D case gets its segmentation thresholded on the device (K uint8 planes to the host instead
        # of K float16 ones; the predicate is the export step's, bit for bit).  A case whose export resamples (its spacing is not the
        # plan's) joins with the extent it had before resampling: the device resamples the logits back (order 1) in front of the
        # threshold and the export step receives uint8 planes already in that extent.  The reference's seam
        # (predict_logits_from_preprocessed_data + export_prediction_from_logits) stays as it is and serves every other case
        kind = label_convention(p.dataset_json).kind
        multilabel = kind == 'multilabel'
        fast_fn = method('predict_segmentation_from_preprocessed_data')
        can_seg = self.device_threshold and multilabel and fast_fn is not None
        # (a foreign predictor, or a double of the engine method, that knows the fast path but not its `out_shape(s)` keyword keeps
        #  the host route for resampled cases, as before the device export existed)
        can_export = can_seg and self._takes(fast_fn, 'out_shapes' if batched else 'out_shape') and window_takes('out_shapes')
        # a label-map model (the ordinary nnU-Net head): the same two host steps - resample-back, then the argmax over the heads - on the
        # device, ONE uint8 plane per case to the host; the export step receives it as the decided label map.  Only a predictor that has
        # the method (and, where it is a double of the engine method, its `labelmap` keyword) takes this route.  A region-based model goes
        # the same way under its own switch and keyword (`regions`: sigmoid predicate per head, painted in class order, kernels_regions.h)
        lm_name = 'predict_labelmap_from_preprocessed_data'
        lm_fn = method(lm_name)
        switch, keyword = ('device_regions', 'regions') if kind == 'regions' else ('device_labelmap', 'labelmap')
        can_lm = getattr(self, switch, False) and not multilabel and lm_fn is not None \
            and self._takes(lm_fn, 'out_shapes' if batched else 'out_shape') and window_takes(keyword)

        # save_probabilities: the decided maps alone cannot give them.  Either the device does everything in one kernel (resample-back, the
        # non-linearity, the fill around the crop box, the decision on the logits: kernels_prob.h) and the export receives the decided map
        # and the float32 planes of the pre-crop extent, or the logits travel and the export's host route computes both.  The guards are
        # those of can_lm: the predictor has the method and, where it is a double of the engine method, the `probabilities` keyword
        pr_name = 'predict_probabilities_from_preprocessed_data'
        pr_fn = method(pr_name)
        can_prob = save_probabilities and getattr(self, 'device_probabilities', False) and pr_fn is not None \
            and self._takes(pr_fn, 'full_shapes' if batched else 'full_shape') and window_takes('probabilities')
        if save_probabilities:
            can_seg = can_export = can_lm = False

        def target(t):
            """The extent the device export resamples case `t` to: None = none needed, False = not a case for it (a stack, a 3-D plan,
            a predictor without the export)."""
            shape = tuple(np.asarray(t[3]).shape[1:])
            if not needs_logits(t[4], shape):
                return None
            tgt = tuple(t[4]['shape_after_cropping_and_before_resampling'])
            return tgt if (can_export or can_lm or can_prob) and len(tgt) == len(shape) == 3 and tgt[0] == shape[0] == 1 else False
        # a stack - a 3-D volume under a 2-D plan, more than one slice left after cropping - gets the decided map of its convention from the
        # device too, every slice one image of the same entries (the predictor's stack methods); its slice count never changes.  Only a predictor
        # that has the methods takes this route, and only with the convention's own switch on.  With save_probabilities the stack takes the
        # predictor's stack probabilities methods instead - the kernel of can_prob per slice, written in place into one [K, Z0, H0, W0] - under a
        # switch of their own, and only for an untransposed plan (the slice axis must be the volume's first)
        st_name = 'predict_stack_probabilities_from_preprocessed_data' if save_probabilities else 'predict_stack_from_preprocessed_data'
        can_stack = getattr(self, 'device_stack', False) and method(st_name) is not None \
            and len(p.configuration_manager.patch_size) == 2 and bool(self.device_threshold if multilabel else getattr(self, switch, False))
        if save_probabilities:
            can_stack = can_stack and getattr(self, 'device_stack_probabilities', False) \
                and list(getattr(p.plans_manager, 'transpose_forward', [0, 1, 2])) == [0, 1, 2]

        def is_stack(t):
            shape = tuple(np.asarray(t[3]).shape[1:])
            tgt = tuple(t[4].get('shape_after_cropping_and_before_resampling', shape))
            return can_stack and len(tgt) == len(shape) == 3 and tgt[0] == shape[0] > 1
        stacks = [t for t in todo if is_stack(t)]
        fast = [t for t in todo if (can_seg or can_lm or can_prob) and not is_stack(t) and target(t) is not False and (not can_prob or np.asarray(t[3]).shape[1] == 1)]
        rest = [t for t in todo if not any(t is f for f in fast + stacks)]
        lm = {'fast': lm_name} if can_lm else {}
        return [(stacks, lambda: self._predict_device(stacks, batched, st_name, placed=save_probabilities)),
                (fast, (lambda: self._predict_device(fast, batched, pr_name, placed=True)) if can_prob else
                 (lambda: self._predict([t[3] for t in fast], True, batched, [target(t) for t in fast], **lm))),
                (rest, lambda: self._predict([t[3] for t in rest], False, batched, None, **lm))]

    def _run(self, inputs: dict, result_dir, override, batched: bool, stamps: dict, save_probabilities: bool = False) -> dict:
        """The reference worker's four stages (``prediction_worker.py:177-242``) over ``inputs``: output file, preprocessing of every
        input, prediction (per group of :meth:`_routes`: the inputs that share the fast-path decision), export of each.
        Each stage fails under its own name - ``"<Stage> failed for <name>: <cause>"`` - so that a HIP error (``ts2d_last_error``)
        tells which stage raised it.  ``stamps[name]`` receives ``start / preprocessed / predicted / exported / done`` per input (the
        inputs of one group share ``predicted``); ``timestamps`` follows the input at work.  ``override=False`` skips existing outputs
        before any device work."""
        p = self._predictor
        results: dict = {}
        todo = []
        for name, img in inputs.items():
            ts = self.timestamps = stamps[name] = {'start': time.time()}
            ofile = None
            try:
                if result_dir is not None:
                    os.makedirs(result_dir, exist_ok=True)
                    ofile = os.path.join(result_dir, name)
                    wanted = ('.nrrd', '.npz', '.pkl') if save_probabilities else ('.nrrd',)
                    if not override and all(os.path.exists(ofile + ext) for ext in wanted):
                        results[name] = ofile + '.nrrd'
                        continue
            except Exception as ex:
                raise RuntimeError(f"Could not create output directory: {ex}") from ex
            try:
                ref, data, props = self._preprocess_input(img)
                ts['preprocessed'] = time.time()
            except Exception as ex:
                raise RuntimeError(f"Preprocessing failed for {name}: {ex}") from ex
            todo.append([name, ofile, ref, data, props, None])
        for group, predict in self._routes(todo, batched, save_probabilities):
            if not group:
                continue
            try:
                out = predict()
            except Exception as ex:
                names = ', '.join(t[0] for t in group)
                m = re.match(r'input (\d+): ', str(ex))          # the predictor names the offending input of the batch by index
                if m and int(m.group(1)) < len(group):
                    names = group[int(m.group(1))][0]
                raise RuntimeError(f"Prediction failed for {names}: {ex}") from ex
            now = time.time()
            for t, o in zip(group, out):
                t[5] = o
                stamps[t[0]]['predicted'] = now
        # the model's postprocessing plan, if it has one: the export applies it to the final map (export_prediction_from_logits) - on the device
        # of the predictor's engines under `device_postprocessing`, on the host (the same bytes) with the switch off or no engine of this library
        post = getattr(self, '_postprocessing', None)
        post_device = self._input_device(getattr(self, 'device_postprocessing', False)) if post is not None else None
        for name, ofile, ref, data, props, logits in todo:
            ts = self.timestamps = stamps[name]
            try:
                more = {}
                if save_probabilities:           # (a pair: the device's decided map and its probabilities; else the logits for the host route)
                    more = {'save_probabilities': True, 'probabilities': logits[1] if isinstance(logits, tuple) else None}
                    logits = logits[0] if isinstance(logits, tuple) else logits
                if post is not None:             # (no plan: the export is called exactly as before)
                    more['postprocess'] = lambda s, ts=ts: self._postprocess(s, post, post_device, ts)
                seg = export_prediction_from_logits(logits, props, p.configuration_manager, p.plans_manager, p.dataset_json, ofile,
                                                    ref_image=ref, labels=self.labels,
                                                    colors=self.colors if isinstance(self.colors, dict) else None, **more)
                ts['exported'] = ts['done'] = time.time()
            except Exception as ex:
                raise RuntimeError(f"Export failed for {name}: {ex}") from ex
            results[name] = (ofile + '.nrrd') if result_dir is not None else seg
        return {name: results[name] for name in inputs}

    @staticmethod
    def _postprocess(seg, plan, device, ts: dict):
        """The closure :meth:`_run` hands to the export: ``postprocess.apply_postprocessing`` of the final map, stamped ``postprocessed``."""
        from .postprocess import apply_postprocessing
        out = apply_postprocessing(seg, plan, device=device)
        ts['postprocessed'] = time.time()
        return out

    def apply_batch(self, inputs: Union[List, Dict], result_dir: Optional[str] = None, override: bool = True,
                    save_probabilities: bool = False) -> dict:
        """:meth:`apply` for several inputs with ONE engine batch (the reference's ``apply`` submits every input to its worker pool before
        it waits, ``ts2d/core/inference/nnu.py:194-216``): the stages of :meth:`_run` over all inputs, the prediction one predictor
        batch call per fast-path group.  Inside the batched engine call the network always takes the full-batch dispatch, so an
        input's result does not depend on the other inputs of the call.  Errors: ``"<Stage> failed for <name>: <cause>"``.
        ``batch_timestamps[name]`` holds the stamps per input; ``timestamps`` is left at the last input's values.
        ``save_probabilities``: as in :meth:`apply`."""
        if self._predictor is None:
            raise RuntimeError("model is not started")
        if isinstance(inputs, (list, tuple)):
            inputs = {f'image{i + 1}': img for i, img in enumerate(inputs)}
        self.batch_timestamps = {}
        return self._run(inputs, result_dir, override, batched=True, stamps=self.batch_timestamps, save_probabilities=save_probabilities)
