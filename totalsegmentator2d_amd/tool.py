"""``TS2D`` - the public API surface of the reference (``ts2d/tool.py:19-311``) on top of the MI355X engine.

Same constructor, ``predict(input, collapse, merge) -> TS2D.Result`` and ``Result`` accessors / ``save`` naming
(``<name>.seg.nrrd``, ``<name>-<group>.seg.nrrd``, ``<name>_<channel>.nrrd``; reference tool.py:235-311,
test/test_030_cli.py:46-50).  Differences: models run in-process (no worker pool, no temp files); the sub-models of one case
run CONCURRENTLY (one host thread per sub-model, each engine on its own HIP stream: a case is 2 tiles x 4 mirror passes = 8 slices
per sub-model, which leaves most of the GPU idle when the five are driven one after the other as the reference does,
tool.py:110-112; ``concurrent_models=False`` restores that order - the results are identical); the PNG twins of ``Result.save``
(``content='visual'`` / ``'all'``, reference tool.py:272-311) are ``image.create_visual`` written by ``png.write`` - rendered on the device of
the engines (C-ABI ``ts2d_visual_labels`` / ``ts2d_visual_grey``), from the host statement in visual.py without one: the bytes are the same.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, List, Optional, Union

import numpy as np

from . import nrrd, png
from .image import (cast, combine_segmentations, compose, create_visual, get_actual_dimension, project, reduce_dimensions, reorient_image,
                    restore_dimension, split_channels)
from .model import HIPModel
from .statistics import dump_statistics, label_statistics
from .zoo import LocalZoo, decompose_model_key, get_label_colors


def _as_list(v):
    return list(v) if isinstance(v, (list, tuple, set)) else [v]


class TS2D:
    def __init__(self, key: str = "ts2d", use_remote: bool = True, fetch_remote: bool = True,
                 models: Optional[Dict[str, HIPModel]] = None, zoo_root: Optional[str] = None, device=None,
                 concurrent_models: bool = True, synthetic_xr=None, synthetic_xr_channels=('xr', 'xray', 'x-ray')):
        """``models``: pre-built ``{id: HIPModel}`` (synthetic-weight models in tests / bench); otherwise `key` is resolved
        against the local zoo.  ``use_remote`` / ``fetch_remote`` are accepted for signature compatibility (no network).

        ``synthetic_xr``: an ``xray.XRGeometry``, or True for its defaults, switches the synthetic radiograph on: for a 3-D input, a channel
        whose name is one of ``synthetic_xr_channels`` is rendered from the volume (``xray.synthetic_xr``, on the engines' device) where
        ``image.project`` would refuse the name, and a 3-D reference is scored through the same rays (``Result._scored_pair``).  Unset (None or
        False), nothing changes: such a channel name on a 3-D input raises what it always raised."""
        self.models: Dict[str, HIPModel] = {}
        self.concurrent_models = bool(concurrent_models)
        self.synthetic_xr = None
        if synthetic_xr is not None and synthetic_xr is not False:
            from .xray import _geometry
            self.synthetic_xr = _geometry(synthetic_xr)
        self.synthetic_xr_channels = tuple(str(c).lower().strip() for c in synthetic_xr_channels)
        if models is None:
            self.zoo = LocalZoo(zoo_root)
            ids = self.zoo.resolve(key, unique_model=True)
            if not ids:
                raise RuntimeError(f"No models were resolved for key: {key}")
            models = {}
            for mid in ids:
                try:
                    cfg = self.zoo.load_config(mid, {'server.workers': 1, 'nnu.result.colors': get_label_colors()})
                    cfg['device'] = device
                    models[mid] = HIPModel(cfg)
                except Exception as ex:
                    raise RuntimeError(f"Failed to load model {mid}" + (f" (resolved from {key})" if key != mid else "")) from ex
        for mid, model in models.items():
            try:
                if getattr(model, 'colors', None) is None:      # reference tool.py:29-33: every model gets the packaged label colours
                    model.colors = get_label_colors()
                model.start(wait=False)
                if not model.multilabel:
                    warnings.warn(f"The loaded model {mid} is not configured for multilabel inference.")
                self.models[mid] = model
            except Exception as ex:
                self.close()
                raise RuntimeError(f"Failed to load model {mid}") from ex
        for model in self.models.values():
            model.await_startup()
        # the projections run on the GPU when every model is backed by HIP engines (always, on the product path)
        self._gpu_projection = all(bool(getattr(getattr(m, '_predictor', None), 'engines', None)) for m in self.models.values())

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        self.close()

    def close(self):
        pool, self._pool = getattr(self, '_pool', None), None
        if pool is not None:
            pool.shutdown(wait=True)
        for model in self.models.values():
            model.stop()
        self.models = {}

    def _executor(self, n: int):
        """One worker thread per sub-model for the life of this object (not five new threads per case)."""
        pool = getattr(self, '_pool', None)
        if pool is None or pool._max_workers < n:
            from concurrent.futures import ThreadPoolExecutor
            if pool is not None:
                pool.shutdown(wait=True)
            pool = self._pool = ThreadPoolExecutor(max_workers=n, thread_name_prefix='ts2d-submodel')
        return pool

    @staticmethod
    def _as_image(input) -> nrrd.Image:
        if isinstance(input, str):
            input = nrrd.read(input)
        if not isinstance(input, nrrd.Image):
            raise RuntimeError(f"input must be a string path or an image, found: {type(input).__name__}")
        return input

    def _fan_out(self, run) -> dict:
        """``{mid: run(mid)}`` over the sub-models - concurrently: the C-ABI's handles are independent (include/ts2d_engine.h: one
        caller thread per engine), every engine runs on its own stream, and ctypes releases the interpreter lock for the duration of a
        call.  On a failure the sub-models that have not started are cancelled and EVERY running one is waited for before the first
        failure (in sub-model order) is raised: no engine is still at work on a worker thread when the caller gets control back."""
        order = sorted(self.models)
        if not (self.concurrent_models and len(order) > 1):
            return {mid: run(mid) for mid in order}
        pool = self._executor(len(order))
        futs = {mid: pool.submit(run, mid) for mid in order}
        done, failure = {}, None
        for mid in order:
            try:
                done[mid] = futs[mid].result()
            except BaseException as ex:
                if failure is None:
                    failure = ex
                    for f in futs.values():
                        f.cancel()
        if failure is not None:
            raise failure
        return done

    @staticmethod
    def _result(input: nrrd.Image, cache: dict, models: dict, merge: bool) -> "TS2D.Result":
        result: dict = {'models': models}
        if merge:
            segs = [r['segmentation'] for _, r in sorted(models.items())]
            drawn = sorted(m for m, r in models.items() if r.get('xr_geometry') is not None)
            if drawn and len(drawn) != len(models) and any(s.size != segs[0].size for s in segs[1:]):
                raise RuntimeError(f"the sub-models on synthetic radiographs ({', '.join(drawn)}) and those on projections "
                                   f"({', '.join(sorted(set(models) - set(drawn)))}) have different grids: there is no merged segmentation, "
                                   f"predict with merge=False")
            result['segmentation'] = segs[0] if len(segs) == 1 else combine_segmentations(segs)
        result['input'] = input
        if cache.get('projections'):
            result['projections'] = cache['projections']
        return TS2D.Result(result)

    def _is_xr_channel(self, name: str) -> bool:
        from .image import parse_projection_mode
        return self.synthetic_xr is not None and parse_projection_mode(name)[0] in self.synthetic_xr_channels

    def _render_xr_channels(self, mid: str, input: nrrd.Image, channels, projections: dict) -> bool:
        """The channels of sub-model ``mid`` that are synthetic radiographs, rendered once per case under their names (``xray.synthetic_xr`` on
        the engines' device, its host statement without one).  True when the sub-model has one; a sub-model that mixes a radiograph with
        projected channels needs them on one grid (parallel rays), which :meth:`_prepare_model_input` checks."""
        mine = [n for _, n in channels if self._is_xr_channel(n)]
        if mine and input.components != 1:
            raise RuntimeError(f"Model {mid}: a synthetic radiograph needs a scalar volume, found {input.components} components")
        for n in mine:
            if n not in projections:
                from .xray import synthetic_xr
                dev = (getattr(self.models[mid]._predictor.device, 'index', 0) or 0) if self._gpu_projection else None
                projections[n] = synthetic_xr(input, self.synthetic_xr, device=dev)
        return bool(mine)

    def predict(self, input: Union[nrrd.Image, str], collapse: bool = False, merge: bool = True, probabilities: bool = False) -> "TS2D.Result":
        """``probabilities``: every sub-model also returns the probabilities of its export (``HIPModel.apply(save_probabilities=True)``:
        float32 [K, *shape of its 2-D input]), kept per sub-model and reachable through ``Result.get_probabilities(model)``.  There is no
        merged array: the reference defines none.  The segmentations are byte for byte those of the call without the flag."""
        input = self._as_image(input)
        cache: dict = {}
        # input side per sub-model (projections are computed once and cached), then the networks
        prepared = {mid: self._prepare_model_input(mid, input, cache) for mid in sorted(self.models)}
        done = self._fan_out(lambda mid: self._apply_model(mid, prepared[mid], collapse, probabilities))
        return self._on_device(self._result(input, cache, done, merge))

    def _on_device(self, result: "TS2D.Result") -> "TS2D.Result":
        """Hand the result the device of the engines (its PNG visuals are rendered there); None where the models are not backed by HIP engines."""
        if self._gpu_projection and self.models:
            first = self.models[sorted(self.models)[0]]
            result.device = getattr(first._predictor.device, 'index', 0) or 0
        return result

    def predict_many(self, inputs, collapse: bool = False, merge: bool = True, max_cases: int = 8, probabilities: bool = False) -> List["TS2D.Result"]:
        """:meth:`predict` for several cases: per sub-model ONE engine batch over groups of at most ``max_cases`` cases
        (``HIPModel.apply_batch``) instead of one small batch per case; the sub-models run concurrently on their own threads and streams as
        in :meth:`predict`.  Inside a batched engine call the network always takes the full-batch dispatch, so a case's result does not
        depend on which other cases travel with it, on their order or on ``max_cases``; against :meth:`predict` (small-batch dispatch)
        it agrees to fp32 summation order (a few float16 ulps at most on the aggregated logits: each rounding into the half buffer may flip).
        ``max_cases=8`` makes 64 network rows for the default case of 2 tiles x 4 mirror passes.  Host memory: every case of a group holds
        its K result planes of Hp x Wp bytes per sub-model until the group is exported (float16 planes where an export resamples).
        ``probabilities``: as in :meth:`predict` (``HIPModel.apply_batch(save_probabilities=True)``)."""
        images = [self._as_image(inp) for inp in inputs]
        max_cases = max(1, int(max_cases))
        order = sorted(self.models)
        caches = [dict() for _ in images]
        prepared = [{mid: self._prepare_model_input(mid, img, cache) for mid in order} for img, cache in zip(images, caches)]

        def run_model(mid):
            out = []
            for g0 in range(0, len(images), max_cases):
                out += self._apply_model_batch(mid, [pr[mid] for pr in prepared[g0:g0 + max_cases]], collapse, first=g0, probabilities=probabilities)
            return out
        done = self._fan_out(run_model)
        return [self._on_device(self._result(img, cache, {mid: done[mid][i] for mid in order}, merge)) for i, (img, cache) in enumerate(zip(images, caches))]

    def _model_result(self, mid: str, prepared, collapse: bool, seg, timestamps: dict) -> dict:
        """What one sub-model contributes to a ``Result``: the segmentation ``model.apply`` returned for ``prepared``, its 3-D geometry restored."""
        input, input2d, native_2d = prepared
        res = {'id': mid, 'revision': self.models[mid].revision}
        if getattr(input2d, 'xr_geometry', None) is not None:      # (a rendered sub-model: a 3-D reference is scored through the same rays)
            res['xr_geometry'] = input2d.xr_geometry
        res['model'], res['group'] = decompose_model_key(mid)
        if getattr(seg, 'probabilities', None) is not None:      # (asked for: the array rides on the image the export returned)
            res['probabilities'] = seg.probabilities
        if not (collapse or native_2d):
            seg = restore_dimension(seg, input)
        res['input'] = input2d if collapse else input
        res['segmentation'] = seg
        res['timestamps'] = dict(timestamps)
        return res

    def _apply_model(self, mid: str, prepared, collapse: bool, probabilities: bool = False) -> dict:
        """Reference tool.py:172-174: ``model.apply`` + restoring the 3-D geometry."""
        model = self.models[mid]
        more = {'save_probabilities': True} if probabilities else {}
        return self._model_result(mid, prepared, collapse, model.apply(prepared[1], **more), model.timestamps)

    def _apply_model_batch(self, mid: str, prepared: list, collapse: bool, first: int = 0, probabilities: bool = False) -> List[dict]:
        """:meth:`_apply_model` for a group of cases: one ``model.apply_batch``."""
        model = self.models[mid]
        names = [f'case{first + i + 1}' for i in range(len(prepared))]
        segs = model.apply_batch({n: pr[1] for n, pr in zip(names, prepared)}, **({'save_probabilities': True} if probabilities else {}))
        return [self._model_result(mid, pr, collapse, segs[n], model.batch_timestamps[n]) for n, pr in zip(names, prepared)]

    def _predict_model(self, mid: str, input: nrrd.Image, collapse: bool, cache: dict) -> dict:
        return self._apply_model(mid, self._prepare_model_input(mid, input, cache), collapse)

    def _prepare_model_input(self, mid: str, input: nrrd.Image, cache: dict):
        """Reference tool.py:145-171: the 2-D multi-channel input of one sub-model (projections cached across sub-models)."""
        model = self.models[mid]
        channels = sorted(model.channels.items())
        projections = cache.setdefault('projections', {})
        rendered = False
        if get_actual_dimension(input) > 2:
            rendered = self.synthetic_xr is not None and self._render_xr_channels(mid, input, channels, projections)
            need = [n for _, n in channels if n not in projections]
            on_device = self._gpu_projection and input.components == 1 and input.array.dtype.name in ('int16', 'uint8', 'float32', 'uint16', 'int32')
            if need and on_device and all(n.lower() in ('max', 'mip', 'mean', 'avg') for n in need):
                # product path: both projections in one pass over the volume on the GPU, reorientation folded into the strides
                from .image import project_coronal_gpu
                pr = project_coronal_gpu(input, getattr(model._predictor.device, 'index', 0) or 0, zscore=True)
                for n in need:
                    projections[n] = pr['max' if n.lower() in ('max', 'mip') else 'mean']
                cache['device_zscore'] = pr['zscore']      # both projections normalised on the device (preprocess.py uses it)
            elif on_device and not self._max_mean_only(channels) and self._project_modes_on_device(model, input, channels, cache):
                pass                                       # every channel of this sub-model projected and normalised by ts2d_project_coronal_modes
            elif need or not rendered:                     # (a sub-model of radiographs alone has nothing left to project: no reorientation copy)
                input = reorient_image(input, 'RAI')
            chs = []
            for _, ch_name in channels:                      # channel NAME = projection mode (reference tool.py:156-158)
                if ch_name not in projections:
                    projections[ch_name] = cast(project(input, mode=ch_name, axis='coronal'), np.float32)
                chs.append(projections[ch_name])
            if rendered and any(c.size != chs[0].size or not np.allclose(c.spacing, chs[0].spacing, rtol=1e-5, atol=1e-8) for c in chs[1:]):
                raise RuntimeError(f"Model {mid} mixes synthetic radiographs and projections on different grids: "
                                   + ', '.join(f"{n}: size {c.size}, spacing {tuple(c.spacing)}" for (_, n), c in zip(channels, chs))
                                   + " (parallel rays put them on one grid)")
            input = compose(chs) if len(chs) > 1 else chs[0]
        else:
            if len(channels) != input.components:
                raise RuntimeError(f"The number of channels in the input image does not match the models channel definition "
                                   f"({len(channels)} vs {input.components}).")
            projections.update((f"ch{i}", ch) for i, ch in enumerate(split_channels(input)))
        native_2d = input.dimension < 3
        input2d = input if native_2d else reduce_dimensions(input)
        dz = cache.get('device_zscore')
        if dz is not None and not native_2d and all(n.lower() in ('max', 'mip', 'mean', 'avg') for _, n in channels):
            # channel order of THIS model over the (max, mean) planes the device normalised
            input2d.device_zscore = dict(dz, order=tuple(0 if n.lower() in ('max', 'mip') else 1 for _, n in channels))
        zp = cache.get('device_zscore_planes', {})
        if not native_2d and not self._max_mean_only(channels) and all(n in zp for _, n in channels):
            # this model's own channel set over the planes ts2d_project_coronal_modes normalised one by one: stacked in its channel order,
            # the non-zero box the union of its planes' boxes - the shape preprocess.py reads
            mine = [zp[n] for _, n in channels]
            input2d.device_zscore = {'norm': np.stack([p['norm'] for p in mine]), 'order': tuple(range(len(mine))),
                                     'stats': tuple(v for p in mine for v in p['stats']), 'shape': mine[0]['shape'],
                                     'box': (min(p['box'][0] for p in mine), max(p['box'][1] for p in mine),
                                             min(p['box'][2] for p in mine), max(p['box'][3] for p in mine))}
        # one preprocessing per distinct (channels, plan) of the case, shared by the sub-models (they run on threads: model.py takes the lock)
        import threading
        input2d.preprocess_cache = cache.setdefault('preprocessed', {'lock': threading.Lock(), 'items': {}})
        if rendered:
            input2d.xr_geometry = self.synthetic_xr
        return input, input2d, native_2d

    @staticmethod
    def _max_mean_only(channels) -> bool:
        return all(n.lower() in ('max', 'mip', 'mean', 'avg') for _, n in channels)

    def _project_modes_on_device(self, model, input: nrrd.Image, channels, cache: dict) -> bool:
        """A sub-model with a channel name beyond max / mean: ONE call of ``ts2d_project_coronal_modes`` for those of its names that the case
        has no device-normalised plane of yet (``cache['device_zscore_planes']``, shared by name across the sub-models like the projections).
        False - nothing taken - when a name is no device mode, the entry is missing, or it refused the volume (a non-finite sample, rays above
        the cap): the whole case then stays on the host branch."""
        from . import _lib, engine
        from .image import ProjectionDeviceRefused, _reorient_plan, device_projection_mode, project_coronal_gpu
        if cache.get('host_projection') or not engine.has_entry('ts2d_project_coronal_modes', tolerant=False) or input.dimension != 3:
            return False
        planes = cache.setdefault('device_zscore_planes', {})
        want = list(dict.fromkeys(n for _, n in channels if n not in planes))
        ny = input.size[_reorient_plan(input)[0][1]]
        if len(want) > _lib.PROJECT_MAX_MODES or any(device_projection_mode(n, ny) is None for _, n in channels):
            return False
        if want:
            try:
                pr = project_coronal_gpu(input, getattr(model._predictor.device, 'index', 0) or 0, zscore=True, modes=want)
            except ProjectionDeviceRefused:
                cache['host_projection'] = True
                return False
            for n in want:
                cache['projections'].setdefault(n, pr[n])
                planes[n] = pr['zscore'][n]
        return True

    class Result:
        def __init__(self, data: dict, device: Optional[int] = None):
            self.data = data
            self.device = device          # where save() renders the PNG visuals: a device index, or None for the host statement

        @property
        def models(self) -> List[str]:
            return sorted(self.data.get('models', {}).keys())

        def get_input(self, model: Optional[str] = None):
            return self.data.get('models', {}).get(model, {}).get('input') if model is not None else self.data.get('input')

        def get_segmentation(self, model: Optional[str] = None):
            return self.data.get('models', {}).get(model, {}).get('segmentation') if model is not None else self.data.get('segmentation')

        def get_probabilities(self, model: str):
            """float32 [K, *shape of the sub-model's 2-D input] of sub-model ``model`` (``predict(..., probabilities=True)``), else None."""
            return self.data.get('models', {}).get(model, {}).get('probabilities')

        def save_probabilities(self, dest: str, name: str = 'result', naming: str = 'group') -> List[str]:
            """One ``<name>-<group or model>.npz`` (``np.savez_compressed``, key ``probabilities``) per sub-model that has them."""
            assert naming in {'group', 'model'}
            os.makedirs(dest, exist_ok=True)
            written = []
            for key in self.models:
                prob = self.get_probabilities(key)
                if prob is not None:
                    written.append(os.path.join(dest, f"{name}-{(decompose_model_key(key)[1] or key) if naming == 'group' else key}.npz"))
                    np.savez_compressed(written[-1], probabilities=prob)
            return written

        def get_projection(self, channel: Optional[str] = None):
            pr = self.data.get('projections', {})
            return pr.get(channel) if channel is not None else pr

        def statistics(self, model: Optional[str] = None, channels='all', percentiles=()) -> Dict[str, dict]:
            """Per-label statistics (``statistics.label_statistics``: count, mm, box, centroid, and min / max / mean / std of the intensity
            under the label) of the merged segmentation (``model=None``) or of sub-model ``model``'s, against the projections of
            :meth:`get_projection` - all of them, or the channel names in ``channels``.  Computed on ``self.device`` (C-ABI
            ``ts2d_label_statistics``), from the host statement without one: the numbers are the same bit for bit.  ``percentiles`` (0 ... 100,
            at most 8) adds ``intensity[channel]['percentile'][repr(float(q))]``, the percentile of the channel under the label (50: the
            median; on the device by ``ts2d_label_percentiles``)."""
            seg = self.get_segmentation(model)
            if seg is None:
                raise ValueError(f"no segmentation for model {model!r}")
            pr = self.get_projection()
            want = list(pr) if isinstance(channels, str) and channels.strip().lower() == 'all' else [str(c) for c in _as_list(channels)]
            missing = [c for c in want if c not in pr]
            if missing:
                raise ValueError(f"no projection named {missing}; the result has {sorted(pr)}")
            spatial = tuple(seg.array.shape[:seg.dimension])
            images = {}
            for c in want:
                a = pr[c].array
                if a.shape != spatial and int(a.size) == int(np.prod(spatial)) and [s for s in a.shape if s > 1] == [s for s in spatial if s > 1]:
                    a = a.reshape(spatial)          # a collapsed segmentation against a projection that kept its unit axis
                images[c] = a
            if not len(percentiles):
                return label_statistics(seg, images, device=self.device)
            return label_statistics(seg, images, device=self.device, percentiles=percentiles)

        def save_statistics(self, dest: str, name: str = 'result', models='final', naming: str = 'group', percentiles=()) -> List[str]:
            """``<name>.statistics.json`` for the merged segmentation and ``<name>-<group or model>.statistics.json`` per sub-model, selected
            by ``models`` as in :meth:`save`: ``json.dump`` of :meth:`statistics` (with ``percentiles``) with sorted keys (None of an empty
            label is ``null``)."""
            assert naming in {'group', 'model'}
            mset = {str(t).strip().lower() for t in _as_list(models)}
            keys = []
            if {'all', 'final'} & mset and self.get_segmentation() is not None:
                keys.append(None)
            keys += [m for m in self.models if ('all' in mset or m.lower() in mset) and self.get_segmentation(m) is not None]
            os.makedirs(dest, exist_ok=True)
            written = []
            for key in keys:
                stem = name if key is None else f"{name}-{(decompose_model_key(key)[1] or key) if naming == 'group' else key}"
                stats = self.statistics(key, percentiles=percentiles) if len(percentiles) else self.statistics(key)
                written.append(dump_statistics(stats, os.path.join(dest, f"{stem}.statistics.json")))
            return written

        def components(self, model: Optional[str] = None, connectivity: str = 'full') -> Dict[str, dict]:
            """Per label its connected components (``components.label_components``: count, mm, how many pieces, the largest, every size and
            where each piece starts) of the merged segmentation (``model=None``) or of sub-model ``model``'s.  Computed on ``self.device``
            (C-ABI ``ts2d_label_components``), from the host statement without one: the numbers are the same."""
            from .components import label_components
            seg = self.get_segmentation(model)
            if seg is None:
                raise ValueError(f"no segmentation for model {model!r}")
            return label_components(seg, device=self.device, connectivity=connectivity)

        def cleaned(self, keep_largest: bool = False, min_size_mm: float = 0.0, connectivity: str = 'full', models='all') -> "TS2D.Result":
            """A NEW result whose segmentations are cleaned (``components.clean_components``: per label, ``keep_largest`` keeps the pieces
            of the largest size only, ``min_size_mm`` drops every piece below that area or volume): the merged segmentation and that of every
            sub-model ``models`` selects ('all', or model keys).  Input and projections are shared with this result, which stays untouched;
            with the defaults the new result holds equal bytes."""
            from .components import clean_components
            mset = {str(t).strip().lower() for t in _as_list(models)}

            def clean(seg):
                return clean_components(seg, device=self.device, connectivity=connectivity, keep_largest=keep_largest, min_size_mm=min_size_mm)[0]
            data = dict(self.data)
            if self.get_segmentation() is not None:
                data['segmentation'] = clean(self.get_segmentation())
            data['models'] = {m: dict(d) for m, d in self.data.get('models', {}).items()}
            for m, d in data['models'].items():
                if ('all' in mset or m.lower() in mset) and d.get('segmentation') is not None:
                    d['segmentation'] = clean(d['segmentation'])
            return type(self)(data, self.device)

        def morphology(self, op: str, radius_mm: float, labels='all', models='all') -> "TS2D.Result":
            """A NEW result whose segmentations are grown ('dilate'), shrunk ('erode'), opened or closed by ``radius_mm`` with an exact
            Euclidean disc (``morphology.label_morphology``; ``labels``: 'all' or label names - a segmentation is asked for those of them it
            has): the merged segmentation and that of every sub-model ``models`` selects ('all', or model keys).  Input and projections are
            shared with this result, which stays untouched; with ``radius_mm = 0`` the new result holds equal bytes."""
            from .image import get_annotation_labels
            from .morphology import label_morphology
            mset = {str(t).strip().lower() for t in _as_list(models)}
            wanted = None if (isinstance(labels, str) and labels == 'all') else {str(n) for n in _as_list(labels)}

            def work(seg):
                mine = 'all' if wanted is None else sorted(wanted & set(get_annotation_labels(seg)))
                return label_morphology(seg, op, radius_mm, device=self.device, labels=mine)[0]
            if wanted is not None:
                known = set()
                for seg in [self.get_segmentation()] + [d.get('segmentation') for d in self.data.get('models', {}).values()]:
                    if seg is not None:
                        known |= set(get_annotation_labels(seg))
                if wanted - known:
                    raise ValueError(f"morphology: labels {sorted(wanted - known)} are in no segmentation of this result")
            data = dict(self.data)
            if self.get_segmentation() is not None:
                data['segmentation'] = work(self.get_segmentation())
            data['models'] = {m: dict(d) for m, d in self.data.get('models', {}).items()}
            for m, d in data['models'].items():
                if ('all' in mset or m.lower() in mset) and d.get('segmentation') is not None:
                    d['segmentation'] = work(d['segmentation'])
            return type(self)(data, self.device)

        def save_components(self, dest: str, name: str = 'result', models='final', naming: str = 'group', connectivity: str = 'full') -> List[str]:
            """``<name>.components.json`` for the merged segmentation and ``<name>-<group or model>.components.json`` per sub-model, selected
            by ``models`` and named as in :meth:`save_statistics`: ``json.dump`` of :meth:`components` with sorted keys."""
            from .components import dump_components
            assert naming in {'group', 'model'}
            mset = {str(t).strip().lower() for t in _as_list(models)}
            keys = []
            if {'all', 'final'} & mset and self.get_segmentation() is not None:
                keys.append(None)
            keys += [m for m in self.models if ('all' in mset or m.lower() in mset) and self.get_segmentation(m) is not None]
            os.makedirs(dest, exist_ok=True)
            written = []
            for key in keys:
                stem = name if key is None else f"{name}-{(decompose_model_key(key)[1] or key) if naming == 'group' else key}"
                written.append(dump_components(self.components(key, connectivity), os.path.join(dest, f"{stem}.components.json")))
            return written

        def _xr_geometry(self, model: Optional[str] = None):
            """The ``xray.XRGeometry`` sub-model ``model`` was rendered under, None for a projected one.  The merged segmentation
            (``model=None``) has one when every sub-model has that one; a mix of rendered and projected sub-models has no grid of its own and is
            refused by name: score its sub-models one by one."""
            models = self.data.get('models', {})
            if model is not None:
                return models.get(model, {}).get('xr_geometry')
            found = {m: d.get('xr_geometry') for m, d in models.items()}
            with_xr = sorted(m for m, g in found.items() if g is not None)
            if not with_xr:
                return None
            if len(with_xr) != len(found) or any(found[m] != found[with_xr[0]] for m in with_xr):
                raise ValueError(f"the merged segmentation mixes sub-models on synthetic radiographs ({', '.join(with_xr)}) and on projections "
                                 f"({', '.join(sorted(set(found) - set(with_xr)))}): score each sub-model with model=<key>")
            return found[with_xr[0]]

        def _scored_pair(self, reference, model: Optional[str] = None):
            """(segmentation, reference on its grid) as :meth:`evaluate` and :meth:`confusion` score them: a 3-D label volume is reoriented,
            projected along the coronal axis and collapsed as the segmentation is, an already-2-D segmentation is taken as it is, and a
            reference that does not lie on the segmentation's grid raises ``ValueError`` with both extents."""
            from . import evaluate as ev
            seg = self.get_segmentation(model)
            if seg is None:
                raise ValueError(f"no segmentation for model {model!r}")
            ref = TS2D._as_image(reference)
            if ref.components == 1 and get_actual_dimension(ref) > 2 and get_actual_dimension(seg) <= 2:
                from .image import get_annotation_labels
                num = seg.components if seg.components > 1 else max([int(i['value']) for i in get_annotation_labels(seg).values()] or [1])
                geometry = self._xr_geometry(model)
                if geometry is not None:                   # a result on a synthetic radiograph: the reference goes through the same rays
                    from .xray import project_labels_xr
                    ref = project_labels_xr(ref, num, geometry, device=self.device)
                elif self.device is not None and ev.device_projects(ref):
                    ref = ev.project_labels_coronal_gpu(ref, num, self.device)
                else:
                    ref = ev.project_labels(reorient_image(ref, 'RAI'), num, 'coronal')
                if seg.dimension < 3:
                    ref = reduce_dimensions(ref)
            e_seg, e_ref = tuple(seg.array.shape[:seg.dimension]), tuple(ref.array.shape[:ref.dimension])
            if e_seg != e_ref or not np.allclose(seg.spacing, ref.spacing, rtol=1e-5, atol=1e-8):
                raise ValueError(f"the reference does not lie on the segmentation's grid: extent {e_ref} with spacing {tuple(ref.spacing)} against "
                                 f"extent {e_seg} with spacing {tuple(seg.spacing)}")
            return seg, ref

        def evaluate(self, reference, model: Optional[str] = None, tolerances=(2.0,), percentiles=(), average_distance: bool = False) -> Dict[str, dict]:
            """Scores of the merged segmentation (``model=None``) or of sub-model ``model``'s against ``reference`` (``evaluate.evaluate``:
            per label the counts, Dice, IoU, precision, recall and, for a 2-D result, surface Dice per tolerance in mm and the Hausdorff distance).
            On request, for a 2-D result: ``percentiles`` (0 ... 100, at most 8) adds ``hausdorff_percentile[repr(float(q))]``, the percentile
            Hausdorff distance (HD95 for 95), and ``average_distance=True`` adds ``asd_pred_to_ref``, ``asd_ref_to_pred``, ``assd`` and ``masd``,
            the average surface distances in mm; without them the result is what it always was.

            ``reference`` (an image or a path) is one of two things.  A 3-D label volume: it is reoriented and projected along the coronal axis
            with ``evaluate.project_labels`` (``num`` = the number of labels of that segmentation) - on ``self.device`` where the result has one
            and the entry serves the volume (C-ABI ``ts2d_project_labels_coronal``) - and collapsed as the result's segmentation is; label ``v``
            of the volume is component ``v - 1``, the convention ``statistics.label_statistics`` documents.  Or an already-2-D segmentation of
            the result's extent.  A shape or spacing mismatch raises ``ValueError`` with both extents.  Computed on ``self.device``, from the
            host statements without one: the numbers are the same bit for bit."""
            from . import evaluate as ev
            seg, ref = self._scored_pair(reference, model)
            return ev.evaluate(seg, ref, device=self.device, tolerances=tolerances, percentiles=percentiles, average_distance=average_distance)

        def save_evaluation(self, dest: str, name: str, reference, models='final', naming: str = 'group', tolerances=(2.0,), percentiles=(),
                            average_distance: bool = False) -> List[str]:
            """``<name>.evaluation.json`` for the merged segmentation and ``<name>-<group or model>.evaluation.json`` per sub-model, selected by
            ``models`` and named as in :meth:`save_statistics`: ``json.dump`` of :meth:`evaluate` against ``reference`` with sorted keys.
            ``percentiles`` and ``average_distance`` as in :meth:`evaluate`: the keys ``hausdorff_percentile``, ``asd_pred_to_ref``,
            ``asd_ref_to_pred``, ``assd`` and ``masd`` appear in the files only on request."""
            from .evaluate import dump_evaluation
            assert naming in {'group', 'model'}
            mset = {str(t).strip().lower() for t in _as_list(models)}
            keys = []
            if {'all', 'final'} & mset and self.get_segmentation() is not None:
                keys.append(None)
            keys += [m for m in self.models if ('all' in mset or m.lower() in mset) and self.get_segmentation(m) is not None]
            ref = TS2D._as_image(reference)
            os.makedirs(dest, exist_ok=True)
            written = []
            for key in keys:
                stem = name if key is None else f"{name}-{(decompose_model_key(key)[1] or key) if naming == 'group' else key}"
                written.append(dump_evaluation(self.evaluate(ref, key, tolerances, percentiles, average_distance), os.path.join(dest, f"{stem}.evaluation.json")))
            return written

        def confusion(self, reference, model: Optional[str] = None, top: int = 3) -> dict:
            """The confusion matrix of the merged segmentation (``model=None``) or of sub-model ``model``'s against ``reference``
            (``evaluate.confusion``: what every structure of the reference was taken for - rows the reference, columns the prediction, the
            margins, per label the ``top`` classes it was predicted as and predicted from).  ``reference`` is prepared exactly as in
            :meth:`evaluate`.  Computed on ``self.device`` (C-ABI ``ts2d_label_confusion``), from the host statement without one: the integers
            are the same."""
            from . import evaluate as ev
            seg, ref = self._scored_pair(reference, model)
            return ev.confusion(seg, ref, device=self.device, top=top)

        def save_confusion(self, dest: str, name: str, reference, models='final', naming: str = 'group', top: int = 3) -> List[str]:
            """``<name>.confusion.json`` for the merged segmentation and ``<name>-<group or model>.confusion.json`` per sub-model, selected by
            ``models`` and named as in :meth:`save_evaluation`: ``json.dump`` of :meth:`confusion` against ``reference`` with sorted keys."""
            from .evaluate import dump_evaluation
            assert naming in {'group', 'model'}
            mset = {str(t).strip().lower() for t in _as_list(models)}
            keys = []
            if {'all', 'final'} & mset and self.get_segmentation() is not None:
                keys.append(None)
            keys += [m for m in self.models if ('all' in mset or m.lower() in mset) and self.get_segmentation(m) is not None]
            ref = TS2D._as_image(reference)
            os.makedirs(dest, exist_ok=True)
            written = []
            for key in keys:
                stem = name if key is None else f"{name}-{(decompose_model_key(key)[1] or key) if naming == 'group' else key}"
                written.append(dump_evaluation(self.confusion(ref, key, top), os.path.join(dest, f"{stem}.confusion.json")))
            return written

        def save(self, dest: str, name: str = 'result', ext: str = 'nrrd', models='final', targets='all', content: str = 'all',
                 naming: str = 'group'):
            assert ext.lower() != 'png', "PNG is not a valid export format for the 'file' content type."
            """Reference tool.py:235-311.  ``content``: 'file' writes ``<base>.<ext>``, ``<base>.seg.<ext>`` and ``<name>_<channel>.<ext>``;
            'visual' their PNG twins (``<base>.png`` - ``<base>-ch<i>.png`` per channel of a multi-channel input -, ``<base>.seg.png``,
            ``<name>_<channel>.png``: ``create_visual`` along the coronal axis, on ``self.device``); 'all' both.  Returns every path written."""
            assert naming in {'group', 'model'} and content in {'file', 'visual', 'all'}
            kinds = {'file', 'visual'} if content == 'all' else {content}
            mset = {str(t).strip().lower() for t in _as_list(models)}
            keys: set = set()
            if 'all' in mset:
                keys |= set(self.models) | {None}
            if 'final' in mset:
                keys |= {None}
            keys |= {m for m in self.models if m.lower() in mset}
            tset = {str(t).strip().lower() for t in _as_list(targets)}

            def fname(base, key):
                if key is not None and naming == 'group':
                    return f"{base}-{decompose_model_key(key)[1]}"
                return base if key is None else f"{base}-{key}"

            os.makedirs(dest, exist_ok=True)
            written = []

            def write_file(img, stem):
                if 'file' in kinds:
                    written.append(os.path.join(dest, f"{stem}.{ext}"))
                    nrrd.write(img, written[-1], True)

            def write_visual(img, stem, **how):
                written.append(os.path.join(dest, f"{stem}.png"))
                png.write(create_visual(img, device=self.device, **how), written[-1])

            if {'all', 'input'} & tset:
                for key in keys:
                    img = self.get_input(key)
                    if img is not None:
                        base = fname(name, key)
                        write_file(img, base)
                        if 'visual' in kinds:
                            chs = split_channels(img)
                            for i, ch in enumerate(chs):
                                write_visual(ch, base if len(chs) == 1 else f"{base}-ch{i}", labels=False, axis='coronal')
            if {'all', 'segmentation'} & tset:
                for key in keys:
                    img = self.get_segmentation(key)
                    if img is not None:
                        write_file(img, f"{fname(name, key)}.seg")
                        if 'visual' in kinds:
                            write_visual(img, f"{fname(name, key)}.seg", labels=True, axis='coronal')
            if {'all', 'projection'} & tset:
                for channel, img in self.get_projection().items():
                    write_file(img, f"{name}_{channel}")
                    if 'visual' in kinds:
                        write_visual(img, f"{name}_{channel}")
            return written
