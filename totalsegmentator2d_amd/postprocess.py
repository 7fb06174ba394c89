"""nnU-Net's postprocessing of a decided label map: the plan ``nnUNetv2_find_best_configuration`` determines and stores beside a trained
model, applied between ``convert_predicted_logits_to_segmentation_with_correct_shape`` and the image (export.py).

[UPSTREAM-RECALL] The one function such a plan holds is ``remove_all_but_largest_component_from_segmentation(segmentation,
labels_or_regions, background_label=0)``, first over the whole foreground and then per label or region, wherever it improved the
cross-validation Dice.  nnunetv2, acvl_utils and skimage are not importable here, so the definition below is upstream's as recalled, and
:func:`keep_largest_components_statement` IS this project's definition of the step: the host route, and the oracle the device kernels
(csrc/kernels_post_cc.h, C-ABI ts2d_keep_largest_components) are held to byte for byte.

A step ``(labels_or_regions, background_label)`` on ``seg`` uint8 [Z, H, W] (a 2-D case: Z = 1):

1. ``mask`` = the voxels whose value is any label named anywhere in ``labels_or_regions`` (a region contributes all of its labels);
2. its components under FULL connectivity - 26 neighbours, 8 at Z = 1: skimage's ``label(connectivity=None)``;
3. every component of the largest size stays (ties all stay);
4. ``seg[mask & ~keep] = background_label``;
5. an empty mask changes nothing.

Steps run in order, each on the output of the one before.  Only the segmentation changes: probabilities are left as they are, upstream
postprocesses the written label maps.  An axis permutation and the crop box preserve the components, so the step runs on the final array.
"""
from __future__ import annotations

import glob
import json
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

FUNCTION_NAME = 'remove_all_but_largest_component_from_segmentation'
MAX_DEVICE_VOXELS = 2 ** 31 - 1          # the device entry's indices are int32 (include/ts2d_engine.h)
STAT_NAMES = ('mask_voxels', 'components', 'largest', 'removed')


def _normalise_step(step, where: str) -> Tuple[Tuple[int, ...], int]:
    """One step -> (sorted tuple of the distinct labels it names, background label), validated."""
    if isinstance(step, dict):
        lor, bg = step.get('labels_or_regions'), step.get('background_label', 0)
    elif isinstance(step, (list, tuple)) and len(step) == 2:
        lor, bg = step
    else:
        raise ValueError(f"{where}: a step is (labels_or_regions, background_label), found {step!r}")
    if isinstance(lor, (int, np.integer)) and not isinstance(lor, bool):
        lor = [lor]
    if not isinstance(lor, (list, tuple)) or len(lor) == 0:
        raise ValueError(f"{where}: labels_or_regions must be a non-empty list, found {lor!r}")
    labels = []
    for entry in lor:
        region = entry if isinstance(entry, (list, tuple)) else [entry]
        if len(region) == 0:
            raise ValueError(f"{where}: an empty region in {lor!r}")
        for v in region:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{where}: a label must be an int, found {v!r}")
            if not 0 <= int(v) <= 255:
                raise ValueError(f"{where}: label {int(v)} is outside 0..255 (the map is uint8)")
            labels.append(int(v))
    if bg is None:
        bg = 0
    if isinstance(bg, bool) or not isinstance(bg, (int, np.integer)) or not 0 <= int(bg) <= 255:
        raise ValueError(f"{where}: background_label must be an int in 0..255, found {bg!r}")
    return tuple(sorted(set(labels))), int(bg)


class PostprocessingPlan:
    """An ordered list of steps ``(labels, background_label)``, labels a sorted tuple of ints in 0..255 (a region is flattened into the
    step's union: the mask is all a step reads of it)."""

    def __init__(self, steps: Sequence):
        if isinstance(steps, PostprocessingPlan):
            steps = steps.steps
        if not isinstance(steps, (list, tuple)) or len(steps) == 0:
            raise ValueError(f"a postprocessing plan is a non-empty list of (labels_or_regions, background_label), found {steps!r}")
        self.steps: Tuple[Tuple[Tuple[int, ...], int], ...] = tuple(_normalise_step(s, f'step {i}') for i, s in enumerate(steps))

    def __len__(self):
        return len(self.steps)

    def __eq__(self, other):
        return isinstance(other, PostprocessingPlan) and self.steps == other.steps

    def __repr__(self):
        return f'PostprocessingPlan({list(self.steps)!r})'

    @property
    def compiled(self):
        """What the device entry takes: ``(tables, backgrounds)`` - uint8 [n_steps, 256] with 1 at every label of the step, uint8 [n_steps]."""
        tables = np.zeros((len(self.steps), 256), dtype=np.uint8)
        for k, (labels, _) in enumerate(self.steps):
            tables[k, list(labels)] = 1
        return tables, np.array([bg for _, bg in self.steps], dtype=np.uint8)


def as_plan(plan) -> Optional[PostprocessingPlan]:
    return None if plan is None else plan if isinstance(plan, PostprocessingPlan) else PostprocessingPlan(plan)


def keep_largest_components_statement(seg, plan):
    """The definition of the step (module docstring) in numpy and scipy: ``scipy.ndimage.label`` with the full 3 x 3 x 3 structure,
    ``np.bincount`` of its labels, every component of the largest size kept.  ``seg``: uint8 [Z, H, W] or [H, W] (Z = 1).  Returns
    ``(seg_out, stats)``: a new array of the same shape, and int64 [n_steps, 4] = (mask voxels, components, largest size, voxels
    removed) per step."""
    from scipy import ndimage
    plan = as_plan(plan)
    src = np.asarray(seg)
    if src.dtype != np.uint8 or src.ndim not in (2, 3):
        raise ValueError(f"expected a uint8 label map [Z, H, W] or [H, W], found {src.dtype} {src.shape}")
    out = np.array(src, dtype=np.uint8, order='C')
    vol = out.reshape(((1,) + out.shape)[-3:])
    tables, backgrounds = plan.compiled
    stats = np.zeros((len(plan), 4), dtype=np.int64)
    structure = np.ones((3, 3, 3), dtype=bool)
    for k in range(len(plan)):
        mask = tables[k][vol].astype(bool)
        n_mask = int(mask.sum())
        if n_mask == 0:
            continue
        lab, n = ndimage.label(mask, structure=structure)
        sizes = np.bincount(lab.ravel(), minlength=n + 1)
        sizes[0] = 0                                             # (label 0 is everything outside the mask)
        largest = int(sizes.max())
        drop = mask & (sizes < largest)[lab]
        vol[drop] = backgrounds[k]
        stats[k] = (n_mask, n, largest, int(drop.sum()))
    return out, stats


def load_postprocessing(path) -> PostprocessingPlan:
    """The plan of a trained model.  ``path``: a plain list of ``(labels_or_regions, background_label)`` pairs (or a plan), a
    ``postprocessing.json`` file, or a trained-model folder - there ``postprocessing.json`` directly, else the first (sorted) of
    ``crossval_results_folds_*/postprocessing.json``.

    The file's form is RECALLED, NOT VERIFIED [UPSTREAM-RECALL: nnUNetv2_find_best_configuration / determine_postprocessing]:
    ``{"postprocessing_fns": [name, ...], "postprocessing_kwargs": [{"labels_or_regions": ..., "background_label": ...}, ...]}``, one
    kwargs dict per function name.  Any function other than ``remove_all_but_largest_component_from_segmentation`` is refused by name.
    ``postprocessing.pkl`` is never read: it names upstream functions by module path, and unpickling it would import them."""
    if isinstance(path, PostprocessingPlan):
        return path
    if isinstance(path, (list, tuple)):
        return PostprocessingPlan(path)
    path = os.fspath(path)
    if os.path.isdir(path):
        found = [os.path.join(path, 'postprocessing.json')] if os.path.isfile(os.path.join(path, 'postprocessing.json')) \
            else sorted(glob.glob(os.path.join(path, 'crossval_results_folds_*', 'postprocessing.json')))
        if not found:
            raise FileNotFoundError(f"no postprocessing.json in {path} or its crossval_results_folds_* folders")
        path = found[0]
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or 'postprocessing_fns' not in doc or 'postprocessing_kwargs' not in doc:
        raise ValueError(f"{path}: expected the keys postprocessing_fns and postprocessing_kwargs")
    fns, kwargs = doc['postprocessing_fns'], doc['postprocessing_kwargs']
    if not isinstance(fns, list) or not isinstance(kwargs, list) or len(fns) != len(kwargs):
        raise ValueError(f"{path}: postprocessing_fns and postprocessing_kwargs must be lists of one length")
    for name in fns:
        if str(name).rsplit('.', 1)[-1] != FUNCTION_NAME or not isinstance(name, str):
            raise ValueError(f"{path}: postprocessing function {name!r} is not supported (only {FUNCTION_NAME})")
    if not fns:
        raise ValueError(f"{path}: the plan has no steps")
    return PostprocessingPlan([dict(kw) if isinstance(kw, dict) else kw for kw in kwargs])


def _device_entry():
    """``engine.keep_largest_components`` where the engine library has the entry, else None (no library built, or one built before it)."""
    from . import engine
    return engine.keep_largest_components if engine.has_keep_largest_components() else None


def apply_postprocessing(seg, plan, device: Optional[int] = None):
    """``plan`` on ``seg`` (uint8 [Z, H, W] or [H, W]).  Returns ``(seg_out, stats, route)``, route 'device' or 'host': the device entry
    where ``device`` is given, the library has it and the case is inside its limits (at most 2^31 - 1 voxels), else
    :func:`keep_largest_components_statement` - also when the device gives up (a bounded loop at its cap: TS2D_CC_GIVE_UP).  Both routes
    give the same bytes and counters."""
    plan = as_plan(plan)
    src = np.asarray(seg)
    if device is not None and src.dtype == np.uint8 and src.ndim in (2, 3) and 0 < src.size <= MAX_DEVICE_VOXELS:
        entry = _device_entry()
        if entry is not None:
            tables, backgrounds = plan.compiled
            out, stats, status = entry(src, tables, backgrounds, device=int(device))
            if not status:
                return out, stats, 'device'
    out, stats = keep_largest_components_statement(src, plan)
    return out, stats, 'host'
