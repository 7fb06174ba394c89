"""The label convention of a ``dataset.json``: which of nnU-Net's three conventions a model was trained under, how many heads its
network has, and what the export paints.

=================  ==========================================  =================================================  ===================
kind               ``dataset.json``                            heads                                              export
=================  ==========================================  =================================================  ===================
``'multilabel'``   ``"multilabel": true`` (the ts2d fork)      one per foreground label                           sigmoid > 0.5 per head, K planes
``'labelmap'``     integer label values                        ``len(labels)`` (background is head 0)             argmax over the heads, one plane
``'regions'``      label values are lists +                    one per foreground region                          sigmoid > 0.5 per region, painted in
                   ``regions_class_order``                                                                         order into one plane
=================  ==========================================  =================================================  ===================

nnunetv2 is not installed here, so the region rules restate its ``LabelManager`` from memory [UPSTREAM-RECALL]:
``has_regions`` is true when any label value is a list or tuple with more than one entry; the foreground regions are the label values
in ``dataset.json`` order without the key ``"ignore"`` and without every entry whose value is 0 or a list whose unique values are
``[0]``; ``regions_class_order`` is required and holds one class value per foreground region; the network has one head per foreground
region and the inference non-linearity is the sigmoid.  The class values go into a uint8 plane here, so they must lie in 0..255.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple


class LabelConvention(NamedTuple):
    kind: str                                  # 'multilabel' | 'labelmap' | 'regions'
    n_heads: int                               # output channels of the network
    class_order: Optional[Tuple[int, ...]]     # 'regions': the class value head i paints; else None
    names: Dict[int, str]                      # class value -> name, for the annotation metadata (background excluded)


def _is_multilabel(dataset_json: dict) -> bool:
    return bool(dataset_json.get('multilabel', dataset_json.get('multiclass', False)))


def _is_region(value) -> bool:
    return isinstance(value, (list, tuple)) and len(value) > 1


def label_convention(dataset_json: dict) -> LabelConvention:
    """``dataset.json`` -> :class:`LabelConvention`.  Raises ValueError, with the reason, for region labels without
    ``regions_class_order``, a ``regions_class_order`` whose length is not the number of foreground regions, and a class value outside
    0..255."""
    labels = dataset_json.get('labels', {})
    multilabel = _is_multilabel(dataset_json)
    if not any(_is_region(v) for v in labels.values()):
        # the two integer conventions, exactly as before the region-based one existed
        names = {int(v): k for k, v in labels.items() if k != 'background'}
        n_fg = len([k for k, v in labels.items() if k != 'background' and v != 0])
        return LabelConvention('multilabel' if multilabel else 'labelmap', n_fg if multilabel else len(labels), None, names)
    if multilabel:
        raise ValueError("dataset.json is marked multilabel and has region labels (lists of label values): the two conventions exclude each other")
    regions = []
    for name, value in labels.items():
        if name == 'ignore':
            continue
        values = {int(v) for v in value} if isinstance(value, (list, tuple)) else {int(value)}
        if values == {0}:
            continue                      # background, spelled 0 or [0]
        regions.append(name)
    order = dataset_json.get('regions_class_order')
    if order is None:
        raise ValueError(f"dataset.json has region labels ({', '.join(regions)}) but no regions_class_order: a region-based model needs one "
                         f"class value per foreground region")
    order = tuple(int(c) for c in order)
    if len(order) != len(regions):
        raise ValueError(f"regions_class_order has {len(order)} entries for {len(regions)} foreground regions ({', '.join(regions)})")
    bad = [c for c in order if c < 0 or c > 255]
    if bad:
        raise ValueError(f"regions_class_order holds the class value {bad[0]}, outside 0..255: the segmentation is one uint8 plane")
    # a class value painted by several regions carries the name of the last one, as its pixels do; 0 is background whoever paints it
    names = {c: name for c, name in zip(order, regions) if c != 0}
    return LabelConvention('regions', len(regions), order, names)
