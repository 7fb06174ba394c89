"""``ts2d`` command line (reference ``ts2d/main.py:10-115``): same flags, same output file names."""
from __future__ import annotations

import math
import os
from glob import glob

from .tool import TS2D
from .zoo import DEFAULT_MODEL


_KNOWN_EXT = ('nrrd', 'nii', 'nii.gz', 'mha', 'mhd')     # what the reference CLI accepts (ts2d/main.py:25)
_READABLE_EXT = ('nrrd',)                                 # what this build can read (no SimpleITK / nibabel)


def _check_case(path: str):
    """(case name, path) for one input file, or a ValueError / FileNotFoundError saying why it is not a case."""
    if not os.path.isfile(path):
        if not os.path.exists(path):
            raise FileNotFoundError(f"Source file does not exist: {path}")
        raise ValueError(f"Source is not a regular file: {path}")
    name, dot, ext = os.path.basename(path).partition('.')           # case name = up to the FIRST dot ('a.nii.gz' -> 'a')
    if not dot:
        raise ValueError(f"Source file does not have an extension: {os.path.basename(path)}")
    if ext not in _KNOWN_EXT:
        raise ValueError(f"Unsupported file extension: {ext} in {os.path.basename(path)}")
    if ext not in _READABLE_EXT:
        raise ValueError(f"only NRRD input is implemented in the MI355X build (no SimpleITK): {os.path.basename(path)}")
    return name, path


def _enumerate_cases(src: str):
    """A single file must be a valid case (its error propagates); a directory contributes every file that is one and silently
    skips the rest - the behaviour of the reference CLI (ts2d/main.py:10-32), in sorted order."""
    if not os.path.isdir(src):
        return [_check_case(src)]
    cases = []
    for path in sorted(glob(os.path.join(src, "*.*"))):
        try:
            cases.append(_check_case(path))
        except (ValueError, FileNotFoundError):
            pass
    return cases


def _references(reference, cases, src_is_dir: bool) -> dict:
    """case name -> reference file of ``--reference``: a file serves a single input; in a directory the reference of case ``<case>.nrrd`` is the
    file of the same name, and a case without one is an error that names it (before anything is predicted)."""
    if reference is None:
        return {}
    if os.path.isdir(reference):
        found = {name: os.path.join(reference, os.path.basename(path)) for name, path in cases}
        missing = [name for name, ref in found.items() if not os.path.isfile(ref)]
        if missing:
            raise FileNotFoundError(f"No reference for case{'s' if len(missing) != 1 else ''} {', '.join(missing)} in {reference} "
                                    f"(expected {', '.join(os.path.basename(found[n]) for n in missing)})")
        return found
    if not os.path.isfile(reference):
        raise FileNotFoundError(f"Reference does not exist: {reference}")
    if src_is_dir or len(cases) != 1:
        raise ValueError(f"A reference file serves a single input; for the {len(cases)} cases of a directory give a directory of references")
    return {cases[0][0]: reference}


def ts2d_run(src: str, dest: str, model: str = None, use_remote: bool = True, fetch_remote: bool = True, collapse: bool = False,
             visualize: bool = True, save_all: bool = False, silent: bool = False, models=None, batch_cases: int = 1, save_probabilities: bool = False,
             statistics: bool = False, reference: str = None, hausdorff_percentiles=(), average_distance: bool = False,
             statistics_percentiles=(), keep_largest: bool = False, min_component_mm: float = 0.0, components: bool = False,
             component_connectivity: str = 'full', confusion: bool = False, synthetic_xr=None, morphology=None, morphology_labels='all'):
    """``morphology``: None, or ``(op, radius_mm)`` with op 'dilate', 'erode', 'open' or 'close' - ``Result.morphology`` of every result, on
    ``morphology_labels``, BEFORE the component clean-up.  ``synthetic_xr``: an ``xray.XRGeometry`` (or True) switches the synthetic radiograph of ``TS2D`` on; None: the call of before."""
    model = DEFAULT_MODEL if model is None else model
    content = 'all' if visualize else 'file'
    which = 'all' if save_all else 'final'
    log = (lambda *a: None) if silent else print
    log("TS2D is a research tool. It is NOT validated for clinical use and should NOT be used for medical diagnosis or treatment.")
    stat_kw = {'percentiles': tuple(statistics_percentiles)} if len(statistics_percentiles) else {}      # without them: the call of before

    def tidy(res):          # morphology, then the clean-up, both before a result is saved, measured or scored; without their flags the result is the one predicted
        if morphology is not None:
            res = res.morphology(morphology[0], morphology[1], labels=morphology_labels)
        if keep_largest or min_component_mm > 0:
            res = res.cleaned(keep_largest=keep_largest, min_size_mm=min_component_mm, connectivity=component_connectivity)
        return res
    xr_kw = {} if synthetic_xr is None else {'synthetic_xr': synthetic_xr}
    with TS2D(key=model, use_remote=use_remote, fetch_remote=fetch_remote, models=models, **xr_kw) as ts:
        cases = list(_enumerate_cases(src))
        references = _references(reference, cases, os.path.isdir(src))
        log(f"Predicting {len(cases)} case{'s' if len(cases) != 1 else ''}")
        if batch_cases > 1:
            # groups of `batch_cases` cases share one engine batch per sub-model (TS2D.predict_many); same files, same log lines per case
            for g0 in range(0, len(cases), batch_cases):
                group = cases[g0:g0 + batch_cases]
                for i, (name, _) in enumerate(group):
                    log(f"[{g0 + i + 1}/{len(cases)}] Processing: {name}")
                for (name, _), res in zip(group, ts.predict_many([path for _, path in group], collapse=collapse, max_cases=batch_cases,
                                                                  probabilities=save_probabilities)):
                    res = tidy(res)
                    res.save(dest=dest, name=name, models=which, content=content, targets=['segmentation', 'projection'])
                    res.save_probabilities(dest, name)
                    if statistics:
                        res.save_statistics(dest, name, models=which, **stat_kw)
                    if components:
                        res.save_components(dest, name, models=which, connectivity=component_connectivity)
                    if references:
                        res.save_evaluation(dest, name, references[name], percentiles=hausdorff_percentiles, average_distance=average_distance)
                        if confusion:
                            res.save_confusion(dest, name, references[name])
            return
        for i, (name, path) in enumerate(cases):
            log(f"[{i + 1}/{len(cases)}] Processing: {name}")
            res = tidy(ts.predict(path, collapse=collapse, probabilities=save_probabilities))
            res.save(dest=dest, name=name, models=which, content=content, targets=['segmentation', 'projection'])
            res.save_probabilities(dest, name)
            if statistics:
                res.save_statistics(dest, name, models=which, **stat_kw)
            if components:
                res.save_components(dest, name, models=which, connectivity=component_connectivity)
            if references:
                res.save_evaluation(dest, name, references[name], percentiles=hausdorff_percentiles, average_distance=average_distance)
                if confusion:
                    res.save_confusion(dest, name, references[name])


def ts2d_entry_point(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="Runs TotalSegmentator2D (TS2D) on images or directories of images (MI355X engine).")
    p.add_argument("--src", "-i", "--input", type=str, required=True, help="Input image file or directory (nrrd)")
    p.add_argument("--dest", "-o", "--output", type=str, required=True, help="Output directory for results.")
    p.add_argument("--model", type=str, default=None, help=f"Model key for prediction, defaults to '{DEFAULT_MODEL}'.")
    p.add_argument("--no-remote", action="store_true", help="Disable remote model download (always the case here).")
    p.add_argument("--no-fetch", action="store_true", help="Do not fetch model URLs (always the case here).")
    p.add_argument("--collapse", action="store_true", help="Collapse projected images to 2D.")
    p.add_argument("--visualize", action="store_true", help="Visualize the results as PNG images.")
    p.add_argument("--save-all", action="store_true", help="Also save results for each individual model.")
    p.add_argument("--silent", action="store_true", help="Hides any unnecessary output.")
    p.add_argument("--batch-cases", type=int, default=1, help="Cases of a directory that share one engine batch per sub-model (1: one case at a time). "
                   "A case's result does not depend on the other cases of its batch.")
    p.add_argument("--save-probabilities", action="store_true", help="Also write the probabilities of every sub-model: one "
                   "<case>-<group>.npz (key 'probabilities', float32 [K, *shape of the sub-model's 2-D input]) per sub-model.")
    p.add_argument("--statistics", action="store_true", help="Also write <case>.statistics.json: per label count, mm, bounding box, centroid and "
                   "min / max / mean / std of every projection under it (with --save-all one <case>-<group>.statistics.json per sub-model too).")
    p.add_argument("--statistics-percentile", type=float, action="append", default=None, metavar="Q", help="With --statistics: also write per label "
                   "and projection percentile[Q], the Q-th percentile of the projection under the label (50: the median), Q in 0 ... 100; may be "
                   "given up to 8 times.")
    p.add_argument("--reference", type=str, default=None, help="Score every result against a reference and write <case>.evaluation.json (per label "
                   "Dice, IoU, precision, recall, surface Dice at 2 mm, Hausdorff distance): a 3-D label volume (label v = segment v) or a 2-D "
                   "segmentation; a file for a single input, or a directory that holds a file of the same name for every case.")
    p.add_argument("--hausdorff-percentile", type=float, action="append", default=None, metavar="Q", help="With --reference: also write per label "
                   "hausdorff_percentile[Q], the Q-th percentile Hausdorff distance in mm (95: HD95), Q in 0 ... 100; may be given up to 8 times.")
    p.add_argument("--average-distance", action="store_true", help="With --reference: also write per label the average surface distances in mm: "
                   "asd_pred_to_ref, asd_ref_to_pred, assd (both borders pooled) and masd (the mean of the two).")
    p.add_argument("--confusion", action="store_true", help="With --reference: also write <case>.confusion.json, the confusion matrix of the result "
                   "against the reference (rows the reference, columns the prediction; per label what it was predicted as and predicted from).")
    p.add_argument("--keep-largest", action="store_true", help="Clean the result before it is saved, measured or scored: of every label only the "
                   "connected components of the largest size stay.")
    p.add_argument("--min-component-mm", type=float, default=0.0, metavar="A", help="Clean the result before it is saved, measured or scored: every "
                   "connected component of a label below A (an area or volume in the unit of mm of the statistics) is removed; A >= 0.")
    p.add_argument("--components", action="store_true", help="Also write <case>.components.json: per label how many connected components it has, "
                   "their sizes and where each starts (with --save-all one <case>-<group>.components.json per sub-model too).")
    p.add_argument("--component-connectivity", choices=("full", "faces"), default=None, help="With --keep-largest, --min-component-mm or --components: "
                   "which neighbours connect, full (8 / 26, the default) or faces (4 / 6).")
    p.add_argument("--grow", type=float, default=None, metavar="MM", help="Grow every label by MM (an exact Euclidean disc in the spacing of the "
                   "result) before the component clean-up and before the result is saved, measured or scored.  At most one of --grow, --shrink, "
                   "--open and --close.")
    p.add_argument("--shrink", type=float, default=None, metavar="MM", help="Shrink every label by MM (a label at the image edge is not eaten from that edge).")
    p.add_argument("--open", type=float, default=None, metavar="MM", help="Open every label by MM: shrink, then grow - thin bridges and specks go.")
    p.add_argument("--close", type=float, default=None, metavar="MM", help="Close every label by MM: grow, then shrink - pin-holes and gaps fill.")
    p.add_argument("--morphology-labels", type=str, default=None, metavar="NAME[,NAME...]", help="With --grow, --shrink, --open or --close: only "
                   "these labels are changed; the others stay as they are (in a label map: obstacles).")
    p.add_argument("--synthetic-xr", action="store_true", help="Render a synthetic radiograph of a 3-D input for every model channel named xr, xray "
                   "or x-ray (a cone beam along the coronal axis; the line integral of the density in mm of water), and score a 3-D --reference "
                   "through the same rays.")
    p.add_argument("--xr-source-detector", type=float, default=None, metavar="MM", help="With --synthetic-xr: source-to-detector distance (1800).")
    p.add_argument("--xr-source-center", type=float, default=None, metavar="MM", help="With --synthetic-xr: source-to-volume-centre distance (1500).")
    p.add_argument("--xr-view", choices=("ap", "pa"), default=None, help="With --synthetic-xr: the source in front of the patient (ap, the default) "
                   "or behind (pa).")
    p.add_argument("--xr-parallel", action="store_true", help="With --synthetic-xr: parallel rays instead of a cone beam.")
    a = p.parse_args(argv)
    xr_kw = {}
    if a.synthetic_xr:
        from .xray import XRGeometry
        given = {'source_detector_mm': a.xr_source_detector, 'source_center_mm': a.xr_source_center, 'view': a.xr_view,
                 'parallel': True if a.xr_parallel else None}
        xr_kw = {'synthetic_xr': XRGeometry(**{k: v for k, v in given.items() if v is not None})}
    elif a.xr_source_detector is not None or a.xr_source_center is not None or a.xr_view is not None or a.xr_parallel:
        p.error("--xr-source-detector, --xr-source-center, --xr-view and --xr-parallel shape the synthetic radiograph: give --synthetic-xr")
    if a.batch_cases < 1:
        p.error("--batch-cases must be at least 1")
    if (a.hausdorff_percentile or a.average_distance) and a.reference is None:
        p.error("--hausdorff-percentile and --average-distance score against a reference: give --reference")
    if a.confusion and a.reference is None:
        p.error("--confusion compares against a reference: give --reference")
    if a.statistics_percentile and not a.statistics:
        p.error("--statistics-percentile adds to the statistics: give --statistics")
    if a.statistics_percentile and (len(a.statistics_percentile) > 8 or any(not (math.isfinite(q) and 0.0 <= q <= 100.0) for q in a.statistics_percentile)):
        p.error("--statistics-percentile: at most 8 values, each in 0 ... 100")
    if not (math.isfinite(a.min_component_mm) and a.min_component_mm >= 0.0):
        p.error("--min-component-mm must be a number >= 0")
    clean_kw = {}
    if a.keep_largest or a.min_component_mm > 0 or a.components:          # without the flags: the call of before
        clean_kw = {'keep_largest': a.keep_largest, 'min_component_mm': a.min_component_mm, 'components': a.components,
                    'component_connectivity': a.component_connectivity or 'full'}
    elif a.component_connectivity is not None:
        p.error("--component-connectivity chooses how components connect: give --keep-largest, --min-component-mm or --components")
    morph_kw = {}
    given = [(op, mm) for op, mm in (('dilate', a.grow), ('erode', a.shrink), ('open', a.open), ('close', a.close)) if mm is not None]
    if len(given) > 1:
        p.error("--grow, --shrink, --open and --close: at most one per run")
    if given:
        if not (math.isfinite(given[0][1]) and given[0][1] >= 0.0):
            p.error("--grow, --shrink, --open and --close take a number of mm >= 0")
        morph_kw = {'morphology': given[0]}
        if a.morphology_labels is not None:
            names = [n.strip() for n in a.morphology_labels.split(',') if n.strip()]
            if not names:
                p.error("--morphology-labels names no label")
            morph_kw['morphology_labels'] = names
    elif a.morphology_labels is not None:
        p.error("--morphology-labels chooses the labels of a morphology step: give --grow, --shrink, --open or --close")
    ts2d_run(src=a.src, dest=a.dest, model=a.model, use_remote=not a.no_remote, fetch_remote=not a.no_fetch, collapse=a.collapse,
             visualize=a.visualize, save_all=a.save_all, silent=a.silent, batch_cases=a.batch_cases, save_probabilities=a.save_probabilities,
             statistics=a.statistics, reference=a.reference, hausdorff_percentiles=tuple(a.hausdorff_percentile or ()),
             average_distance=a.average_distance, **({'statistics_percentiles': tuple(a.statistics_percentile)} if a.statistics_percentile else {}), **clean_kw,
             **({'confusion': True} if a.confusion else {}), **xr_kw, **morph_kw)          # without the flags: the call of before


if __name__ == '__main__':
    ts2d_entry_point()
