"""Per-case wall time of a LABEL-MAP model (the ordinary nnU-Net head: one head per label, background at 0, export = resample the logits
back, then the argmax over the heads): the host route (K float16 planes to the host, scipy order 1 per plane where the case is off the
plan spacing, ``astype(float32).argmax(0)``; a fold ensemble adds numpy's half sum and division: ``device_labelmap = False``) against
the device route (C-ABI ts2d_ensemble_predict_tiled_labelmap: every fold in one engine call, the mean on the device, resample-back and
argmax in one kernel, csrc/kernels_labelmap.h, ONE uint8 plane to the host).  One canonical sub-model (K = 18 heads, synthetic weights
per fold) with F in {1, 3}; the three off-spacing geometries of scripts/gpu_resampled_case.py and one case on the plan spacing, every
case its own image object with its own pixels.  HIPModel.apply: median of N cases after warm-up; HIPModel.apply_batch: ms per case over
GROUPS groups of 8 distinct cases.  Stage spans on the host clock (preprocess / predict / export; the median over the cases, the cases
of one apply_batch share the predict span of their group).
On a checkout that has no device route (the switch is simply absent) the host route alone runs and is reported: the baseline to run
back to back with this tree on the same box.

    timeout -k 10 900 python scripts/gpu_labelmap_case.py [N=10] [GROUPS=2] > profiles/r15_labelmap_case.txt     # exit status 0 = complete"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from totalsegmentator2d_amd import nrrd
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel
from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10
GROUPS = int(sys.argv[2]) if len(sys.argv) > 2 else 2
K = 18
# ([y, x] extent, (x, y) spacing in mm): on the plan spacing (1.5 mm), then the three geometries of profiles/r10_resampled_case.txt
GEOMETRIES = [((400, 273), (1.5, 1.5)), ((600, 512), (0.8, 1.0)), ((400, 512), (0.75, 2.5)), ((1000, 512), (0.7, 0.6))]
HAS_DEVICE_ROUTE = hasattr(HIPnnUNetPredictor, 'predict_labelmap_from_preprocessed_data')

arch = UNetArch.canonical(num_classes=K)
ds = {'channel_names': {'0': 'mean', '1': 'max'}, 'labels': {'background': 0, **{f'cardiac_{j}': j for j in range(1, K)}}, 'file_ending': '.nrrd'}
blobs = [(np.random.default_rng(f).standard_normal(arch.n_params()) * 0.02).astype(np.float32) for f in range(3)]


def images(hw, spacing, n, seed0):
    """n distinct cases: own Image object, own pixels."""
    return [nrrd.Image((np.random.default_rng(seed0 + s).standard_normal(hw + (2,)) * 200 + 50).astype(np.float32), spacing, (0.0, 0.0),
                       (1.0, 0.0, 0.0, 1.0), 2, {}, None) for s in range(n)]


def spans(stamps):
    """ms per case of the three stages: the median over the cases."""
    return {b: float(np.median([t[b] - t[a] for t in stamps])) * 1e3
            for a, b in (('start', 'preprocessed'), ('preprocessed', 'predicted'), ('predicted', 'exported'))}


def fmt(st):
    return 'preprocess {preprocessed:6.1f}  predict {predicted:6.1f}  export {exported:6.1f}'.format(**st)


print(f'label-map model, K = {K} heads, canonical net, 512 x 512 patch; device route in this tree: {HAS_DEVICE_ROUTE}')
all_equal = True
for F in (1, 3):
    m = HIPModel({'model': 'ts2d-v2-ep4000b2_cardiac', 'revision': 1, 'param': {},
                  'synthetic': {'arch': arch, 'blobs': blobs[:F], 'patch_size': (512, 512), 'dataset_json': ds}})
    assert not m.multilabel
    m.start()
    try:
        for hw, sp in GEOMETRIES:
            net = tuple(int(round(n * s / 1.5)) for n, s in zip(hw, (sp[1], sp[0])))
            res = {}
            for route, dev in (('host route', False), ('device route', True)):
                if dev and not HAS_DEVICE_ROUTE:
                    continue
                m.device_labelmap = dev
                cases = images(hw, sp, N, 100)                       # the same cases for both routes
                groups = [images(hw, sp, 8, 1000 + 8 * g) for g in range(GROUPS)]
                for im in images(hw, sp, 3, 500):
                    m.apply(im)
                m.apply_batch(images(hw, sp, 8, 600))
                t, out, st1 = [], [], []
                for im in cases:
                    t0 = time.perf_counter(); out.append(m.apply(im).array); t.append(time.perf_counter() - t0)
                    st1.append(dict(m.timestamps))
                t0 = time.perf_counter()
                many, st8 = [], []
                for g in groups:
                    many += [r.array for r in m.apply_batch(g).values()]
                    st8 += [dict(s) for s in m.batch_timestamps.values()]
                per_case8 = (time.perf_counter() - t0) / (8 * GROUPS)
                res[route] = (float(np.median(t)), per_case8, out, many, spans(st1), spans(st8))
            h = res['host route']
            labels = sorted(set(np.unique(np.concatenate([a.ravel() for a in h[2]])).tolist()))
            print(f'F = {F}, {hw[0]} x {hw[1]} at {sp[1]} x {sp[0]} mm -> {net[0]} x {net[1]}: {len(labels)} labels in the {N} label maps')
            for route, (med, per8, _, _, s1, s8) in res.items():
                print(f'    {route:13s} apply median of {N}: {med * 1e3:7.1f} ms per case   [{fmt(s1)}]')
                print(f'    {"":13s} apply_batch of 8, {8 * GROUPS} distinct cases: {per8 * 1e3:7.1f} ms per case   [{fmt(s8)}]')
            if 'device route' in res:
                d = res['device route']
                eq = (all(np.array_equal(a, b) for a, b in zip(h[2], d[2])), all(np.array_equal(a, b) for a, b in zip(h[3], d[3])))
                all_equal &= all(eq) and len(labels) >= 2
                print(f'    label maps of all {N} + {8 * GROUPS} cases byte-identical across the routes (apply, apply_batch): {eq}')
                print(f'    device route: {h[0] / d[0]:.2f}x the host route per case (apply), {h[1] / d[1]:.2f}x in apply_batch', flush=True)
    finally:
        m.stop()
if HAS_DEVICE_ROUTE:
    print(f'label maps byte-identical between the two routes in every measured case: {all_equal}')
sys.exit(0 if all_equal else 1)
