"""Per-case wall time of a REGION-BASED model (label values are lists, one head per foreground region, `regions_class_order`; export =
resample the logits back, sigmoid > 0.5 per head, paint the regions in order): the host route (K float16 planes to the host, scipy
order 1 per plane where the case is off the plan spacing, threshold and the painting loop in numpy; a fold ensemble adds numpy's half
sum and division: ``device_regions = False``) against the device route (C-ABI ts2d_ensemble_predict_tiled_regions: every fold in one
engine call, the mean on the device, resample-back, predicate and painting in one kernel, csrc/kernels_regions.h, ONE uint8 plane to
the host) - and, in the same process, the device route of a LABEL-MAP model with the same K (ts2d_ensemble_predict_tiled_labelmap): the
two calls move the same bytes, so that one is the yardstick.  One canonical sub-model (synthetic weights per fold), K in {3, 18}
regions, F in {1, 3} folds; the three off-spacing geometries of scripts/gpu_resampled_case.py and one case on the plan spacing, every
case its own image object with its own pixels.  HIPModel.apply: median of N cases after warm-up; HIPModel.apply_batch: ms per case over
GROUPS groups of 8 distinct cases.

Without arguments the script is the driver: one child process per (K, F) step, each under its own `timeout`, stopping at the first
step that fails; the steps' output is the report.

    python scripts/gpu_regions_case.py [N=10] [GROUPS=2] > profiles/r17_regions_case.txt      # every step; exit status 0 = complete
    timeout -k 10 300 python scripts/gpu_regions_case.py --step K F [N] [GROUPS]              # one step"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [(3, 1), (3, 3), (18, 1), (18, 3)]
STEP_SECONDS = 300

if sys.argv[1:2] != ['--step']:
    for K, F in STEPS:
        sys.stdout.flush()
        rc = subprocess.call(['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step', str(K), str(F)] + sys.argv[1:3])
        if rc != 0:
            print(f'step K = {K}, F = {F} ended with status {rc}: stopped here', flush=True)
            sys.exit(rc)
    sys.exit(0)

import numpy as np

from totalsegmentator2d_amd import nrrd
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel

K, F = int(sys.argv[2]), int(sys.argv[3])
N = int(sys.argv[4]) if len(sys.argv) > 4 else 10
GROUPS = int(sys.argv[5]) if len(sys.argv) > 5 else 2
# ([y, x] extent, (x, y) spacing in mm): on the plan spacing (1.5 mm), then the three geometries of profiles/r10_resampled_case.txt
GEOMETRIES = [((400, 273), (1.5, 1.5)), ((600, 512), (0.8, 1.0)), ((400, 512), (0.75, 2.5)), ((1000, 512), (0.7, 0.6))]

arch = UNetArch.canonical(num_classes=K)
base = {'channel_names': {'0': 'mean', '1': 'max'}, 'file_ending': '.nrrd'}
# nested regions, BraTS style: region j holds the labels j+1 .. K; painted in order, so class j+1 is "region j without region j+1"
ds_regions = dict(base, labels={'background': 0, **{f'region_{j}': list(range(j + 1, K + 1)) for j in range(K)}}, regions_class_order=list(range(1, K + 1)))
ds_labelmap = dict(base, labels={'background': 0, **{f'label_{j}': j for j in range(1, K)}})
blobs = [(np.random.default_rng(f).standard_normal(arch.n_params()) * 0.02).astype(np.float32) for f in range(F)]


def images(hw, spacing, n, seed0):
    """n distinct cases: own Image object, own pixels."""
    return [nrrd.Image((np.random.default_rng(seed0 + s).standard_normal(hw + (2,)) * 200 + 50).astype(np.float32), spacing, (0.0, 0.0),
                       (1.0, 0.0, 0.0, 1.0), 2, {}, None) for s in range(n)]


def model(ds):
    return HIPModel({'model': 'ts2d-v2-ep4000b2_cardiac', 'revision': 1, 'param': {},
                     'synthetic': {'arch': arch, 'blobs': blobs, 'patch_size': (512, 512), 'dataset_json': ds}})


def measure(m, hw, sp):
    """(median s per case of apply, s per case of apply_batch, the arrays of both, median ms of the predict span of apply)."""
    cases = images(hw, sp, N, 100)
    groups = [images(hw, sp, 8, 1000 + 8 * g) for g in range(GROUPS)]
    for im in images(hw, sp, 3, 500):
        m.apply(im)
    m.apply_batch(images(hw, sp, 8, 600))
    t, out, pred = [], [], []
    for im in cases:
        t0 = time.perf_counter(); out.append(m.apply(im).array); t.append(time.perf_counter() - t0)
        pred.append((m.timestamps['predicted'] - m.timestamps['preprocessed']) * 1e3)
    t0 = time.perf_counter()
    many = []
    for g in groups:
        many += [r.array for r in m.apply_batch(g).values()]
    return float(np.median(t)), (time.perf_counter() - t0) / (8 * GROUPS), out, many, float(np.median(pred))


print(f'K = {K} heads, F = {F} folds, canonical net, 512 x 512 patch; region-based model against a label-map model of the same K')
ok = True
mr, ml = model(ds_regions), model(ds_labelmap)
assert not mr.multilabel and not ml.multilabel
mr.start(); ml.start()
try:
    assert mr._predictor.regions_class_order == tuple(range(1, K + 1)) and ml._predictor.regions_class_order is None
    for hw, sp in GEOMETRIES:
        net = tuple(int(round(n * s / 1.5)) for n, s in zip(hw, (sp[1], sp[0])))
        res = {}
        for route, m, dev in (('regions host', mr, False), ('regions device', mr, True), ('labelmap device', ml, True)):
            m.device_regions = m.device_labelmap = dev
            res[route] = measure(m, hw, sp)
        h, d, l = res['regions host'], res['regions device'], res['labelmap device']
        classes = sorted(set(np.unique(np.concatenate([a.ravel() for a in h[2]])).tolist()))
        eq = (all(np.array_equal(a, b) for a, b in zip(h[2], d[2])), all(np.array_equal(a, b) for a, b in zip(h[3], d[3])))
        ok &= all(eq)
        print(f'{hw[0]} x {hw[1]} at {sp[1]} x {sp[0]} mm -> {net[0]} x {net[1]}: {len(classes)} classes in the {N} region maps')
        for route, r in res.items():
            print(f'    {route:16s} apply median of {N}: {r[0] * 1e3:7.1f} ms per case (predict span {r[4]:6.1f})   '
                  f'apply_batch of 8, {8 * GROUPS} distinct cases: {r[1] * 1e3:7.1f} ms per case')
        print(f'    region maps of all {N} + {8 * GROUPS} cases byte-identical across the routes (apply, apply_batch): {eq}')
        print(f'    regions device: {h[0] / d[0]:.2f}x the host route per case (apply), {h[1] / d[1]:.2f}x in apply_batch')
        print(f'    regions device / labelmap device: {d[0] / l[0]:.3f} (apply), {d[1] / l[1]:.3f} (apply_batch), {d[4] / l[4]:.3f} (predict span)', flush=True)
finally:
    mr.stop(); ml.stop()
print(f'K = {K}, F = {F}: region maps byte-identical between the two routes in every measured case: {ok}', flush=True)
sys.exit(0 if ok else 1)
