"""Per-case wall time of a FOLD ENSEMBLE (what nnU-Net trains by default: F folds, their logits averaged): the host route (per fold the
float16 logits to the host, numpy's half sum and division, then the export's widening, scipy order 1 and threshold on the host:
``device_threshold = False``) against the device route (C-ABI ts2d_ensemble_predict_tiled_export: every fold in one engine call, the
mean of the folds on the device, csrc/kernels_fold.h, then the device export).  One canonical sub-model (K = 18, synthetic weights per
fold) with F in {1, 2, 5}; one case on the plan spacing (400 x 273 at 1.5 mm) and one off it (600 x 512 at 1.0 x 0.8 mm -> 400 x 273),
every case its own image object with its own pixels.  HIPModel.apply: median of N cases after warm-up; HIPModel.apply_batch: ms per
case over 3 groups of 8 distinct cases.  Stage spans on the host clock (preprocess / predict / export; the median over the cases, the
cases of one apply_batch share the predict span of their group).  `over F x net`: the per-case time minus F times the predict span of
the single-fold case of the same geometry on the device route - what an ensemble costs beyond running the network F times.

    timeout -k 10 900 python scripts/gpu_ensemble_case.py [N=12] > profiles/r11_ensemble_case.txt     # exit status 0 = complete"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from totalsegmentator2d_amd import nrrd
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel

N = int(sys.argv[1]) if len(sys.argv) > 1 else 12
GROUPS = 3
K = 18
GEOMETRIES = [('on the plan spacing', (400, 273), (1.5, 1.5)), ('off the plan spacing', (600, 512), (0.8, 1.0))]   # ([y, x] extent, (x, y) spacing in mm)

arch = UNetArch.canonical(num_classes=K)
ds = {'channel_names': {'0': 'mean', '1': 'max'}, 'labels': {'background': 0, **{f'cardiac_{j + 1}': j + 1 for j in range(K)}},
      'file_ending': '.nrrd', 'multilabel': True}
blobs = [(np.random.default_rng(f).standard_normal(arch.n_params()) * 0.02).astype(np.float32) for f in range(5)]


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


net1 = {}                         # geometry -> predict span (ms) of the single-fold case on the device route
all_equal = True
for F in (1, 2, 5):
    m = HIPModel({'model': 'ts2d-v2-ep4000b2_cardiac', 'revision': 1, 'param': {},
                  'synthetic': {'arch': arch, 'blobs': blobs[:F], 'patch_size': (512, 512), 'dataset_json': ds}})
    m.start()
    try:
        for gname, hw, sp in GEOMETRIES:
            res = {}
            for route, dev in (('host route', False), ('device route', True)):
                m.device_threshold = dev
                cases = images(hw, sp, N, 100)                       # the same cases for both routes
                groups = [images(hw, sp, 8, 1000 + 8 * g) for g in range(GROUPS)]
                for im in images(hw, sp, 4, 500):
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
            h, d = res['host route'], res['device route']
            eq = (all(np.array_equal(a, b) for a, b in zip(h[2], d[2])), all(np.array_equal(a, b) for a, b in zip(h[3], d[3])))
            all_equal &= all(eq) and all(a.any() for a in d[2])
            if F == 1:
                net1[gname] = d[4]['predicted']
            print(f'F = {F}, {hw[0]} x {hw[1]} at {sp[1]} x {sp[0]} mm ({gname}): masks of all {N} + {8 * GROUPS} cases equal (apply, apply_batch): {eq}')
            for route, (med, per8, _, _, s1, s8) in res.items():
                print(f'    {route:13s} apply median of {N}: {med * 1e3:7.1f} ms per case   [{fmt(s1)}]   over F x net: {med * 1e3 - F * net1[gname]:6.1f} ms')
                print(f'    {"":13s} apply_batch of 8, {8 * GROUPS} distinct cases: {per8 * 1e3:7.1f} ms per case   [{fmt(s8)}]')
            print(f'    device route: {h[0] / d[0]:.2f}x the host route per case (apply), {h[1] / d[1]:.2f}x in apply_batch', flush=True)
    finally:
        m.stop()
print(f'masks byte-identical between the two routes in every measured case: {all_equal}')
sys.exit(0 if all_equal else 1)
