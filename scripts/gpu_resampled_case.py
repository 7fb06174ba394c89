"""Per-case wall time of cases whose spacing is NOT the plan's (1.5 mm): the host route of the export (float16 logits to the host,
scipy order 1 per plane, threshold) against the device export (csrc/kernels_resample.h: resample-back + threshold behind the sliding
window) and against the device export with the order-3 INPUT resample on the device as well (csrc/kernels_resample_in.h, the product
default).  Five canonical sub-models (K = 18/23/24/26/26, synthetic weights) as in scripts/gpu_case_latency.py; synthetic two-channel
images of the three geometries of the issue (original extent at its spacing -> network extent), every case its OWN image object with
its own pixels (the sub-models of one case share a preprocessing cache that hangs on the image: aliases of one image would share it
across cases).  TS2D.predict: median of N cases after warm-up; predict_many(max_cases=8): cases/s over 3 groups of 8 distinct cases.
Stage spans (host clock, summed over the five sub-models, which run concurrently - they add up to more than the wall time) and the
order-3 input resample of one case timed on its own, on the host and on the device (the whole synchronous call: allocation, copies in,
three kernels, copy out), say where the time over an un-resampled case of the same network geometry goes.

    timeout -k 10 600 python scripts/gpu_resampled_case.py [N=20] > profiles/r10_resampled_case.txt     # exit status 0 = complete"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from totalsegmentator2d_amd import nrrd
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel
from totalsegmentator2d_amd.tool import TS2D

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
GROUPS = 3                                                                                         # predict_many: 3 x 8 = 24 cases
GEOMETRIES = [((600, 512), (0.8, 1.0)), ((400, 512), (0.75, 2.5)), ((1000, 512), (0.7, 0.6))]      # ([y, x] extent, (x, y) spacing in mm)

groups = [('cardiac', 18), ('muscles', 23), ('organs', 24), ('ribs', 26), ('vertebrae', 26)]
models = {}
for i, (g, K) in enumerate(groups):
    arch = UNetArch.canonical(num_classes=K)
    blob = (np.random.default_rng(i).standard_normal(arch.n_params()) * 0.02).astype(np.float32)
    ds = {'channel_names': {'0': 'mean', '1': 'max'}, 'labels': {'background': 0, **{f'{g}_{j+1}': j + 1 for j in range(K)}},
          'file_ending': '.nrrd', 'multilabel': True}
    models[f'ts2d-v2-ep4000b2_{g}'] = HIPModel({'model': f'ts2d-v2-ep4000b2_{g}', 'revision': 1, 'param': {},
                                               'synthetic': {'arch': arch, 'blobs': [blob], 'patch_size': (512, 512), 'dataset_json': ds}})


def images(hw, spacing, n, seed0):
    """n distinct cases: own Image object, own pixels."""
    return [nrrd.Image((np.random.default_rng(seed0 + s).standard_normal(hw + (2,)) * 200 + 50).astype(np.float32), spacing, (0.0, 0.0),
                       (1.0, 0.0, 0.0, 1.0), 2, {}, None) for s in range(n)]


def route(ts, device, device_input):
    for m in ts.models.values():
        m.device_threshold = device
        m.device_input_resample = device_input


def stages(results):
    """ms per case of the three stages, summed over the sub-models."""
    st = {}
    for res in results:
        for r in res.data['models'].values():
            t = r['timestamps']
            for a, b in (('start', 'preprocessed'), ('preprocessed', 'predicted'), ('predicted', 'exported')):
                st[b] = st.get(b, 0.0) + (t[b] - t[a]) * 1e3 / len(results)
    return 'preprocess {preprocessed:6.1f}  predict {predicted:6.1f}  export {exported:6.1f}'.format(**st)


with TS2D(models=models) as ts:
    for hw, sp in GEOMETRIES:
        net = tuple(int(round(n * s / 1.5)) for n, s in zip(hw, (sp[1], sp[0])))
        # the host order-3 input resample of ONE case of this geometry, on its own (it runs once per case: the sub-models share it)
        z = np.stack([P.zscore(c) for c in np.moveaxis(images(hw, sp, 1, 900)[0].array, -1, 0)])[:, None]
        P.resample_data_to_shape(z, (1,) + net, order=3)
        t0 = time.perf_counter()
        for _ in range(5):
            P.resample_data_to_shape(z, (1,) + net, order=3)
        t_in = (time.perf_counter() - t0) / 5
        ref = P.resample_data_to_shape(z, (1,) + net, order=3)
        got = P.resample_data_to_shape(z, (1,) + net, order=3, device=0)                 # (warm-up of the three kernels as well)
        same_in = np.array_equal(ref.view(np.uint32), got.view(np.uint32))
        t0 = time.perf_counter()
        for _ in range(20):
            P.resample_data_to_shape(z, (1,) + net, order=3, device=0)
        t_dev = (time.perf_counter() - t0) / 20
        res = {}
        for name, dev, dev_in, ehw, esp in (('host route', False, False, hw, sp), ('device export', True, False, hw, sp),
                                            ('device in + export', True, True, hw, sp), ('un-resampled', True, True, net, (1.5, 1.5))):
            route(ts, dev, dev_in)
            cases = images(ehw, esp, N, 100)                     # the same N cases for both routes
            many_in = [images(ehw, esp, 8, 1000 + 8 * g) for g in range(GROUPS)]
            for im in images(ehw, esp, 3, 500):
                ts.predict(im)
            ts.predict_many(images(ehw, esp, 8, 600), max_cases=8)
            t, out = [], []
            for im in cases:
                t0 = time.perf_counter(); out.append(ts.predict(im)); t.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            many = [ts.predict_many(g, max_cases=8) for g in many_in]
            rate = 8 * GROUPS / (time.perf_counter() - t0)
            res[name] = (float(np.median(t)), rate, [r.get_segmentation().array for r in out],
                         [r.get_segmentation().array for g in many for r in g], stages(out), stages([r for g in many for r in g]))
        h, d, di, u = (res[k] for k in ('host route', 'device export', 'device in + export', 'un-resampled'))
        eq = (all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(h[2], d[2], di[2])),
              all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(h[3], d[3], di[3])))
        print(f'{hw[0]} x {hw[1]} at {sp[1]} x {sp[0]} mm -> {net[0]} x {net[1]}: masks of all {N} + {8 * GROUPS} cases equal (predict, predict_many): {eq}')
        for name, (med, rate, _, _, s1, s8) in res.items():
            print(f'    {name:18s} predict median of {N}: {med * 1e3:6.1f} ms per case   [{s1}]')
            print(f'    {"":18s} predict_many(max_cases=8), {8 * GROUPS} distinct cases: {rate:5.1f} cases/s   [{s8}]')
        print(f'    order-3 input resample of one case, on its own: host {t_in * 1e3:.1f} ms, device {t_dev * 1e3:.2f} ms (whole call), same bits: {same_in}')
        print(f'    device in + export: {d[0] / di[0]:.2f}x the device export per case ({(d[0] - di[0]) * 1e3:.1f} ms less; {di[1] / d[1]:.2f}x in cases/s), '
              f'{di[0] / u[0]:.2f}x an un-resampled case ({(di[0] - u[0]) * 1e3:.1f} ms more)')
        print(f'    device export: {h[0] / d[0]:.1f}x the host route per case ({d[1] / h[1]:.1f}x in cases/s), {d[0] / u[0]:.2f}x an un-resampled case '
              f'of the same network geometry ({(d[0] - u[0]) * 1e3:.1f} ms more, of which the input resample is {t_in * 1e3:.1f} ms)', flush=True)
