"""Per-case wall time and accuracy of ``save_probabilities`` (the export's float32 probabilities, [K, *original shape]): the device route
(C-ABI ts2d_ensemble_predict_tiled_probabilities: every fold in one engine call, the mean on the device, resample-back, softmax, the
fill around the crop box and the argmax in one kernel, csrc/kernels_prob.h; K float32 planes and ONE uint8 plane to the host) against
the host route (K float16 planes to the host, scipy order 1 per plane, numpy's non-linearity and crop insert: ``device_probabilities =
False``) and against the same case without ``save_probabilities`` (the label-map device route), all in one process.  One canonical
label-map sub-model (the softmax: the kernel's three passes), K in {3, 18} heads, F in {1, 3} folds; the three off-spacing geometries
of scripts/gpu_resampled_case.py and one case on the plan spacing (400 x 273: an odd full width, the scalar-store path), every case its own image object with its own pixels.
HIPModel.apply: median of N cases after warm-up; HIPModel.apply_batch: ms per case over one group of 8 distinct cases; everything
twice, both runs reported.

Without arguments the script is the driver: one child process per step, each under its own `timeout`, stopping at the first step that
fails; the steps' output is the report.

    python scripts/gpu_probabilities_case.py [N=4] > profiles/r18_probabilities_case.txt        # every timing step
    python scripts/gpu_probabilities_case.py --accuracy > profiles/r18_probabilities_accuracy.txt
    timeout -k 10 300 python scripts/gpu_probabilities_case.py --step K F [N]                   # one step"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [(3, 1), (3, 3), (18, 1), (18, 3)]
STEP_SECONDS = 300

if sys.argv[1:2] == ['--accuracy']:       # the driver of the accuracy table: one child under its own limit
    sys.exit(subprocess.call(['timeout', '-k', '10', '120', sys.executable, os.path.abspath(__file__), '--accuracy-step']))
if sys.argv[1:2] not in (['--step'], ['--accuracy-step']):
    for K, F in STEPS:
        sys.stdout.flush()
        rc = subprocess.call(['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step', str(K), str(F)] + sys.argv[1:2])
        if rc != 0:
            print(f'step K = {K}, F = {F} ended with status {rc}: stopped here', flush=True)
            sys.exit(rc)
    sys.exit(0)

import numpy as np

from totalsegmentator2d_amd import export, nrrd

if sys.argv[1] == '--accuracy-step':
    # the input sets of tests/test_gpu_probabilities.py and of the issue, per mode and per K: max ulp error of torch-CPU, the numpy statement
    # and the device against float64 (tests/prob_util.py), and the largest |sum - 1| of the softmax from torch and from the device
    from tests import prob_util
    from totalsegmentator2d_amd.engine import probabilities_from_logits
    halves = np.arange(65536, dtype=np.uint16).view(np.float16).reshape(1, 256, 256)
    sets = [('all 65536 halves', 'multilabel', halves)]
    for K in (1, 2, 3, 18):
        lg = np.random.default_rng(100 + K).uniform(-20, 20, (K, 64, 64)).astype(np.float16)
        sets += [(f'uniform +-20, K = {K}, 64 x 64', 'multilabel', lg), (f'uniform +-20, K = {K}, 64 x 64', 'labelmap', lg)]
    sets.append(('normal x 8, K = 18, 64 x 64', 'labelmap', (np.random.default_rng(18).standard_normal((18, 64, 64)) * 8).astype(np.float16)))
    print('max error in float32 ulps against float64 over outputs >= 2^-126 (ulp / ref_ulp: the route / torch on the CPU; bound = 2 x ref_ulp + 1)')
    ok = True
    for name, mode, lg in sets:
        hw = lg.shape[1:]
        for out in (hw, (hw[0] + 9, hw[1] - 7)):
            v = prob_util.resampled(lg, (0, 0) + hw, out)
            dev = probabilities_from_logits(lg, (0, 0) + hw, out, out, (0, 0), mode, want_decided=False)[0]
            st = export.probabilities_statement(lg, (0, 0) + hw, out, out, (0, 0), mode)
            for route, p in (('statement', st), ('device', dev)):
                fig = prob_util.measure(f'[{name} -> {out[0]} x {out[1]}, {mode}] {route}:', p, v, mode == 'labelmap')
                ok &= fig['ulp'] <= fig['bound'] and fig['small_ok'] and fig['nan_ok']
            print(f'    device == statement on {float((dev.view(np.uint32) == st.view(np.uint32)).mean()) * 100:.4f} % of the values', flush=True)
    sys.exit(0 if ok else 1)

from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel

K, F = int(sys.argv[2]), int(sys.argv[3])
N = int(sys.argv[4]) if len(sys.argv) > 4 else 4
# ([y, x] extent, (x, y) spacing in mm): on the plan spacing (1.5 mm), then the three geometries of profiles/r10_resampled_case.txt
GEOMETRIES = [((400, 273), (1.5, 1.5)), ((600, 512), (0.8, 1.0)), ((400, 512), (0.75, 2.5)), ((1000, 512), (0.7, 0.6))]

arch = UNetArch.canonical(num_classes=K)
ds = {'channel_names': {'0': 'mean', '1': 'max'}, 'file_ending': '.nrrd', 'labels': {'background': 0, **{f'label_{j}': j for j in range(1, K)}}}
blobs = [(np.random.default_rng(f).standard_normal(arch.n_params()) * 0.02).astype(np.float32) for f in range(F)]


def images(hw, spacing, n, seed0):
    """n distinct cases: own Image object, own pixels."""
    return [nrrd.Image((np.random.default_rng(seed0 + s).standard_normal(hw + (2,)) * 200 + 50).astype(np.float32), spacing, (0.0, 0.0),
                       (1.0, 0.0, 0.0, 1.0), 2, {}, None) for s in range(n)]


def measure(m, hw, sp, save):
    """(median s per case of apply, s per case of apply_batch of 8, the results of both)."""
    kw = {'save_probabilities': True} if save else {}
    m.apply(images(hw, sp, 1, 500)[0], **kw)
    m.apply_batch(images(hw, sp, 8, 600), **kw)
    t, out = [], []
    for im in images(hw, sp, N, 100):
        t0 = time.perf_counter(); out.append(m.apply(im, **kw)); t.append(time.perf_counter() - t0)
    group = images(hw, sp, 8, 1000)
    t0 = time.perf_counter()
    many = list(m.apply_batch(group, **kw).values())
    return float(np.median(t)), (time.perf_counter() - t0) / 8, out, many


print(f'K = {K} heads, F = {F} folds, canonical net, 512 x 512 patch, label-map model (softmax); N = {N}')
ok = True
m = HIPModel({'model': 'ts2d-v2-ep4000b2_cardiac', 'revision': 1, 'param': {},
              'synthetic': {'arch': arch, 'blobs': blobs, 'patch_size': (512, 512), 'dataset_json': ds}})
m.start()
try:
    for hw, sp in GEOMETRIES:
        net = tuple(int(round(n * s / 1.5)) for n, s in zip(hw, (sp[1], sp[0])))
        print(f'{hw[0]} x {hw[1]} at {sp[1]} x {sp[0]} mm -> {net[0]} x {net[1]}: {K * hw[0] * hw[1] * 4 / 1e6:.1f} MB of float32 per case')
        runs = []
        for run in range(2):
            res = {}
            for route, dev, save in (('host route', False, True), ('device route', True, True), ('no probabilities', True, False)):
                m.device_probabilities = dev
                res[route] = measure(m, hw, sp, save)
            runs.append(res)
            for route, r in res.items():
                print(f'    run {run}: {route:16s} apply median of {N}: {r[0] * 1e3:7.1f} ms per case   apply_batch of 8: {r[1] * 1e3:7.1f} ms per case')
        h, d, n0 = (runs[-1][k] for k in ('host route', 'device route', 'no probabilities'))
        same = all(np.array_equal(a.array, b.array) and np.array_equal(a.array, c.array) for i in (2, 3) for a, b, c in zip(h[i], d[i], n0[i]))
        diff = max(float(np.abs(a.probabilities - b.probabilities).max()) for i in (2, 3) for a, b in zip(h[i], d[i]))
        ok &= same and diff < 1e-6
        spread = max(abs(runs[0][k][i] - runs[1][k][i]) / runs[1][k][i] for k in runs[0] for i in (0, 1))
        print(f'    segmentations byte-identical across the three routes: {same}; largest |device - host| probability: {diff:.3g}')
        print(f'    device route: {h[0] / d[0]:.2f}x the host route per case (apply), {h[1] / d[1]:.2f}x in apply_batch; '
              f'{d[0] / n0[0]:.2f}x / {d[1] / n0[1]:.2f}x the time of the case without probabilities; run-to-run spread up to {spread * 100:.1f} %', flush=True)
finally:
    m.stop()
sys.exit(0 if ok else 1)
