"""Per-case wall time of nnU-Net's largest-component postprocessing (postprocess.py): a label-map model with the plan "all foreground, then every
label" (K steps for K - 1 labels), the step on the device (``device_postprocessing`` on: ts2d_keep_largest_components, csrc/kernels_post_cc.h) against
the host route (off: scipy.ndimage.label per step) and against the same case with no plan, in ONE process, the three alternating over the same cases.
One canonical sub-model (K heads, F = 1, synthetic weights, so the maps are speckle: tens of thousands of components per label, far more than an
anatomical map holds); one-channel inputs:
    0   a stack of 64 slices, 512 x 512 on the plan spacing          1   a stack of 64 slices, 600 x 512 at 1.0 x 0.8 mm
    2   one 2-D case, 512 x 512                                      3   a small volume, 16 x 128 x 128
HIPModel.apply per route: the median of N cases, each its own image object with its own voxels.  "step" is the span around the postprocessing alone
(img.postprocessing['seconds']: upload, every step, download - or scipy), "apply" the whole call.  Every route is warmed up first.

    timeout -k 10 600 python scripts/gpu_postprocess_case.py 18 0 [N=5] >> profiles/r25_postprocess_case.txt     # K: 3 | 18; geometry: 0 .. 3
    (one invocation per K and geometry, each under its own time limit; exit status 0 = complete and byte-identical)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from totalsegmentator2d_amd import nrrd, weights
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel

K = int(sys.argv[1]) if len(sys.argv) > 1 else 18
GEOMETRY = int(sys.argv[2]) if len(sys.argv) > 2 else 0
N = int(sys.argv[3]) if len(sys.argv) > 3 else 5
# (slices or None for a 2-D case, [y, x] extent, in-plane (x, y) spacing in mm)
Z, HW, SP = [(64, (512, 512), (1.5, 1.5)), (64, (600, 512), (0.8, 1.0)), (None, (512, 512), (1.5, 1.5)), (16, (128, 128), (1.5, 1.5))][GEOMETRY]

arch = UNetArch.canonical(input_channels=1, num_classes=K)
ds = {'channel_names': {'0': 'ct'}, 'labels': {'background': 0, **{f'organ_{j}': j for j in range(1, K)}}, 'file_ending': '.nrrd'}
blob = weights.pack_blob(arch, weights.synthetic_state_dict(arch, 25))
PLAN = [(list(range(1, K)), 0)] + [([j], 0) for j in range(1, K)]


def case(seed, z=Z):
    """One case: own Image object, own voxels; a margin of zeros for the crop box to bite."""
    rng = np.random.default_rng(seed)
    if z is None:
        a = np.zeros(HW, np.float32)
        a[5:HW[0] - 3, 4:HW[1] - 8] = rng.standard_normal((HW[0] - 8, HW[1] - 12)) * 200 + 50
        return nrrd.Image(a, SP, (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 1, {}, None)
    a = np.zeros((z,) + HW, np.float32)
    a[1:z - 1, 5:HW[0] - 3, 4:HW[1] - 8] = rng.standard_normal((z - 2, HW[0] - 8, HW[1] - 12)) * 200 + 50
    return nrrd.Image(a, SP + (3.0,), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), 1, {}, 'left-posterior-superior')


ROUTES = [('no plan', None, True), ('plan, host route', PLAN, False), ('plan, device route', PLAN, True)]
m = HIPModel({'model': 'ts2d-v2-ep4000b2_labelmap', 'revision': 1, 'param': {},
              'synthetic': {'arch': arch, 'blobs': [blob], 'patch_size': (512, 512), 'dataset_json': ds}})
m.start()
ok = True
try:
    def route(plan, device):
        m.set_postprocessing(plan)
        m.device_postprocessing = device

    for _, plan, device in ROUTES:                                   # warm-up: every route on a case of the same in-plane extent
        route(plan, device)
        m.apply(case(900, None if Z is None else 4))
    cases = [case(100 + s) for s in range(N)]
    t, step, res, info = ({r[0]: [] for r in ROUTES} for _ in range(4))
    for im in cases:                                                 # the routes alternate over the same cases
        for name, plan, device in ROUTES:
            route(plan, device)
            t0 = time.perf_counter(); out = m.apply(im); t[name].append(time.perf_counter() - t0)
            res[name].append(out.array)
            post = getattr(out, 'postprocessing', None)
            step[name].append(post['seconds'] if post else 0.0)
            info[name].append(post)
    shape = res['no plan'][0].shape
    first = info['plan, host route'][0]['stats']
    print(f'label-map model, K = {K} heads, {len(PLAN)} steps, canonical net, F = 1; map {" x ".join(str(v) for v in shape)} ({int(np.prod(shape))} voxels), '
          f'first case: {int(first[0, 0])} foreground voxels in {int(first[0, 1])} components, {int(first[1:, 1].sum())} components over the labels, '
          f'{int(first[:, 3].sum())} voxels removed')
    base = float(np.median(t['no plan']))
    for name, plan, device in ROUTES:
        med, sp = float(np.median(t[name])), float(np.median(step[name]))
        line = f'    {name:20s} apply, median of {N} (min {min(t[name]) * 1e3:9.1f}, max {max(t[name]) * 1e3:9.1f}): {med * 1e3:9.1f} ms  (+{(med - base) * 1e3:9.1f} over no plan)  step {sp * 1e3:9.1f} ms'
        if plan is not None:
            want = 'device' if device else 'host'
            same = all(np.array_equal(a, b) for a, b in zip(res[name], res['plan, host route'])) \
                and all(np.array_equal(p['stats'], q['stats']) for p, q in zip(info[name], info['plan, host route']))
            routed = all(p['route'] == want for p in info[name])
            changed = all(not np.array_equal(a, b) for a, b in zip(res[name], res['no plan']))
            ok &= same and routed and changed
            line += f'  route {want}: {routed}  bytes and counters equal to the host route: {same}'
        print(line)
    h, d = float(np.median(step['plan, host route'])), float(np.median(step['plan, device route']))
    print(f'    step, host / device: {h / d:7.2f}x', flush=True)
    assert ok, 'a route differs'
finally:
    m.stop()
sys.exit(0 if ok else 1)
