"""Per-case wall time of a STACK - a 3-D volume that a 2-D model takes slice by slice (what `nnUNetv2_predict -c 2d` does with a CT): the host
routes of both sides against the device routes, each switched on its own in ONE process.
  input   ``device_input_stack`` off: crop_to_nonzero with the 3-D hole filling, numpy's normalisation passes, scipy's cubic zoom per (channel, slice)
          where the volume is off the plan spacing (the old switches stay on: they refuse a stack);  on: ts2d_planes_create_stack /
          ts2d_planes_crop_normalize_stack (csrc/kernels_prep_stack.h), the resample on the handle, one download.
  output  ``device_stack`` off: K float16 planes per slice to the host, scipy order 1 per (head, slice), argmax or threshold over [K, Z, H, W];  on: the
          predictor's stack methods - every slice one image of ts2d_ensemble_predict_tiled_labelmap / _export, uint8 planes to the host.
One canonical sub-model (K = 18 heads, F = 1, synthetic weights) as a label-map model and as its multilabel twin; one-channel volumes of Z = 64
slices, 512 x 512 on the plan spacing and 600 x 512 at 1.0 x 0.8 mm.  HIPModel.apply per route: the median of N volumes, each its own image object
with its own voxels, the routes alternating; HIPModel.apply_batch of two volumes with everything off and everything on, and with everything on under
``stack_call_bytes`` of 256 MiB, 1 GiB and 4 GiB.  Every route is warmed up on a stack of four slices of the same extent.  Stage spans on the host
clock.  The baseline is the same process with the switch off: the route the parent commit takes.

    timeout -k 10 900 python scripts/gpu_stack_case.py labelmap 0 [N=5] >> profiles/r20_stack_case.txt     # model: labelmap | multilabel; volume: 0 | 1
    (one invocation per model and volume, each under its own time limit; exit status 0 = complete and byte-identical)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from totalsegmentator2d_amd import nrrd, weights
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel

KIND = sys.argv[1] if len(sys.argv) > 1 else 'labelmap'
VOLUME = int(sys.argv[2]) if len(sys.argv) > 2 else 0
N = int(sys.argv[3]) if len(sys.argv) > 3 else 5
K, Z = 18, 64
# ([y, x] extent, (x, y, z) spacing in mm): on the plan spacing (1.5 mm in plane), and off it
HW, SPACING = [((512, 512), (1.5, 1.5, 3.0)), ((600, 512), (0.8, 1.0, 3.0))][VOLUME]
BUDGETS = (256 << 20, 1 << 30, 4 << 30)

arch = UNetArch.canonical(input_channels=1, num_classes=K)
labels = {'background': 0, **{f'organ_{j}': j for j in range(1, K + (KIND == 'multilabel'))}}
ds = {'channel_names': {'0': 'ct'}, 'labels': labels, 'file_ending': '.nrrd', **({'multilabel': True} if KIND == 'multilabel' else {})}
blob = weights.pack_blob(arch, weights.synthetic_state_dict(arch, 20))


def volume(seed, z=Z):
    """One case: own Image object, own voxels; a margin of zeros (two slices, eight rows, twelve columns) for the crop box to bite."""
    a = np.zeros((z,) + HW, np.float32)
    a[1:z - 1, 5:HW[0] - 3, 4:HW[1] - 8] = np.random.default_rng(seed).standard_normal((z - 2, HW[0] - 8, HW[1] - 12)) * 200 + 50
    return nrrd.Image(a, SPACING, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), 1, {}, 'left-posterior-superior')


def spans(stamps):
    return {b: float(np.median([t[b] - t[a] for t in stamps])) * 1e3
            for a, b in (('start', 'preprocessed'), ('preprocessed', 'predicted'), ('predicted', 'exported'))}


def fmt(st):
    return 'preprocess {preprocessed:8.1f}  predict {predicted:8.1f}  export {exported:8.1f}'.format(**st)


ROUTES = [('host input, host output', False, False), ('device input, host output', True, False), ('host input, device output', False, True),
          ('device input, device output', True, True)]
m = HIPModel({'model': f'ts2d-v2-ep4000b2_{KIND}', 'revision': 1, 'param': {},
              'synthetic': {'arch': arch, 'blobs': [blob], 'patch_size': (512, 512), 'dataset_json': ds}})
assert m.multilabel == (KIND == 'multilabel')
m.start()
ok = True
try:
    def route(inp, out):
        m.device_input_stack, m.device_stack = inp, out

    for _, inp, out in ROUTES:                                   # warm-up: every route, the slices' own extent, four slices
        route(inp, out)
        m.apply(volume(900, 4))
        m.apply_batch([volume(901, 4), volume(902, 4)])
    cases = [volume(100 + s) for s in range(N)]
    t, res, st = {r[0]: [] for r in ROUTES}, {r[0]: [] for r in ROUTES}, {r[0]: [] for r in ROUTES}
    for im in cases:                                              # the routes alternate over the same cases
        for name, inp, out in ROUTES:
            route(inp, out)
            t0 = time.perf_counter(); res[name].append(m.apply(im).array); t[name].append(time.perf_counter() - t0)
            st[name].append(dict(m.timestamps))
    net = tuple(int(round(n * s / 1.5)) for n, s in zip(HW, (SPACING[1], SPACING[0])))
    print(f'{KIND} model, K = {K} heads, F = 1, canonical net, 512 x 512 patch; one channel, Z = {Z}, {HW[0]} x {HW[1]} at {SPACING[1]} x {SPACING[0]} mm '
          f'-> {net[0]} x {net[1]} per slice; {len(np.unique(res[ROUTES[0][0]][0]))} values in the first result')
    base = float(np.median(t[ROUTES[0][0]]))
    for name, _, _ in ROUTES:
        med = float(np.median(t[name]))
        same = all(np.array_equal(a, b) for a, b in zip(res[name], res[ROUTES[0][0]]))
        ok &= same
        print(f'    {name:28s} apply, median of {N} (min {min(t[name]) * 1e3:8.1f}, max {max(t[name]) * 1e3:8.1f}): {med * 1e3:8.1f} ms per volume  '
              f'{base / med:5.2f}x  [{fmt(spans(st[name]))}]  bytes equal: {same}')
    pairs = [[volume(200 + 2 * g), volume(201 + 2 * g)] for g in range(N)]
    tb, rb, sb = {}, {}, {}
    for name, _, _ in (ROUTES[0], ROUTES[3]):
        tb[name], rb[name], sb[name] = [], [], []
    for pair in pairs:
        for name, inp, out in (ROUTES[0], ROUTES[3]):
            route(inp, out)
            t0 = time.perf_counter(); r = m.apply_batch(pair); tb[name].append((time.perf_counter() - t0) / 2)
            rb[name] += [v.array for v in r.values()]
            sb[name] += [dict(s) for s in m.batch_timestamps.values()]
    base = float(np.median(tb[ROUTES[0][0]]))
    for name in tb:
        med = float(np.median(tb[name]))
        same = all(np.array_equal(a, b) for a, b in zip(rb[name], rb[ROUTES[0][0]]))
        ok &= same
        print(f'    {name:28s} apply_batch of 2, {N} pairs: {med * 1e3:8.1f} ms per volume  {base / med:5.2f}x  [{fmt(spans(sb[name]))}]  bytes equal: {same}')
    route(True, True)
    sweep = {b: [] for b in BUDGETS}
    for g, pair in enumerate(pairs):
        for b in BUDGETS:
            m._predictor.stack_call_bytes = b
            t0 = time.perf_counter(); r = m.apply_batch(pair); sweep[b].append((time.perf_counter() - t0) / 2)
            ok &= all(np.array_equal(v.array, w) for v, w in zip(r.values(), rb[ROUTES[3][0]][2 * g:2 * g + 2]))
    print('    stack_call_bytes sweep, device routes, apply_batch of 2 (ms per volume, median of %d): ' % N
          + ', '.join(f'{b >> 20} MiB {float(np.median(v)) * 1e3:8.1f}' for b, v in sweep.items()) + f'  bytes equal throughout: {ok}', flush=True)
finally:
    m.stop()
sys.exit(0 if ok else 1)
