"""Per-case wall time of a STACK that asks for PROBABILITIES (``nnUNetv2_predict -c 2d --save_probabilities`` on a CT): the host route against
the device route in ONE process.
  off      ``device_stack_probabilities`` off - the parent commit's route and the baseline: K float16 planes per slice to the host, scipy order 1 per
           (head, slice) in float64, numpy's sigmoid / softmax with a float64 exp, the insertion into float32 [K, Z0, H0, W0].
  on       the predictor's stack probabilities methods: every slice through sw_probabilities<ProbStackSeg> (csrc/kernels_prob.h), written in place into
           ONE float32 [K, Z0, H0, W0] by K copies per run of slices (C-ABI ts2d_ensemble_predict_tiled_probabilities_stack).
  no flag  the same volumes without ``save_probabilities``: the decided map alone (scripts/gpu_stack_case.py measures that route).
One canonical sub-model (K heads, F = 1, synthetic weights) as a label-map model or its multilabel twin; one-channel volumes of Z = 64 slices, 512 x 512
on the plan spacing or 600 x 512 at 1.0 x 0.8 mm.  HIPModel.apply per route, no ``result_dir``: the median of N volumes, each its own image object with
its own voxels, the routes alternating, every route warmed up on a stack of four slices; the ``predicted`` and ``exported`` spans on the host clock.
The results are compared case by case and dropped (K = 18: 1.2 GB each): segmentation bytes, the probabilities outside the box, the largest difference
inside it.  ``--result-dir``: ONE more volume per route with a ``result_dir`` (the .npz compression is the host's on both routes), reported apart.

    timeout -k 10 900 python scripts/gpu_stack_probabilities_case.py labelmap 0 [K=18] [N=5] [--result-dir] >> profiles/r23_stack_probabilities_case.txt
    (model: labelmap | multilabel; volume: 0 | 1; one invocation per model and volume, each under its own time limit; exit status 0 = complete, the
    segmentations byte-identical and the fill exact)"""
import os, shutil, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from totalsegmentator2d_amd import nrrd, weights
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel

args = [a for a in sys.argv[1:] if not a.startswith('--')]
KIND = args[0] if len(args) > 0 else 'labelmap'
VOLUME = int(args[1]) if len(args) > 1 else 0
K = int(args[2]) if len(args) > 2 else 18
N = int(args[3]) if len(args) > 3 else 5
WITH_DIR = '--result-dir' in sys.argv
Z = 64
HW, SPACING = [((512, 512), (1.5, 1.5, 3.0)), ((600, 512), (0.8, 1.0, 3.0))][VOLUME]

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


ROUTES = [('off (host route)', False, True), ('on (device route)', True, True), ('no flag', True, False)]
m = HIPModel({'model': f'ts2d-v2-ep4000b2_{KIND}', 'revision': 1, 'param': {},
              'synthetic': {'arch': arch, 'blobs': [blob], 'patch_size': (512, 512), 'dataset_json': ds}})
assert m.multilabel == (KIND == 'multilabel')
m.start()
ok = True
try:
    for _, on, flag in ROUTES:                                   # warm-up: every route, the slices' own extent, four slices
        m.device_stack_probabilities = on
        m.apply(volume(900, 4), save_probabilities=flag)
    t, st = {r[0]: [] for r in ROUTES}, {r[0]: [] for r in ROUTES}
    worst, fill_same, seg_same = 0.0, True, True
    for s in range(N):                                            # the routes alternate over the same cases
        im = volume(100 + s)
        got = {}
        for name, on, flag in ROUTES:
            m.device_stack_probabilities = on
            t0 = time.perf_counter(); r = m.apply(im, save_probabilities=flag); t[name].append(time.perf_counter() - t0)
            st[name].append(dict(m.timestamps))
            got[name] = r
        host, dev, plain = (got[r[0]] for r in ROUTES)
        seg_same &= np.array_equal(host.array, plain.array) and np.array_equal(dev.array, plain.array)
        a, b = host.probabilities, dev.probabilities
        assert a.shape == b.shape == (K, Z) + HW and a.dtype == b.dtype == np.float32
        inside = (slice(None), slice(1, Z - 1), slice(5, HW[0] - 3), slice(4, HW[1] - 8))
        for k in range(K):                                        # (plane by plane: no third copy of the volume)
            worst = max(worst, float(np.abs(a[k][inside[1:]] - b[k][inside[1:]]).max()))
            edge_a, edge_b = a[k].copy(), b[k].copy()
            edge_a[inside[1:]] = edge_b[inside[1:]] = 0
            fill_same &= np.array_equal(edge_a, edge_b)
        del got, host, dev, plain, a, b
    ok &= seg_same and fill_same
    net = tuple(int(round(n * s / 1.5)) for n, s in zip(HW, (SPACING[1], SPACING[0])))
    print(f'{KIND} model, K = {K} heads, F = 1, canonical net, 512 x 512 patch; one channel, Z = {Z}, {HW[0]} x {HW[1]} at {SPACING[1]} x {SPACING[0]} mm '
          f'-> {net[0]} x {net[1]} per slice; probabilities float32 [{K}, {Z}, {HW[0]}, {HW[1]}] = {K * Z * HW[0] * HW[1] * 4 / 2 ** 20:.0f} MiB')
    base = float(np.median(t[ROUTES[0][0]]))
    for name, _, _ in ROUTES:
        med = float(np.median(t[name]))
        print(f'    {name:18s} apply, median of {N} (min {min(t[name]) * 1e3:8.1f}, max {max(t[name]) * 1e3:8.1f}): {med * 1e3:8.1f} ms per volume  '
              f'{base / med:5.2f}x  [{fmt(spans(st[name]))}]')
    print(f'    segmentations byte-identical over the three routes: {seg_same};  probabilities outside the box equal: {fill_same};  '
          f'largest |device - host| inside it: {worst:.3g}', flush=True)
    if WITH_DIR:
        im = volume(300)
        for name, on, flag in ROUTES[:2]:
            m.device_stack_probabilities = on
            d = tempfile.mkdtemp()
            try:
                t0 = time.perf_counter(); m.apply({'case': im}, d, save_probabilities=True); dt = time.perf_counter() - t0
                size = os.path.getsize(os.path.join(d, 'case.npz'))
            finally:
                shutil.rmtree(d)
            print(f'    {name:18s} apply with a result_dir, ONE volume: {dt * 1e3:8.1f} ms  [{fmt(spans([dict(m.timestamps)]))}]  .npz {size / 2 ** 20:.0f} MiB', flush=True)
finally:
    m.stop()
sys.exit(0 if ok else 1)
