"""Per-case wall time of inputs that are 2-D when they arrive, with crop box + z-score (+ the order-3 resample) on device-resident planes
(``HIPModel.device_input_normalize``, csrc/kernels_prep.h) and with numpy on the host.  One process, medians of N cases after warm-up:

    preprocess   HIPModel._preprocess_input alone (read -> crop -> z-score -> resample), the stage the switch moves
    apply        HIPModel.apply: that stage + the sliding window + the export
    predict      TS2D.predict with two sub-models that share one preprocessing (two-channel inputs only)

Inputs: the reference's three sample assets (two 2-channel projections, one X-ray image), a synthetic two-channel case off the plan spacing
with zero borders, and a one-channel 1024 x 1024-patch, 9-stage model of the X-ray family on synthetic 2000 x 2500 and 3000 x 3000 images
off its spacing.  The size threshold of the route is lifted for the "on" runs so that every input takes it; the last lines sweep
square two-channel planes on the plan spacing to place the threshold.  Masks are compared: equal bytes on both routes.

    timeout -k 10 600 python scripts/gpu_native2d_case.py [N=15] > profiles/r12_native2d_case.txt     # exit status 0 = complete"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from totalsegmentator2d_amd import nrrd
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel
from totalsegmentator2d_amd.tool import TS2D

N = int(sys.argv[1]) if len(sys.argv) > 1 else 15
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'assets')
SHIPPED_THRESHOLD = P.DEVICE_NORMALIZE_MIN_SAMPLES


def model(mid, channels, K, n_stages, patch, spacing, seed):
    arch = UNetArch.canonical(input_channels=len(channels), num_classes=K, n_stages=n_stages)
    blob = (np.random.default_rng(seed).standard_normal(arch.n_params()) * 0.02).astype(np.float32)
    ds = {'channel_names': {str(i): c for i, c in enumerate(channels)}, 'labels': {'background': 0, **{f'l{j + 1}': j + 1 for j in range(K)}},
          'file_ending': '.nrrd', 'multilabel': True}
    return HIPModel({'model': mid, 'revision': 1, 'param': {},
                     'synthetic': {'arch': arch, 'blobs': [blob], 'patch_size': patch, 'spacing': spacing, 'dataset_json': ds}})


def synthetic(seed, hw, spacing, channels, border):
    a = (np.random.default_rng(seed).standard_normal(hw + (channels,)) * 200 + 50).astype(np.float32)
    if border:
        a[:border] = 0; a[-border:] = 0; a[:, :border] = 0; a[:, -border:] = 0
    return nrrd.Image(a if channels > 1 else a[..., 0], spacing, (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), channels, {}, None)


def copies(img, n):
    """n cases with the pixels of `img`, every one its OWN image object (the preprocessing cache of TS2D.predict hangs on the image)."""
    return [nrrd.Image(img.array.copy(), img.spacing, img.origin, img.direction, img.components, dict(img.meta or {}), None) for _ in range(n)]


def median_ms(fn, cases):
    for c in cases[:3]:
        fn(c)
    t = []
    for c in cases[3:]:
        t0 = time.perf_counter(); fn(c); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def measure(name, img, m, ts=None):
    row, masks = {}, {}
    for on in (True, False):
        P.DEVICE_NORMALIZE_MIN_SAMPLES = 0 if on else SHIPPED_THRESHOLD
        for mm in ([m] if ts is None else list(ts.models.values())):
            mm.device_input_normalize = on
        row[on] = [median_ms(lambda c: m._preprocess_input(c), copies(img, N + 3)), median_ms(m.apply, copies(img, N + 3))]
        masks[on] = [m.apply(img).array]
        if ts is not None:
            row[on].append(median_ms(ts.predict, copies(img, N + 3)))
            masks[on].append(ts.predict(copies(img, 1)[0]).get_segmentation().array)
    P.DEVICE_NORMALIZE_MIN_SAMPLES = SHIPPED_THRESHOLD
    same = all(np.array_equal(a, b) for a, b in zip(masks[True], masks[False]))
    pre = m._preprocess_input(img)[1]
    print(f'{name}: {img.array.shape} at {tuple(round(s, 3) for s in img.spacing)} mm -> network input {tuple(pre.shape)}; masks equal on both routes: {same}')
    for k, label in enumerate(('preprocess', 'apply', 'predict')[:len(row[True])]):
        print(f'    {label:10s} median of {N}: device {row[True][k]:8.2f} ms   host {row[False][k]:8.2f} ms   ({row[False][k] / row[True][k]:.2f}x, {row[False][k] - row[True][k]:+.2f} ms)')
    sys.stdout.flush()


print(f'shipped threshold: DEVICE_NORMALIZE_MIN_SAMPLES = {SHIPPED_THRESHOLD}')
ct = {f'ts2d-v2-ep4000b2_{g}': model(f'ts2d-v2-ep4000b2_{g}', ('mean', 'max'), K, 8, (512, 512), (1.5, 1.5), i) for i, (g, K) in enumerate((('cardiac', 18), ('ribs', 26)))}
with TS2D(models=ct) as ts:
    first = next(iter(ts.models.values()))
    s0332 = nrrd.read(os.path.join(ASSETS, 'sample_s0332.nrrd'))
    flat = nrrd.Image(np.ascontiguousarray(s0332.array[:, 0]), (s0332.spacing[0], s0332.spacing[2]), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)
    s0616 = nrrd.read(os.path.join(ASSETS, 'sample_s0616.nrrd'))
    measure('sample_s0616', nrrd.Image(s0616.array.astype(np.float32), s0616.spacing, s0616.origin, s0616.direction, 2, {}, None), first, ts)
    measure('sample_s0332', flat, first, ts)
    measure('synthetic 2-channel, zero borders, off spacing', synthetic(1, (1000, 512), (0.7, 0.6), 2, 40), first, ts)
    # where the route starts to pay: square two-channel planes on the plan spacing, preprocessing alone
    print('threshold sweep, 2 channels on the plan spacing, preprocess alone (device / host, ms):')
    first.device_input_normalize = True
    for side in (64, 96, 128, 192, 256, 384, 512, 1024, 2048):
        img = synthetic(side, (side, side), (1.5, 1.5), 2, 0)
        t = {}
        for on in (True, False):
            P.DEVICE_NORMALIZE_MIN_SAMPLES = 0 if on else 1 << 40
            t[on] = median_ms(lambda c: first._preprocess_input(c), copies(img, N + 3))
        print(f'    {side:5d}^2 x 2 = {2 * side * side:9d} samples: {t[True]:7.2f} / {t[False]:7.2f}   ({t[False] / t[True]:.2f}x)', flush=True)
    P.DEVICE_NORMALIZE_MIN_SAMPLES = SHIPPED_THRESHOLD

xr = model('tsxr-v1_lung', ('xray',), 6, 9, (1024, 1024), (0.3, 0.3), 7)
xr.start()
try:
    chex = nrrd.read(os.path.join(ASSETS, 'sample_chexpert.nrrd'))
    measure('sample_chexpert (X-ray, plan spacing 0.3 mm)', nrrd.Image(chex.array.astype(np.float32), chex.spacing, chex.origin, chex.direction, 1, {}, None), xr)
    measure('synthetic X-ray 2000 x 2500', synthetic(2, (2500, 2000), (0.14, 0.14), 1, 60), xr)
    measure('synthetic X-ray 3000 x 3000', synthetic(3, (3000, 3000), (0.12, 0.12), 1, 100), xr)
finally:
    xr.stop()
