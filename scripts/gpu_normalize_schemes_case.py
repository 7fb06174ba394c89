"""Per-case wall time of native 2-D inputs whose plan does not use the plain z-score - CTNormalization, the z-score inside the non-zero mask,
RescaleTo01Normalization, RGBTo01Normalization, NoNormalization - with crop box + normalisation (+ the order-3 resample) on device-resident planes
(``HIPModel.device_input_normalize_schemes``, csrc/kernels_prep_schemes.h) and with numpy on the host.  One process, per scheme and input the
median of N cases after 3 warm-up cases, with the quartiles of the N times beside it:

    preprocess   HIPModel._preprocess_input alone (to array -> crop -> normalise -> resample), the stage the switch moves
    apply        HIPModel.apply: that stage + the sliding window + the export

Inputs: square two-channel planes of 128, 192 and 256 samples a side on the plan spacing (where the size gate of the plain z-score route lies,
preprocess.DEVICE_NORMALIZE_MIN_SAMPLES), the extents of the reference's two 2-channel sample assets, and a 1000 x 512 case off the plan
spacing.  The size gate is lifted for the "on" runs so that every input takes the route.  Masks are compared: equal bytes on both routes.

    timeout -k 10 900 python scripts/gpu_normalize_schemes_case.py [N=15] > profiles/r16_normalize_schemes_case.txt     # exit status 0 = complete"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from totalsegmentator2d_amd import nrrd
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel

N = int(sys.argv[1]) if len(sys.argv) > 1 else 15
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'assets')
SHIPPED_THRESHOLD = P.DEVICE_NORMALIZE_MIN_SAMPLES
FIP = {str(c): {'percentile_00_5': -300.0, 'percentile_99_5': 420.5, 'mean': 48.0 + c, 'std': 190.0} for c in range(2)}
SCHEMES = {'CT': (['CTNormalization'] * 2, [False] * 2), 'masked z-score': (['ZScoreNormalization'] * 2, [True] * 2),
           'Rescale01': (['RescaleTo01Normalization'] * 2, [False] * 2), 'RGB01': (['RGBTo01Normalization'] * 2, [False] * 2),
           'none': (['NoNormalization'] * 2, [False] * 2)}


def model():
    arch = UNetArch.canonical(input_channels=2, num_classes=18, n_stages=8)
    blob = (np.random.default_rng(0).standard_normal(arch.n_params()) * 0.02).astype(np.float32)
    ds = {'channel_names': {'0': 'mean', '1': 'max'}, 'labels': {'background': 0, **{f'l{j + 1}': j + 1 for j in range(18)}}, 'file_ending': '.nrrd', 'multilabel': True}
    return HIPModel({'model': 'schemes', 'revision': 1, 'param': {},
                     'synthetic': {'arch': arch, 'blobs': [blob], 'patch_size': (512, 512), 'spacing': (1.5, 1.5), 'dataset_json': ds}})


def synthetic(seed, hw, spacing, border, rgb):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, hw + (2,)).astype(np.float32) if rgb else (rng.standard_normal(hw + (2,)) * 200 + 50).astype(np.float32)
    a[rng.random(hw) < 0.1] = 0                        # zeros in the interior: the non-zero mask is not the box
    if border:
        a[:border] = 0; a[-border:] = 0; a[:, :border] = 0; a[:, -border:] = 0
    return nrrd.Image(a, spacing, (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), 2, {}, None)


def copies(img, n):
    return [nrrd.Image(img.array.copy(), img.spacing, img.origin, img.direction, img.components, dict(img.meta or {}), None) for _ in range(n)]


def times_ms(fn, cases):
    for c in cases[:3]:
        fn(c)
    t = []
    for c in cases[3:]:
        t0 = time.perf_counter(); fn(c); t.append(time.perf_counter() - t0)
    return np.percentile(np.array(t) * 1e3, [50, 25, 75])


def measure(name, img, m, with_apply):
    row, masks = {}, {}
    for on in (True, False):
        P.DEVICE_NORMALIZE_MIN_SAMPLES = 0 if on else SHIPPED_THRESHOLD
        m.device_input_normalize_schemes = on
        row[on] = [times_ms(lambda c: m._preprocess_input(c), copies(img, N + 3))] + ([times_ms(m.apply, copies(img, N + 3))] if with_apply else [])
        masks[on] = m.apply(img).array
    P.DEVICE_NORMALIZE_MIN_SAMPLES = SHIPPED_THRESHOLD
    pre = m._preprocess_input(img)[1]
    print(f'  {name}: {img.array.shape} at {tuple(round(s, 3) for s in img.spacing)} mm -> network input {tuple(pre.shape)}; masks equal on both routes: {np.array_equal(masks[True], masks[False])}')
    for k, label in enumerate(('preprocess', 'apply')[:len(row[True])]):
        d, h = row[True][k], row[False][k]
        print(f'    {label:10s} median of {N} [quartiles]: device {d[0]:7.2f} [{d[1]:.2f} {d[2]:.2f}] ms   host {h[0]:7.2f} [{h[1]:.2f} {h[2]:.2f}] ms   ({h[0] / d[0]:.2f}x, {h[0] - d[0]:+.2f} ms)')
    sys.stdout.flush()


print(f'shipped threshold: DEVICE_NORMALIZE_MIN_SAMPLES = {SHIPPED_THRESHOLD}')
m = model()
m.start()
try:
    s0616 = nrrd.read(os.path.join(ASSETS, 'sample_s0616.nrrd'))
    s0332 = nrrd.read(os.path.join(ASSETS, 'sample_s0332.nrrd'))
    extents = [('2 x 128^2', (128, 128), (1.5, 1.5), 0, False), ('2 x 192^2', (192, 192), (1.5, 1.5), 0, False), ('2 x 256^2', (256, 256), (1.5, 1.5), 0, False),
               ('extent of sample_s0616', tuple(s0616.array.shape[:2]), tuple(s0616.spacing[:2]), 0, True),
               ('extent of sample_s0332', (s0332.array.shape[0], s0332.array.shape[2]), (s0332.spacing[0], s0332.spacing[2]), 0, True),
               ('1000 x 512, zero borders, off spacing', (1000, 512), (0.7, 0.6), 40, True)]
    for scheme, (names, use_mask) in SCHEMES.items():
        cm = m._predictor.configuration_manager
        cm.normalization_schemes, cm.use_mask_for_norm = names, use_mask
        m._predictor.plans_manager.plans = {'foreground_intensity_properties_per_channel': FIP}
        print(f'{scheme}:')
        for i, (name, hw, spacing, border, with_apply) in enumerate(extents):
            measure(name, synthetic(i, hw, spacing, border, scheme == 'RGB01'), m, with_apply)
finally:
    m.stop()
