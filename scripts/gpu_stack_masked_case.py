"""Per-case wall time of a STACK whose plan normalises inside the non-zero mask (``use_mask_for_norm`` on a z-score channel: the MR plans): the host
route of the input side against the device route, switched in ONE process.
  ``device_input_stack_masked`` off: crop_to_nonzero with scipy's 3-D binary_fill_holes, numpy's masked mean / std / normalisation per channel, scipy's
          cubic zoom per (channel, slice) where the volume is off the plan spacing - the route the parent commit takes for such a plan;
  on:     ts2d_planes_create_stack / ts2d_planes_crop_normalize_stack_masked (csrc/kernels_prep_fill.h: the six-sweep rounds over two bit planes; the
          masked sums, the normalisation inside the mask), the resample on the handle, one download.
The output side keeps its device route (``device_stack``) in both.  One canonical sub-model (K = 18 heads, F = 1, synthetic weights, label-map) with one
or two input channels, all of them masked; head-like volumes - a smooth blob in a margin of zeros, with smooth cavities of zeros, closed ones and open
ones - of Z = 64 slices, 512 x 512 on the plan spacing and 600 x 512 at 1.0 x 0.8 mm, and a small one of 16 x 128 x 128.  HIPModel.apply per route: the
median of N volumes, each its own image object with its own voxels, the routes alternating; the preprocess span on the host clock beside it.  Every
route is warmed up on a stack of four slices of the same extent.  The rounds are those of preprocess.fill_holes_sweeps_statement on the first volume.

    timeout -k 10 600 python scripts/gpu_stack_masked_case.py 1 0 [N=5] >> profiles/r22_stack_masked_case.txt     # channels: 1 | 2; volume: 0 | 1 | 2
    (one invocation per channel count and volume, each under its own time limit; exit status 0 = complete and byte-identical)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from scipy.ndimage import gaussian_filter

from totalsegmentator2d_amd import nrrd, weights
from totalsegmentator2d_amd import preprocess as P
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel

C = int(sys.argv[1]) if len(sys.argv) > 1 else 1
VOLUME = int(sys.argv[2]) if len(sys.argv) > 2 else 0
N = int(sys.argv[3]) if len(sys.argv) > 3 else 5
K = 18
# (slices, [y, x] extent, (x, y, z) spacing in mm): on the plan spacing (1.5 mm in plane), off it, and a small volume
Z, HW, SPACING = [(64, (512, 512), (1.5, 1.5, 3.0)), (64, (600, 512), (0.8, 1.0, 3.0)), (16, (128, 128), (1.5, 1.5, 3.0))][VOLUME]

arch = UNetArch.canonical(input_channels=C, num_classes=K)
ds = {'channel_names': {str(c): f'mr{c}' for c in range(C)}, 'labels': {'background': 0, **{f'organ_{j}': j for j in range(1, K)}}, 'file_ending': '.nrrd'}
blob = weights.pack_blob(arch, weights.synthetic_state_dict(arch, 22))


def volume(seed, z=Z):
    """One case: own Image object, own voxels.  An ellipsoid of N(0,1) * 200 + 50 inside a margin of zeros; where a smooth random field is high the voxels
    are zero in every channel - cavities, closed inside the ellipsoid and open at its surface."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, z), np.linspace(-1, 1, HW[0]), np.linspace(-1, 1, HW[1]), indexing='ij')
    head = (zz * 0.9) ** 2 + yy ** 2 + xx ** 2 < 0.85
    sigma = max(2.0, HW[0] / 48.0)
    field = gaussian_filter(rng.standard_normal((z,) + HW, dtype=np.float32), (min(sigma, z / 6.0), sigma, sigma))
    keep = head & (field < 1.2 * field.std())
    a = (rng.standard_normal((z,) + HW + (C,), dtype=np.float32) * 200 + 50) * keep[..., None]
    a = a.astype(np.float32) if C > 1 else a[..., 0].astype(np.float32)
    return nrrd.Image(a, SPACING, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), C, {}, 'left-posterior-superior')


def pre_ms(stamps):
    return float(np.median([t['preprocessed'] - t['start'] for t in stamps])) * 1e3


ROUTES = [('host input', False), ('device input', True)]
m = HIPModel({'model': 'ts2d-v2-ep4000b2_mr', 'revision': 1, 'param': {},
              'synthetic': {'arch': arch, 'blobs': [blob], 'patch_size': (512, 512), 'dataset_json': ds}})
m.start()
ok = True
try:
    m._predictor.configuration_manager.use_mask_for_norm = [True] * C                # the MR plan: every channel normalised inside the mask
    for _, inp in ROUTES:                                                            # warm-up: both routes, the slices' own extent, four slices
        m.device_input_stack_masked = inp
        m.apply(volume(900, 4))
    cases = [volume(100 + s) for s in range(N)]
    first = np.asarray(cases[0].array).reshape((Z,) + HW + (C,))
    raw = (first != 0).any(axis=-1)
    box = P.crop_box3_statement(np.moveaxis(first, -1, 0))
    crop = raw[tuple(slice(b[0], b[1]) for b in box)]
    filled, rounds = P.fill_holes_sweeps_statement(crop)
    t, res, st = {r[0]: [] for r in ROUTES}, {r[0]: [] for r in ROUTES}, {r[0]: [] for r in ROUTES}
    for im in cases:                                                                 # the routes alternate over the same cases
        for name, inp in ROUTES:
            m.device_input_stack_masked = inp
            t0 = time.perf_counter(); res[name].append(m.apply(im).array); t[name].append(time.perf_counter() - t0)
            st[name].append(dict(m.timestamps))
    print(f'{C} masked z-score channel(s), Z = {Z}, {HW[0]} x {HW[1]} at {SPACING[1]} x {SPACING[0]} mm; first volume: box {box}, {int(crop.sum())} non-zero voxels, '
          f'{int(filled.sum() - crop.sum())} filled, {rounds} rounds')
    base, base_pre = float(np.median(t[ROUTES[0][0]])), pre_ms(st[ROUTES[0][0]])
    for name, _ in ROUTES:
        med = float(np.median(t[name]))
        same = all(np.array_equal(a, b) for a, b in zip(res[name], res[ROUTES[0][0]]))
        ok &= same
        pre = [(s['preprocessed'] - s['start']) * 1e3 for s in st[name]]
        print(f'    {name:14s} apply, median of {N} (min {min(t[name]) * 1e3:8.1f}, max {max(t[name]) * 1e3:8.1f}): {med * 1e3:8.1f} ms per volume  {base / med:5.2f}x   '
              f'preprocess span, median (min {min(pre):8.1f}, max {max(pre):8.1f}): {pre_ms(st[name]):8.1f} ms  {base_pre / pre_ms(st[name]):5.2f}x   bytes equal: {same}', flush=True)
finally:
    m.stop()
sys.exit(0 if ok else 1)
