"""Wall time of the PNG visuals, device route (image.create_visual(device=0): ts2d_visual_labels / ts2d_visual_grey, csrc/kernels_visual.h, uploads and
downloads included) against the host statement (device=None, totalsegmentator2d_amd/visual.py), in ONE process, the routes alternating.  Cases:
    segmentations  K = 117 and K = 18 multilabel planes (plane-major memory, as combine_segmentations hands them out) at 644 x 337 (isotropic) and at
                   600 x 512 with spacing 0.8 x 2.5; the same at 53 x 133 (the projections of the 3-D sample asset), isotropic and 0.8 x 2.5
    grey           float32 and int16 planes of the same extents
    x-ray          the 320 x 320 uint8 asset (tests/golden/assets/sample_chexpert.nrrd), grey
Every figure is the median of N with its minimum and maximum; every route is warmed up first; the bytes of the two routes are compared.  The size
gates of visual.py (LABELS_DEVICE_MIN, GREY_UNIFORM_DEVICE_MIN) are lifted for the run: they were set from these figures.

    timeout -k 10 600 python scripts/gpu_visual_case.py [N=5] >> profiles/r27_visual_case.txt        (exit status 0 = complete and equal)"""
import os, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from totalsegmentator2d_amd import image, nrrd, visual

visual.LABELS_DEVICE_MIN = visual.GREY_UNIFORM_DEVICE_MIN = 0      # the size gates are what this measurement decides: lifted, so device=0 is the device at every size
N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
EYE2 = (1.0, 0.0, 0.0, 1.0)
EXTENTS = (((337, 644), (1.5, 1.5)), ((512, 600), (2.5, 0.8)),      # array [H, W] and the spacing of (axis 0, axis 1)
           ((133, 53), (1.5, 1.5)), ((133, 53), (2.5, 0.8)))       # ... and the extent of the 3-D sample asset's projections: the small end
rng = np.random.default_rng(27)


def segmentation(K, shape, sp):
    planes = np.zeros((K,) + shape, np.uint8)
    for k in range(K):                                               # a blob per label, overlapping its neighbours
        cy, cx = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        planes[k, max(cy - 40, 0):cy + 40, max(cx - 30, 0):cx + 30] = 1
    seg = nrrd.Image(np.moveaxis(planes, 0, -1), (sp[1], sp[0]), (0.0, 0.0), EYE2, K, {}, None)
    image.set_annotation_meta(seg, {i + 1: f'label{i}' for i in range(K)}, {f'label{i}': tuple(int(v) for v in rng.integers(0, 256, 3)) for i in range(K)})
    return seg


def grey(dtype, shape, sp):
    a = rng.normal(size=shape) * 400 + 100
    return nrrd.Image(a.astype(dtype), (sp[1], sp[0]), (0.0, 0.0), EYE2, 1, {}, None)


def run(name, img, **how):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                              # (the uint8 asset: "falling back to nearest neighbour")
        image.create_visual(img, device=0, **how); image.create_visual(img, **how)      # warm-up
        th, td, same = [], [], True
        for _ in range(N):                                           # the routes alternate
            t0 = time.perf_counter(); h = image.create_visual(img, **how); th.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); d = image.create_visual(img, device=0, **how); td.append(time.perf_counter() - t0)
            same &= bool(np.array_equal(h.array, d.array))
    mh, md = float(np.median(th)), float(np.median(td))
    print(f'    {name:46s} -> {h.array.shape[0]:4d} x {h.array.shape[1]:4d}   host {mh * 1e3:8.2f} ms (min {min(th) * 1e3:8.2f}, max {max(th) * 1e3:8.2f})   '
          f'device {md * 1e3:8.2f} ms (min {min(td) * 1e3:8.2f}, max {max(td) * 1e3:8.2f})   host / device {mh / md:7.2f}x   equal: {same}', flush=True)
    return same


print(f'PNG visuals, median of {N}; device = image.create_visual(device=0) with uploads and downloads, host = image.create_visual(device=None)')
ok = True
for shape, sp in EXTENTS:
    for K in (117, 18):
        ok &= run(f'labels K = {K:3d}  {shape[1]} x {shape[0]} spacing {sp[1]} x {sp[0]}', segmentation(K, shape, sp), labels=True)
    for dtype in ('float32', 'int16'):
        ok &= run(f'grey {dtype:8s}    {shape[1]} x {shape[0]} spacing {sp[1]} x {sp[0]}', grey(dtype, shape, sp), labels=False)
xr = nrrd.read(os.path.join(ROOT, 'tests', 'golden', 'assets', 'sample_chexpert.nrrd'))
ok &= run(f'x-ray asset {xr.array.dtype} {xr.size[0]} x {xr.size[1]} spacing {xr.spacing[0]:g} x {xr.spacing[1]:g}', xr, labels=False)
sys.exit(0 if ok else 1)
