"""Wall time of the projection modes (image.project_coronal_gpu(modes=...): ts2d_project_coronal_modes, csrc/kernels_project_modes.h) against the host
statement (image.project behind image.reorient_image, the reorientation copy included), per mode, and of TS2D.predict of a synthetic (median, std)
sub-model, device route against host route (``_gpu_projection`` off), in ONE process, the routes alternating.  Volumes:
    0   the 3-D sample asset (tests/golden/assets/sample_s0521.nrrd)          1   a synthetic int16 CT of 512 x 512 x 600 (x, y, z)
Every figure is the median of N with its minimum and maximum; every route is warmed up first; the planes of the two routes are compared.

    timeout -k 10 900 python scripts/gpu_projection_modes_case.py 1 [N=5] >> profiles/r26_projection_modes_case.txt
    (one invocation per volume, each under its own time limit; exit status 0 = complete and equal)
    ... 1 3 trace: only the device calls of (max), (median), (std) and all seven modes, N times each in that order, for a kernel trace of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/gpu_projection_modes_case.py 1 3 trace"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tests.surface_util import synthetic_model
from totalsegmentator2d_amd import image, nrrd
from totalsegmentator2d_amd.tool import TS2D

VOLUME = int(sys.argv[1]) if len(sys.argv) > 1 else 0
N = int(sys.argv[2]) if len(sys.argv) > 2 else 5
MODES = ('max', 'min', 'mean', 'median', 'std', 'first', 'slice:middle')

if VOLUME == 0:
    vol = nrrd.read(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'assets', 'sample_s0521.nrrd'))
else:
    rng = np.random.default_rng(26)
    a = rng.integers(-1024, 1500, (600, 512, 512), dtype=np.int16)
    a[:, :40] = -1024; a[:, :, :30] = 0                              # air in front of the body, a margin of zeros
    vol = nrrd.Image(a, (0.8, 0.8, 1.5), (0.0, 0.0, 0.0), (-1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0), 1, {}, 'left-posterior-superior')


def host(modes):
    r = image.reorient_image(vol)
    return {m: image.cast(image.project(r, m, 'coronal'), np.float32).array[:, 0, :] for m in modes}


def device(modes, zscore=False):
    got = image.project_coronal_gpu(vol, zscore=zscore, modes=list(modes))
    return {m: got[m].array[:, 0, :] for m in modes}


def line(name, th, td, same):
    mh, md = float(np.median(th)), float(np.median(td))
    print(f'    {name:22s} host {mh * 1e3:9.2f} ms (min {min(th) * 1e3:9.2f}, max {max(th) * 1e3:9.2f})   device {md * 1e3:9.2f} ms (min {min(td) * 1e3:9.2f}, '
          f'max {max(td) * 1e3:9.2f})   host / device {mh / md:8.2f}x   equal: {same}', flush=True)


if len(sys.argv) > 3 and sys.argv[3] == 'trace':
    for modes in (('max',), ('median',), ('std',), MODES):
        for _ in range(N):
            device(modes)
    sys.exit(0)

ok = True
size = vol.size
print(f'volume {VOLUME}: {size[0]} x {size[1]} x {size[2]} {vol.array.dtype} ({vol.array.nbytes / 1e6:.1f} MB), rays of {image.reorient_image(vol).size[1]} samples; '
      f'median of {N}; device = image.project_coronal_gpu(modes=[...]) with upload and download, host = image.project(image.reorient_image(...))')
for modes in [(m,) for m in MODES] + [('median', 'std'), MODES]:
    device(modes); host(modes[:1])                                   # warm-up
    th, td, same = [], [], True
    for _ in range(N):                                               # the routes alternate
        t0 = time.perf_counter(); h = host(modes); th.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); d = device(modes); td.append(time.perf_counter() - t0)
        same &= all(np.array_equal(h[m], d[m]) for m in modes)
    ok &= same
    line(' + '.join(modes) if len(modes) < 3 else f'all {len(modes)} modes', th, td, same)
t0 = time.perf_counter(); device(('median', 'std'), zscore=True); tz = time.perf_counter() - t0
print(f'    median + std with the z-score outputs, one call: {tz * 1e3:9.2f} ms')

models = lambda: {'ts2d-v2-ep4000b2_ribs': synthetic_model('ts2d-v2-ep4000b2_ribs', 4, 62, channels=('median', 'std'), patch=(64, 64), mirror=False)[0]}
with TS2D(models=models()) as ts:
    res, t = {}, {False: [], True: []}
    for dev in (True, False):                                        # warm-up
        ts._gpu_projection = dev
        ts.predict(vol)
    for _ in range(N):
        for dev in (False, True):
            ts._gpu_projection = dev
            t0 = time.perf_counter(); r = ts.predict(vol); t[dev].append(time.perf_counter() - t0)
            res[dev] = r.get_segmentation().array
    same = bool(np.array_equal(res[True], res[False]))
    ok &= same
    line('TS2D.predict (median, std)', t[False], t[True], same)
sys.exit(0 if ok else 1)
