"""Wall time of the synthetic radiograph on the device, the whole call with its upload and its download (csrc/kernels_project_xr.h behind
engine.project_xr / engine.project_labels_xr), against the host statements of totalsegmentator2d_amd/xray.py, in ONE process, the routes
alternating.  Every figure is the median of N with its minimum and maximum; the device route is warmed up first; the results of the routes are
compared in every round (equal: bit for bit, byte for byte).
Cases: volumes of a few planes under detectors of 80 x 6 and 240 x 120 pixels (where the size gate of xray.py lies); the 3-D sample asset; a synthetic int16 CT of
512 x 512 x 600 under a cone beam and under parallel rays, its label projection at num = 117, and - the yardstick for one pass over that volume -
ts2d_project_coronal_modes (mean) on it; TS2D.predict of a one-channel synthetic model on the sample asset with the radiograph as its channel,
beside the render alone and beside the same model on the mean projection without the option.

    timeout -k 10 1100 python scripts/gpu_synthetic_xr_case.py [N=5] >> profiles/r38_synthetic_xr_case.txt        (exit status 0 = complete and equal)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from totalsegmentator2d_amd import engine, image, nrrd, xray as X

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
EYE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
rng = np.random.default_rng(38)


def timed(name, routes, equal):
    routes['device']()                                               # warm-up
    t = {r: [] for r in routes}
    got, same = {}, True
    for _ in range(N):                                               # the routes alternate
        for r, fn in routes.items():
            t0 = time.perf_counter(); got[r] = fn(); t[r].append(time.perf_counter() - t0)
        same &= equal(got)
    med = {r: float(np.median(v)) for r, v in t.items()}
    line = f'    {name:52s}'
    for r in routes:
        line += f'   {r} {med[r] * 1e3:10.2f} ms (min {min(t[r]) * 1e3:10.2f}, max {max(t[r]) * 1e3:10.2f})'
    line += ''.join(f'   {r} / device {med[r] / med["device"]:8.2f}x' for r in routes if r != 'device')
    print(line + f'   equal: {same}', flush=True)
    return same


def radiograph(name, img, geometry=None):
    a, ext, strides, base, _, _ = image._coronal_view(img)
    view, spacing, _, _ = X._view(img)
    tb = X.xr_tables(view.shape, spacing, geometry)

    def statement():
        s = X.synthetic_xr_statement(view, tb)
        return s, (s * tb['step']).astype(np.float32)
    return timed(name, {'device': lambda: engine.project_xr(a, ext, strides, base, tb['geometry'], 0)[:2], 'statement': statement},
                 lambda got: got['device'][0].tobytes() == got['statement'][0].tobytes() and got['device'][1].tobytes() == got['statement'][1].tobytes())


def labels(name, img, num, geometry=None):
    a, ext, strides, base, _, _ = image._coronal_view(img)
    view, spacing, _, _ = X._view(img)
    tb = X.xr_tables(view.shape, spacing, geometry)
    return timed(name, {'device': lambda: engine.project_labels_xr(a, ext, strides, base, num, tb['geometry'], 0)[0],
                        'statement': lambda: X.project_labels_xr_statement(view, num, tb)},
                 lambda got: got['device'].tobytes() == got['statement'].tobytes())


def ct(shape):
    """air around an ellipsoid of soft tissue with a denser core: int16 [nz][ny][nx]"""
    nz, ny, nx = shape
    y, x = np.ogrid[:ny, :nx]
    r2 = (((y - ny / 2) / (ny * 0.35)) ** 2 + ((x - nx / 2) / (nx * 0.4)) ** 2).astype(np.float32)
    v = np.full(shape, -1000, np.int16)
    for z in range(nz):                                              # (slice by slice: no float volume beside the int16 one)
        r = r2 + np.float32(((z - nz / 2) / (nz * 0.45)) ** 2)
        v[z][r < 1.0] = 40
        v[z][r < 0.1] = 700
        v[z] += rng.integers(-20, 21, (ny, nx), dtype=np.int16)
    return v


def label_blocks(shape, num):
    v = np.zeros(shape, np.uint8)
    for k in range(1, num + 1):
        lo = [int(rng.integers(0, s - s // 6)) for s in shape]
        v[tuple(slice(o, o + max(1, s // 6)) for o, s in zip(lo, shape))] = k
    return v


print(f'synthetic radiograph, median of {N}; device = the whole call (ts2d_project_xr: sums and radiograph; ts2d_project_labels_xr) with upload and '
      f'download, statement = xray.synthetic_xr_statement (and the step and cast) / xray.project_labels_xr_statement on the host')
ok = True
# the small end, where a fixed cost of the call (0.15 ms) meets a statement that costs per plane: few planes, two detector sizes
for shape in [(1, 1, 1), (3, 2, 63)] + [(5, ny, 66) for ny in (1, 2, 3, 4, 6, 8, 12, 37)] + [(100, ny, 200) for ny in (1, 2, 3, 4, 6)]:
    small = nrrd.Image(ct(shape), (1.5, 0.75, 2.0), (0.0, 0.0, 0.0), EYE, 1, {}, None)
    ok &= radiograph(f'int16 {shape[2]} x {shape[1]} x {shape[0]}  cone beam', small)
    ok &= labels(f'uint8 {shape[2]} x {shape[1]} x {shape[0]}  labels num = 3', nrrd.Image(label_blocks(shape, 3), (1.5, 0.75, 2.0), (0.0, 0.0, 0.0), EYE, 1, {}, None), 3)
case = nrrd.read(os.path.join(ROOT, 'tests', 'golden', 'assets', 'sample_s0521.nrrd'))
ok &= radiograph('sample_s0521 (53 x 120 x 133 int16)  cone beam', case)
ok &= labels('sample_s0521 grid  labels num = 117', nrrd.Image(label_blocks(case.array.shape, 117), case.spacing, case.origin, case.direction, 1, {}, None), 117)
big = nrrd.Image(ct((600, 512, 512)), (0.8, 0.8, 1.0), (0.0, 0.0, 0.0), EYE, 1, {}, None)
ok &= radiograph('int16 512 x 512 x 600  cone beam', big)
ok &= radiograph('int16 512 x 512 x 600  parallel rays', big, X.XRGeometry(parallel=True))
ok &= labels('uint8 512 x 512 x 600  labels num = 117  cone beam', nrrd.Image(label_blocks((600, 512, 512), 117), big.spacing, big.origin, EYE, 1, {}, None), 117)
image.project_coronal_gpu(big, 0, modes=['mean'])
t = []
for _ in range(N):
    t0 = time.perf_counter(); image.project_coronal_gpu(big, 0, modes=['mean']); t.append(time.perf_counter() - t0)
print(f'    {"int16 512 x 512 x 600  ts2d_project_coronal_modes (mean): one pass over the volume":52s}   device {np.median(t) * 1e3:10.2f} ms '
      f'(min {min(t) * 1e3:10.2f}, max {max(t) * 1e3:10.2f})', flush=True)
del big

from tests.surface_util import synthetic_model
from totalsegmentator2d_amd.tool import TS2D
mx, _, _ = synthetic_model('ts2d-v2-ep4000b2_cardiac', 3, 41, channels=('xray',), feats=(32, 32))
mm, _, _ = synthetic_model('ts2d-v2-ep4000b2_ribs', 3, 41, channels=('mean',), feats=(32, 32))
with TS2D(models={'ts2d-v2-ep4000b2_cardiac': mx}, synthetic_xr=True) as tx, TS2D(models={'ts2d-v2-ep4000b2_ribs': mm}) as tm:
    want = X.synthetic_xr(case).array.tobytes()
    routes = {'predict with the radiograph': lambda: tx.predict(case).get_projection('xray').array.tobytes(),
              'the render alone': lambda: X.synthetic_xr(case, device=0).array.tobytes(),
              'predict on the mean projection': lambda: tm.predict(case) and want}
    for fn in routes.values():
        fn()
    t = {r: [] for r in routes}
    for _ in range(N):
        for r, fn in routes.items():
            t0 = time.perf_counter(); same = fn() == want; t[r].append(time.perf_counter() - t0)
            ok &= same
    print('    TS2D.predict, one sub-model of one channel, sample_s0521:' + ''.join(
        f'   {r} {np.median(v) * 1e3:9.2f} ms (min {min(v) * 1e3:9.2f}, max {max(v) * 1e3:9.2f})' for r, v in t.items()) + f'   equal: {ok}', flush=True)
sys.exit(0 if ok else 1)
