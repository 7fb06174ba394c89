"""Wall time of the evaluation entries, each whole call with its uploads and downloads (csrc/kernels_evaluate.h behind evaluate._device_overlap,
evaluate._device_surface and evaluate.project_labels_coronal_gpu), against the host statements of evaluate.py and against the plain numpy / scipy a
user would write, in ONE process, the routes alternating:
    overlap      device / statement / plain numpy (per label ``==`` or ``> 0`` and ``sum``)
    distances    device / statement / scipy (per label and direction ``distance_transform_edt`` of the other border, read at the own border)
    projection   device / statement behind reorient_image / the reference's nonzero scatter behind reorient_image
Cases (those of scripts/gpu_statistics_case.py): 117 planes at 644 x 337; 18 planes at 600 x 512 with spacing 0.8 x 2.5 (mm per row, per column);
117 planes at 53 x 133; an overlap-only label-map stack 64 x 512 x 512 with 18 labels; for the projection an int16 512 x 512 x 600 label volume with
num = 117 and the extent of the small sample asset (133 x 120 x 53).  Every figure is the median of N with its minimum and maximum; the device
route is warmed up first; the results of device and statement are compared (equal: bit for bit).

    timeout -k 10 1100 python scripts/gpu_evaluate_case.py [N=5] >> profiles/r29_evaluate_case.txt        (exit status 0 = complete and equal)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from scipy import ndimage

from totalsegmentator2d_amd import evaluate as E, image, nrrd

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
DEVICE = None if os.environ.get('TS2D_EVALUATE_HOST_ONLY') else 0            # (host only: the host routes, on a machine without a GPU)
rng = np.random.default_rng(29)


def planes_pair(K, shape):
    """a blob per label, overlapping its neighbours; the other side is the same blob moved by a few pixels"""
    a, b = np.zeros((K,) + shape, np.uint8), np.zeros((K,) + shape, np.uint8)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    for k in range(K):
        cy, cx = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        ry, rx = max(2, shape[0] // 8), max(2, shape[1] // 10)
        a[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        b[k] = ((yy - cy - rng.integers(-3, 4)) / ry) ** 2 + ((xx - cx - rng.integers(-3, 4)) / (rx + 1)) ** 2 <= 1.0
    return a, b


def stack_pair(K, shape):
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for k in range(K):
        cz, cy, cx = (rng.integers(0, s) for s in shape)
        a[max(cz - 12, 0):cz + 12, max(cy - 60, 0):cy + 60, max(cx - 50, 0):cx + 50] = k + 1
        b[max(cz - 11, 0):cz + 13, max(cy - 58, 0):cy + 62, max(cx - 52, 0):cx + 48] = k + 1
    return a, b


def timed(name, routes, same_as=None):
    if 'device' in routes:
        routes['device']()                                           # warm-up
    t = {r: [] for r in routes}
    got, same = {}, True
    for _ in range(N):                                               # the routes alternate
        for r, fn in routes.items():
            t0 = time.perf_counter(); got[r] = fn(); t[r].append(time.perf_counter() - t0)
        if 'device' in routes:
            same &= same_as(got['device'], got['statement'])
    med = {r: float(np.median(v)) for r, v in t.items()}
    line = f'    {name:52s}'
    for r in routes:
        line += f'   {r} {med[r] * 1e3:9.2f} ms (min {min(t[r]) * 1e3:9.2f}, max {max(t[r]) * 1e3:9.2f})'
    if 'device' in routes:
        line += ''.join(f'   {r} / device {med[r] / med["device"]:7.2f}x' for r in routes if r != 'device')
    print(line + f'   equal: {same}', flush=True)
    return same


def dicts_equal(x, y):
    return all(np.array_equal(x[f].view(np.uint64) if x[f].dtype == np.float64 else x[f], y[f].view(np.uint64) if y[f].dtype == np.float64 else y[f]) for f in y)


def overlap(name, a, kind_a, b, kind_b, values, spatial):
    def plain():
        out = []
        for k in range(len(values)):
            ma = a[k] > 0 if kind_a == E.PLANES else a == values[k]
            mb = b[k] > 0 if kind_b == E.PLANES else b == values[k]
            out.append((int(ma.sum()), int(mb.sum()), int((ma & mb).sum())))
        return out
    routes = {'statement': lambda: E.overlap_statement(a, kind_a, b, kind_b, values), 'plain numpy': plain}
    if DEVICE is not None:
        routes = dict({'device': lambda: E._device_overlap(a, kind_a, b, kind_b, values, spatial, DEVICE)}, **routes)
    return timed('overlap    ' + name, routes, dicts_equal)


def distances(name, a, b, spacing, tol=(2.0,)):
    hw = a.shape[1:]

    def with_scipy():
        out = []
        for k in range(a.shape[0]):
            ma, mb = a[k] > 0, b[k] > 0
            ba, bb = ma & ~ndimage.binary_erosion(ma), mb & ~ndimage.binary_erosion(mb)
            for own, other in ((ba, bb), (bb, ba)):
                d = ndimage.distance_transform_edt(~other, sampling=spacing)[own] if other.any() else np.full(int(own.sum()), np.inf)
                out.append((int(own.sum()), float(d.max()) if len(d) else None, int((d <= tol[0]).sum())))
        return out
    routes = {'statement': lambda: E.surface_statement(a, E.PLANES, b, E.PLANES, None, spacing, tol), 'scipy edt': with_scipy}
    if DEVICE is not None:
        routes = dict({'device': lambda: E._device_surface(a, E.PLANES, b, E.PLANES, None, hw, spacing, tol, DEVICE)}, **routes)
    return timed('distances  ' + name, routes, dicts_equal)


def projection(name, shape, num):
    lab = np.zeros(shape, np.int16)
    for v in rng.permutation(np.arange(1, num + 1)):                 # boxes of every label, about a quarter of the volume labelled
        lo = [int(rng.integers(0, s - s // 6)) for s in shape]
        lab[tuple(slice(o, o + max(2, s // 6)) for o, s in zip(lo, shape))] = v
    vol = nrrd.Image(lab, (1.5, 1.5, 1.5), (0.0, 0.0, 0.0), (-1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0), 1, {}, None)

    def reference_scatter():
        arr = image.reorient_image(vol).array.T                      # ts2d/core/util/image.py:168-184, axis = 1
        arr = np.moveaxis(arr, 1, 0)
        idx = np.nonzero(arr)
        out = np.zeros((num, 1) + arr.shape[1:], np.uint8)
        out[(arr[idx] - 1, 0) + idx[1:]] = 1
        return np.moveaxis(out, 1, 2)
    routes = {'statement': lambda: E.project_labels(image.reorient_image(vol), num, 'coronal'), 'reference scatter': reference_scatter}
    if DEVICE is not None:
        routes = dict({'device': lambda: E.project_labels_coronal_gpu(vol, num, DEVICE)}, **routes)
    return timed('projection ' + name, routes, lambda x, y: x.array.tobytes() == y.array.tobytes())


print(f'evaluation, median of {N}; device = the whole call with uploads and downloads, statement = evaluate.py on the host, then the plain numpy / '
      f'scipy / reference formulation')
ok = True
for name, K, shape, spacing in (('K = 117 planes  644 x 337', 117, (337, 644), (1.5, 1.5)), ('K =  18 planes  600 x 512, spacing 0.8 x 2.5', 18, (512, 600), (0.8, 2.5)),
                                ('K = 117 planes   53 x 133', 117, (133, 53), (1.5, 1.5))):
    a, b = planes_pair(K, shape)
    ok &= overlap(name, a, E.PLANES, b, E.PLANES, list(range(1, K + 1)), shape)
    ok &= distances(name, a, b, spacing)
a, b = stack_pair(18, (64, 512, 512))
ok &= overlap('K =  18 label maps 64 x 512 x 512', a, E.LABELMAP, b, E.LABELMAP, list(range(1, 19)), (64, 512, 512))
ok &= projection('int16 133 x 120 x 53, num = 117', (133, 120, 53), 117)
ok &= projection('int16 512 x 512 x 600, num = 117', (600, 512, 512), 117)
sys.exit(0 if ok else 1)
