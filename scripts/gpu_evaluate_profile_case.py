"""Wall time of the distance profile, the whole call with its uploads and downloads (csrc/kernels_evaluate_profile.h behind
evaluate._device_profile), in ONE process, the routes alternating, in the set-up and at the geometries of scripts/gpu_evaluate_case.py:
    (a) device / statement    evaluate.distance_profile_statement on the host
    (b) device / scipy        what a user would write: per label and direction ``distance_transform_edt`` of the other border read at the own
                              border, then ``np.percentile`` and ``mean``
    (c) profile / distances   ts2d_surface_distance_profile against ts2d_surface_distances ALONE on the same input: the price of the extras
Requested: the 95th percentile and the sum, with the tolerance 2 mm.  Cases: 117 planes at 644 x 337; 18 planes at 600 x 512 with spacing
0.8 x 2.5 (mm per row, per column); 117 planes at 53 x 133.  Every figure is the median of N with its minimum and maximum; the device routes are
warmed up first; the results of device and statement are compared in every round (equal: bit for bit).

    timeout -k 10 1100 python scripts/gpu_evaluate_profile_case.py [N=5] >> profiles/r30_distance_profile_case.txt   (exit status 0 = complete and equal)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from scipy import ndimage

from totalsegmentator2d_amd import evaluate as E

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
DEVICE = None if os.environ.get('TS2D_EVALUATE_HOST_ONLY') else 0            # (host only: the host routes, on a machine without a GPU)
QS, TOL = (95.0,), (2.0,)
rng = np.random.default_rng(30)


def planes_pair(K, shape):
    """a blob per label, overlapping its neighbours; the other side is the same blob moved by a few pixels (scripts/gpu_evaluate_case.py)"""
    a, b = np.zeros((K,) + shape, np.uint8), np.zeros((K,) + shape, np.uint8)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    for k in range(K):
        cy, cx = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        ry, rx = max(2, shape[0] // 8), max(2, shape[1] // 10)
        a[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        b[k] = ((yy - cy - rng.integers(-3, 4)) / ry) ** 2 + ((xx - cx - rng.integers(-3, 4)) / (rx + 1)) ** 2 <= 1.0
    return a, b


def dicts_equal(x, y):
    return all(x[f].dtype == y[f].dtype and x[f].tobytes() == y[f].tobytes() for f in x)


def case(name, a, b, spacing):
    hw = a.shape[1:]

    def with_scipy():
        out = []
        for k in range(a.shape[0]):
            ma, mb = a[k] > 0, b[k] > 0
            ba, bb = ma & ~ndimage.binary_erosion(ma), mb & ~ndimage.binary_erosion(mb)
            for own, other in ((ba, bb), (bb, ba)):
                d = ndimage.distance_transform_edt(~other, sampling=spacing)[own] if other.any() else np.full(int(own.sum()), np.inf)
                with np.errstate(invalid='ignore'):
                    out.append((int(own.sum()), float(d.max()) if len(d) else None, int((d <= TOL[0]).sum()),
                                float(np.percentile(d, QS[0])) if len(d) else None, float(d.mean()) if len(d) else None))
        return out
    routes = {'statement': lambda: E.distance_profile_statement(a, E.PLANES, b, E.PLANES, None, spacing, TOL, QS), 'scipy': with_scipy}
    if DEVICE is not None:
        routes = dict({'profile': lambda: E._device_profile(a, E.PLANES, b, E.PLANES, None, hw, spacing, TOL, QS, True, DEVICE),
                       'distances alone': lambda: E._device_surface(a, E.PLANES, b, E.PLANES, None, hw, spacing, TOL, DEVICE)}, **routes)
        routes['profile'](); routes['distances alone']()             # warm-up
    t = {r: [] for r in routes}
    got, same = {}, True
    for _ in range(N):                                               # the routes alternate
        for r, fn in routes.items():
            t0 = time.perf_counter(); got[r] = fn(); t[r].append(time.perf_counter() - t0)
        if DEVICE is not None:
            same &= dicts_equal(got['profile'], got['statement']) and dicts_equal(got['distances alone'], got['profile'])
    med = {r: float(np.median(v)) for r, v in t.items()}
    line = f'    {name:46s}'
    for r in routes:
        line += f'   {r} {med[r] * 1e3:9.2f} ms (min {min(t[r]) * 1e3:9.2f}, max {max(t[r]) * 1e3:9.2f})'
    if DEVICE is not None:
        line += (f'   (a) statement / profile {med["statement"] / med["profile"]:7.2f}x   (b) scipy / profile {med["scipy"] / med["profile"]:7.2f}x'
                 f'   (c) profile / distances alone {med["profile"] / med["distances alone"]:5.2f}x')
    print(line + f'   equal: {same}', flush=True)
    return same


print(f'distance profile (95th percentile and sum), median of {N}; profile = ts2d_surface_distance_profile, the whole call with uploads and downloads; '
      f'distances alone = ts2d_surface_distances; statement = evaluate.distance_profile_statement; scipy = edt, np.percentile, mean')
ok = True
for name, K, shape, spacing in (('K = 117 planes  644 x 337', 117, (337, 644), (1.5, 1.5)), ('K =  18 planes  600 x 512, spacing 0.8 x 2.5', 18, (512, 600), (0.8, 2.5)),
                                ('K = 117 planes   53 x 133', 117, (133, 53), (1.5, 1.5))):
    a, b = planes_pair(K, shape)
    ok &= case(name, a, b, spacing)
sys.exit(0 if ok else 1)
