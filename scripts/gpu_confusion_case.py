"""Wall time of the confusion matrix on the device, the whole call with its uploads and its download (csrc/kernels_confusion.h behind
evaluate._device_confusion), against the host statement evaluate.confusion_statement and against what a user would write in numpy, in ONE process,
the routes alternating:
    two label maps   np.bincount(a_class * (K + 1) + b_class) over the class indices of the two maps
    planes           A.astype(int64) @ B.T over the [K + 2, N] indicator rows
and, on the same input, the device time of ts2d_label_overlap (the three counts per label the matrix contains).
Cases (those of scripts/gpu_evaluate_case.py): 117 planes at 644 x 337; 18 planes at 600 x 512; a label-map stack 64 x 512 x 512 with 18 labels;
117 planes at 53 x 133.  Every figure is the median of N with its minimum and maximum; the device route is warmed up first; the results of the
routes are compared in every round (equal: integer for integer).

    timeout -k 10 1100 python scripts/gpu_confusion_case.py [N=5] >> profiles/r37_confusion_case.txt        (exit status 0 = complete and equal)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from totalsegmentator2d_amd import evaluate as E

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
DEVICE = None if os.environ.get('TS2D_EVALUATE_HOST_ONLY') else 0            # (host only: the host routes, on a machine without a GPU)
rng = np.random.default_rng(37)


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


def plain_maps(a, b, values):
    K = len(values)
    cls = np.zeros(256, np.int64)
    cls[values] = np.arange(1, K + 1)
    inner = np.bincount(cls[a.reshape(-1)] * (K + 1) + cls[b.reshape(-1)], minlength=(K + 1) ** 2).reshape(K + 1, K + 1)
    M = np.zeros((K + 2, K + 2), np.int64)
    M[:K + 1, :K + 1] = inner
    M[:K + 1, K + 1], M[K + 1, :K + 1], M[K + 1, K + 1] = inner.sum(axis=1), inner.sum(axis=0), a.size
    return M


def plain_planes(a, b):
    def rows(x):
        m = x.reshape(x.shape[0], -1) != 0
        return np.concatenate([~m.any(axis=0, keepdims=True), m, np.ones((1, m.shape[1]), bool)]).astype(np.int64)
    return rows(a) @ rows(b).T


def timed(name, routes):
    if 'device' in routes:
        routes['device']()                                           # warm-up
    t = {r: [] for r in routes}
    got, same = {}, True
    for _ in range(N):                                               # the routes alternate
        for r, fn in routes.items():
            t0 = time.perf_counter(); got[r] = fn(); t[r].append(time.perf_counter() - t0)
        same &= all(np.array_equal(got[r], got['statement']) for r in routes if r != 'overlap entry')
        if 'overlap entry' in routes:
            K = got['statement'].shape[0] - 2
            d = np.arange(1, K + 1)
            same &= np.array_equal(np.stack([got['statement'][d, K + 1], got['statement'][K + 1, d], got['statement'][d, d]], 1), got['overlap entry'])
    med = {r: float(np.median(v)) for r, v in t.items()}
    line = f'    {name:44s}'
    for r in routes:
        line += f'   {r} {med[r] * 1e3:9.2f} ms (min {min(t[r]) * 1e3:9.2f}, max {max(t[r]) * 1e3:9.2f})'
    if 'device' in routes:
        line += ''.join(f'   {r} / device {med[r] / med["device"]:7.2f}x' for r in routes if r != 'device')
    print(line + f'   equal: {same}', flush=True)
    return same


def case(name, a, kind_a, b, kind_b, values, spatial):
    plain = (lambda: plain_maps(a, b, values)) if kind_a == kind_b == E.LABELMAP else (lambda: plain_planes(a, b))
    routes = {'statement': lambda: E.confusion_statement(a, kind_a, b, kind_b, values), 'plain numpy': plain}
    if DEVICE is not None:
        from totalsegmentator2d_amd import engine
        zhw = (1,) * (3 - len(spatial)) + tuple(spatial)
        routes = dict({'device': lambda: E._device_confusion(a, kind_a, b, kind_b, values, spatial, DEVICE)}, **routes,
                      **{'overlap entry': lambda: engine.label_overlap(a, kind_a, b, kind_b, values, zhw, DEVICE)})
    return timed(name, routes)


print(f'confusion matrix, median of {N}; device = the whole call ts2d_label_confusion with uploads and download, statement = '
      f'evaluate.confusion_statement on the host, plain numpy = bincount (two label maps) or int64 matrix product (planes), overlap entry = the '
      f'whole call ts2d_label_overlap on the same input')
ok = True
for name, K, shape in (('K = 117 planes  644 x 337', 117, (337, 644)), ('K =  18 planes  600 x 512', 18, (512, 600))):
    a, b = planes_pair(K, shape)
    ok &= case(name, a, E.PLANES, b, E.PLANES, list(range(1, K + 1)), shape)
a, b = stack_pair(18, (64, 512, 512))
ok &= case('K =  18 label maps 64 x 512 x 512', a, E.LABELMAP, b, E.LABELMAP, list(range(1, 19)), (64, 512, 512))
a, b = planes_pair(117, (133, 53))
ok &= case('K = 117 planes   53 x 133', a, E.PLANES, b, E.PLANES, list(range(1, 118)), (133, 53))
sys.exit(0 if ok else 1)
