"""Wall time of the percentiles under a label for q = (5, 50, 95): the device route (ts2d_label_percentiles, csrc/kernels_stats_select.h, with upload,
download and the interpolation on the host: statistics._device_percentiles) against the host statement (statistics.label_percentiles_statement)
and against what a user would write (np.percentile(x[mask], q) per label and channel), in ONE process, the routes alternating; and, on the same
input in the same process, ts2d_label_statistics alone (statistics._device_statistics): the price of the percentiles over it.  Cases, the
geometries of scripts/gpu_statistics_case.py:
    117 x 644 x 337   the merged segmentation of a case (plane-major memory), 2 channels
    18 x 600 x 512    one sub-model, 2 channels
    stack             a label map 64 x 512 x 512 with 18 labels, 1 channel
    117 x 53 x 133    the small end, 2 channels
    stack, constant   the stack with ONE intensity everywhere: every lane of a wave on one bin of the LDS histogram, in every round
Every figure is the median of N with its minimum and maximum; the device route is warmed up first; device and statement are compared bit for bit
(counts, rank values, weights, percentiles), the user's numpy within 1e-12 relative.

    timeout -k 10 1100 python scripts/gpu_statistics_percentiles_case.py [N=5] >> profiles/r35_statistics_percentiles_case.txt   (exit status 0 = complete and equal)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from totalsegmentator2d_amd import statistics as S

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
DEVICE = None if os.environ.get('TS2D_STATISTICS_HOST_ONLY') else 0          # (host only: the two host routes, on a machine without a GPU)
QS = [5.0, 50.0, 95.0]
rng = np.random.default_rng(35)


def planes_case(K, shape):
    planes = np.zeros((K,) + shape, np.uint8)
    for k in range(K):                                               # a blob per label, overlapping its neighbours
        cy, cx = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        planes[k, max(cy - 40, 0):cy + 40, max(cx - 30, 0):cx + 30] = 1
    return planes, None


def stack_case(K, shape):
    a = np.zeros(shape, np.uint8)
    for k in range(K):
        cz, cy, cx = (rng.integers(0, s) for s in shape)
        a[max(cz - 12, 0):cz + 12, max(cy - 60, 0):cy + 60, max(cx - 50, 0):cx + 50] = k + 1
    return a, list(range(1, K + 1))


def plain(seg, values, x):
    """What a user writes with numpy: per label a boolean mask, per channel np.percentile of the boolean-indexed samples."""
    K = seg.shape[0] if values is None else len(values)
    out = np.zeros((K, x.shape[0], len(QS)), np.float64)
    for k in range(K):
        mask = seg[k] > 0 if values is None else seg == values[k]
        if mask.any():
            for c in range(x.shape[0]):
                out[k, c] = np.percentile(x[c][mask], QS)
    return out


def run(name, case, C, constant=False):
    seg, values = case
    spatial = seg.shape if values is not None else seg.shape[1:]
    x = np.full((C,) + spatial, 100.0, np.float32) if constant else (rng.normal(size=(C,) + spatial) * 400 + 100).astype(np.float32)
    routes = {'statement': lambda: S.label_percentiles_statement(seg, x, QS, values), 'plain numpy': lambda: plain(seg, values, x)}
    if DEVICE is not None:
        routes = dict({'device': lambda: S._device_percentiles(seg, values, spatial, x, QS, DEVICE),
                       'statistics alone': lambda: S._device_statistics(seg, values, spatial, x, (1.0,) * len(spatial), DEVICE)}, **routes)
        routes['device'](); routes['statistics alone']()             # warm-up
    t = {r: [] for r in routes}
    got = {}
    same = True
    for _ in range(N):                                               # the routes alternate
        for r, fn in routes.items():
            t0 = time.perf_counter(); got[r] = fn(); t[r].append(time.perf_counter() - t0)
        st = got['statement']
        if DEVICE is not None:
            dev = got['device']
            same &= dev is not None and np.array_equal(dev['count'], st['count']) and all(
                np.array_equal(dev[f].view(np.uint8), st[f].view(np.uint8)) for f in ('rank_value', 'rank_weight', 'percentile'))
        same &= bool((np.abs(got['plain numpy'] - st['percentile']) <= 1e-12 * np.abs(st['percentile'])).all())
    med = {r: float(np.median(v)) for r, v in t.items()}
    line = f'    {name:52s}'
    for r in routes:
        line += f'   {r} {med[r] * 1e3:9.2f} ms (min {min(t[r]) * 1e3:9.2f}, max {max(t[r]) * 1e3:9.2f})'
    if DEVICE is not None:
        line += (f'   statement / device {med["statement"] / med["device"]:7.2f}x   plain / device {med["plain numpy"] / med["device"]:7.2f}x'
                 f'   device / statistics alone {med["device"] / med["statistics alone"]:5.2f}x')
    print(line + f'   equal: {same}', flush=True)
    return same


print(f'percentiles under a label, q = (5, 50, 95), median of {N}; device = ts2d_label_percentiles with upload, download and the interpolation, statement = '
      f'label_percentiles_statement, plain numpy = np.percentile(x[mask], q) per label and channel, statistics alone = ts2d_label_statistics on the same input')
ok = run('K = 117 planes  644 x 337, 2 channels', planes_case(117, (337, 644)), 2)
ok &= run('K =  18 planes  600 x 512, 2 channels', planes_case(18, (512, 600)), 2)
stack = stack_case(18, (64, 512, 512))
ok &= run('K =  18 label map 64 x 512 x 512, 1 channel', stack, 1)
ok &= run('K = 117 planes   53 x 133, 2 channels', planes_case(117, (133, 53)), 2)
ok &= run('K =  18 label map 64 x 512 x 512, constant intensity', stack, 1, constant=True)
sys.exit(0 if ok else 1)
