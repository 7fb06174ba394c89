"""Wall time of the per-label statistics: the device route (statistics.label_statistics(device=0): ts2d_label_statistics, csrc/kernels_stats.h, the
upload and the download included) against the host statement (device=None, statistics.label_statistics_statement) and against the plain per-label
numpy formulation a user would write (boolean index per label and channel: count, argwhere for box and centroid, min / max / mean / std), in ONE
process, the routes alternating.  Cases:
    117 x 644 x 337   the merged segmentation of a case (plane-major memory, as combine_segmentations hands it out), 2 channels
    18 x 600 x 512    one sub-model, 2 channels
    stack             a label map 64 x 512 x 512 with 18 labels, 1 channel
    117 x 53 x 133    the projections of the 3-D sample asset: the small end, 2 channels
Every figure is the median of N with its minimum and maximum; the device route is warmed up first; the dicts of device and statement are compared
(equal: bit for bit, they hold Python floats) and the plain formulation's counts with them.

    timeout -k 10 1100 python scripts/gpu_statistics_case.py [N=5] >> profiles/r28_statistics_case.txt        (exit status 0 = complete and equal)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from totalsegmentator2d_amd import image, nrrd, statistics

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
DEVICE = None if os.environ.get('TS2D_STATISTICS_HOST_ONLY') else 0          # (host only: the two host routes, on a machine without a GPU)
rng = np.random.default_rng(28)


def planes_case(K, shape):
    planes = np.zeros((K,) + shape, np.uint8)
    for k in range(K):                                               # a blob per label, overlapping its neighbours
        cy, cx = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        planes[k, max(cy - 40, 0):cy + 40, max(cx - 30, 0):cx + 30] = 1
    seg = nrrd.Image(np.moveaxis(planes, 0, -1), (1.5, 1.5), (0.0, 0.0), (1.0, 0.0, 0.0, 1.0), K, {}, None)
    image.set_annotation_meta(seg, {i + 1: f'label{i}' for i in range(K)})
    return seg


def stack_case(K, shape):
    a = np.zeros(shape, np.uint8)
    for k in range(K):
        cz, cy, cx = (rng.integers(0, s) for s in shape)
        a[max(cz - 12, 0):cz + 12, max(cy - 60, 0):cy + 60, max(cx - 50, 0):cx + 50] = k + 1
    seg = nrrd.Image(a, (1.5, 1.5, 3.0), (0.0, 0.0, 0.0), tuple(float(v) for v in np.eye(3).reshape(-1)), 1, {}, None)
    image.set_annotation_meta(seg, {i + 1: f'label{i}' for i in range(K)})
    return seg


def plain(seg, chans):
    """What a user writes with numpy: per label a boolean mask, per channel a boolean-indexed reduction."""
    out = {}
    for name, info in image.get_annotation_labels(seg).items():
        mask = seg.array[..., info['value'] - 1] > 0 if seg.components > 1 else seg.array == info['value']
        n = int(np.count_nonzero(mask))
        e = {'count': n}
        if n:
            at = np.argwhere(mask)
            e['bbox'] = [at.min(0).tolist(), at.max(0).tolist()]
            e['centroid_index'] = at.mean(0).tolist()
            for c, x in chans.items():
                v = x[mask]
                e[c] = (float(v.min()), float(v.max()), float(v.mean(dtype=np.float64)), float(v.std(dtype=np.float64)))
        out[name] = e
    return out


def run(name, seg, C):
    spatial = seg.array.shape[:seg.dimension]
    chans = {f'ch{c}': (rng.normal(size=spatial) * 400 + 100).astype(np.float32) for c in range(C)}
    routes = {'statement': lambda: statistics.label_statistics(seg, chans), 'plain numpy': lambda: plain(seg, chans)}
    if DEVICE is not None:
        routes = dict({'device': lambda: statistics.label_statistics(seg, chans, device=DEVICE)}, **routes)
        routes['device']()                                           # warm-up
    t = {r: [] for r in routes}
    got = {}
    same = True
    for _ in range(N):                                               # the routes alternate
        for r, fn in routes.items():
            t0 = time.perf_counter(); got[r] = fn(); t[r].append(time.perf_counter() - t0)
        same &= got.get('device', got['statement']) == got['statement']
        same &= all(got['plain numpy'][n]['count'] == e['count'] and got['plain numpy'][n].get('bbox') == e['bbox'] for n, e in got['statement'].items())
    med = {r: float(np.median(v)) for r, v in t.items()}
    line = f'    {name:44s}'
    for r in routes:
        line += f'   {r} {med[r] * 1e3:9.2f} ms (min {min(t[r]) * 1e3:9.2f}, max {max(t[r]) * 1e3:9.2f})'
    if DEVICE is not None:
        line += f'   statement / device {med["statement"] / med["device"]:7.2f}x   plain / device {med["plain numpy"] / med["device"]:7.2f}x'
    print(line + f'   equal: {same}', flush=True)
    return same


print(f'per-label statistics, median of {N}; device = statistics.label_statistics(device=0) with upload and download, statement = device=None, '
      f'plain numpy = one boolean-indexed reduction per label and channel')
ok = run('K = 117 planes  644 x 337, 2 channels', planes_case(117, (337, 644)), 2)
ok &= run('K =  18 planes  600 x 512, 2 channels', planes_case(18, (512, 600)), 2)
ok &= run('K =  18 label map 64 x 512 x 512, 1 channel', stack_case(18, (64, 512, 512)), 1)
ok &= run('K = 117 planes   53 x 133, 2 channels', planes_case(117, (133, 53)), 2)
sys.exit(0 if ok else 1)
