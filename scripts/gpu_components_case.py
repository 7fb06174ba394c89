"""Wall time of the components of every label at once: the device route (engine.label_components: ts2d_label_components,
csrc/kernels_components.h, the upload and the download included; cleaned array, counters and list, rule keep_largest: ONE call of the entry up to
65 536 components, two beyond; "device, no list": cleaned array and counters only, one call, what the old entry returns) against
    statement     components.label_components_statement, the host route
    scipy         scipy.ndimage.label + np.bincount per label, as a user would write "keep the largest blob" (the cleaned array only)
    old entry     for label maps: K single-label steps of ts2d_keep_largest_components, the only device way before this entry
in ONE process, the routes alternating.  Cases (those of scripts/gpu_statistics_case.py, with 0.5 % speckle added):
    117 x 644 x 337   the merged segmentation of a case, planes
    18 x 600 x 512    one sub-model, planes
    stack             a label map 64 x 512 x 512 with 18 labels
    117 x 53 x 133    the small end, planes
Every figure is the median of N with its minimum and maximum; the device route is warmed up first; the device's three outputs are compared with
the statement's byte for byte, and the cleaned arrays of the other routes with them.

    timeout -k 10 1100 python scripts/gpu_components_case.py [N=5] >> profiles/r36_components_case.txt        (exit status 0 = complete and equal)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from scipy import ndimage

from totalsegmentator2d_amd import _lib, components, engine

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
DEVICE = None if os.environ.get('TS2D_COMPONENTS_HOST_ONLY') else 0          # (host only: the two host routes, on a machine without a GPU)
rng = np.random.default_rng(36)
SPECKLE = 0.005


def planes_case(K, shape):
    planes = np.zeros((K,) + shape, np.uint8)
    for k in range(K):                                               # a blob per label, overlapping its neighbours
        cy, cx = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        planes[k, max(cy - 40, 0):cy + 40, max(cx - 30, 0):cx + 30] = 1
    planes[rng.random(planes.shape) < SPECKLE] = 1
    return planes, None


def stack_case(K, shape):
    a = np.zeros(shape, np.uint8)
    for k in range(K):
        cz, cy, cx = (rng.integers(0, s) for s in shape)
        a[max(cz - 12, 0):cz + 12, max(cy - 60, 0):cy + 60, max(cx - 50, 0):cx + 50] = k + 1
    at = rng.random(shape) < SPECKLE
    a[at] = rng.integers(1, K + 1, int(at.sum()))
    return a, list(range(1, K + 1))


def plain(seg, values):
    """What a user writes with scipy: per label a mask, its labelling, the sizes, the largest kept."""
    out = seg.copy()
    structure = np.ones((3,) * (seg.ndim - (values is None)), bool)
    for k in range(seg.shape[0] if values is None else len(values)):
        mask = seg[k] > 0 if values is None else seg == values[k]
        lab, n = ndimage.label(mask, structure=structure)
        if n:
            sizes = np.bincount(lab.ravel())
            sizes[0] = 0
            (out[k] if values is None else out)[mask & (sizes < sizes.max())[lab]] = 0
    return out


def old_entry(seg, values):
    tables = np.zeros((len(values), 256), np.uint8)
    tables[np.arange(len(values)), values] = 1
    return engine.keep_largest_components(seg, tables, np.zeros(len(values), np.uint8), device=DEVICE)[0]


def run(name, seg, values):
    spatial = seg.shape[1:] if values is None else seg.shape
    zhw = ((1,) + tuple(spatial))[-3:]
    kind = _lib.STATS_PLANES if values is None else _lib.STATS_LABELMAP
    routes = {'statement': lambda: components.label_components_statement(seg, values, 'full', True), 'scipy': lambda: plain(seg, values)}
    if DEVICE is not None:
        routes = dict({'device': lambda: engine.label_components(seg, kind, values, zhw, _lib.COMP_FULL, True, device=DEVICE)}, **routes)
        routes['device, no list'] = lambda: engine.label_components(seg, kind, values, zhw, _lib.COMP_FULL, True, want_list=False, device=DEVICE)
        routes['device']()                                           # warm-up
        if values is not None:
            routes['old entry'] = lambda: old_entry(seg, values)
            routes['old entry']()
    t = {r: [] for r in routes}
    got = {}
    same = True
    for _ in range(N):                                               # the routes alternate
        for r, fn in routes.items():
            t0 = time.perf_counter(); got[r] = fn(); t[r].append(time.perf_counter() - t0)
        want = got['statement']
        if 'device' in got:
            same &= got['device'] is not None and all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got['device'], want))
            same &= got['device, no list'][0].tobytes() == want[0].tobytes() and got['device, no list'][1].tobytes() == want[1].tobytes()
        same &= got['scipy'].tobytes() == want[0].tobytes() and ('old entry' not in got or got['old entry'].tobytes() == want[0].tobytes())
    med = {r: float(np.median(v)) for r, v in t.items()}
    line = f'    {name:36s} components {len(want[2]):7d} removed {int(want[1][:, 4].sum()):7d}'
    for r in routes:
        line += f'   {r} {med[r] * 1e3:9.2f} ms (min {min(t[r]) * 1e3:9.2f}, max {max(t[r]) * 1e3:9.2f})'
    if DEVICE is not None:
        line += f'   statement / device {med["statement"] / med["device"]:7.2f}x   scipy / device {med["scipy"] / med["device"]:7.2f}x'
        if 'old entry' in med:
            line += f'   old entry / device, no list {med["old entry"] / med["device, no list"]:7.2f}x'
    print(line + f'   equal: {same}', flush=True)
    return same


print(f'components of every label at once, keep_largest, full connectivity, median of {N}; device = engine.label_components with upload and download '
      f'(cleaned array, counters, list; no list: one call without it), statement = components.label_components_statement, scipy = label + bincount per label, '
      f'old entry = K single-label steps of ts2d_keep_largest_components')
ok = run('K = 117 planes  644 x 337', *planes_case(117, (337, 644)))
ok &= run('K =  18 planes  600 x 512', *planes_case(18, (512, 600)))
ok &= run('K =  18 label map 64 x 512 x 512', *stack_case(18, (64, 512, 512)))
ok &= run('K = 117 planes   53 x 133', *planes_case(117, (133, 53)))
sys.exit(0 if ok else 1)
