"""Wall time of the label morphology: the device route (engine.label_morphology: ts2d_label_morphology, csrc/kernels_morph.h, the upload and the
download included) against
    statement     morphology.label_morphology_statement, the host route (the scan form in numpy)
    disc          scipy.ndimage.binary_dilation / binary_erosion(border_value=1) per label with the disc as structure, cropped to its radius: what a
                  user writes first
    edt           scipy.ndimage.distance_transform_edt(sampling) per label and a threshold: what a user writes for a large radius
in ONE process, the routes alternating.  Cases:
    117 x 644 x 337   the merged segmentation of a case, planes, 1.5 x 1.5 mm
    18 x 600 x 512    one sub-model, planes, 0.8 x 2.5 mm
    label map         18 labels, 512 x 512, 1 x 1 mm
    117 x 53 x 133    the small end, planes, 1 x 1 mm
each with radius 2 mm and 10 mm, dilate and open.  Every figure is the median of N with its minimum and maximum; the device route is warmed up
first; the device's output and counters are compared with the statement's byte for byte, and the masks of the two scipy routes with them.

    timeout -k 10 1100 python scripts/gpu_morphology_case.py [N=5] >> profiles/r39_morphology_case.txt        (exit status 0 = complete and equal)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from scipy import ndimage

from totalsegmentator2d_amd import _lib, engine, morphology

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
DEVICE = None if os.environ.get('TS2D_MORPHOLOGY_HOST_ONLY') else 0          # (host only: the host routes, on a machine without a GPU)
rng = np.random.default_rng(39)
SPECKLE = 0.005


def planes_case(K, shape):
    planes = np.zeros((K,) + shape, np.uint8)
    for k in range(K):                                               # a blob per label with pin-holes, and speckle around it
        cy, cx = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        planes[k, max(cy - 40, 0):cy + 40, max(cx - 30, 0):cx + 30] = 1
    planes[rng.random(planes.shape) < SPECKLE] ^= 1
    return planes, None


def map_case(K, shape):
    a = np.zeros(shape, np.uint8)
    for k in range(K):
        cy, cx = (rng.integers(0, s) for s in shape)
        a[max(cy - 60, 0):cy + 60, max(cx - 50, 0):cx + 50] = k + 1
    at = rng.random(shape) < SPECKLE
    a[at] = rng.integers(0, K + 1, int(at.sum()))
    return a, list(range(1, K + 1))


def small_disc(r, sy, sx):
    ny, nx = int(r / sy) + 1, int(r / sx) + 1
    return morphology.sd_candidate(np.abs(np.arange(-ny, ny + 1))[:, None], np.abs(np.arange(-nx, nx + 1))[None, :], sy, sx) <= np.float64(r) * np.float64(r)


def by_disc(B):
    def dil(m):
        return ndimage.binary_dilation(m, structure=B)

    def ero(m):
        return ndimage.binary_erosion(m, structure=B, border_value=1)
    return dil, ero


def by_edt(r, sp):
    def dil(m):
        return ndimage.distance_transform_edt(~m, sampling=sp) <= r if m.any() else m.copy()

    def ero(m):
        return ndimage.distance_transform_edt(m, sampling=sp) > r if not m.all() else m.copy()
    return dil, ero


def user(seg, values, op, dil, ero):
    """What a user writes: per label a mask, the operation, and the label rules of morphology.py."""
    out = seg.copy()
    for k in range(seg.shape[0] if values is None else len(values)):
        m = seg[k] > 0 if values is None else seg == values[k]
        res = dil(m) if op == 'dilate' else dil(ero(m))
        if values is None:
            out[k][res & ~m] = 1
            out[k][~res] = 0
        elif op == 'dilate':
            out[res & (out == 0)] = values[k]
        else:
            out[m & ~res] = 0
    return out


def run(name, seg, values, sp, r, op):
    kind = _lib.STATS_PLANES if values is None else _lib.STATS_LABELMAP
    B = small_disc(r, *sp)
    routes = {'statement': lambda: morphology.label_morphology_statement(seg, values, op, r, sp),
              'disc': lambda: user(seg, values, op, *by_disc(B)), 'edt': lambda: user(seg, values, op, *by_edt(r, sp))}
    if DEVICE is not None:
        routes = dict({'device': lambda: engine.label_morphology(seg, kind, values, seg.shape[-2:], sp, morphology.OPS.index(op), r, device=DEVICE)}, **routes)
        routes['device']()                                           # warm-up
    t = {k: [] for k in routes}
    got = {}
    same = {k: True for k in routes if k != 'statement'}
    for _ in range(N):                                               # the routes alternate
        for k, fn in routes.items():
            t0 = time.perf_counter(); got[k] = fn(); t[k].append(time.perf_counter() - t0)
        want = got['statement']
        if 'device' in got:
            same['device'] &= all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got['device'], want))
        same['disc'] &= got['disc'].tobytes() == want[0].tobytes()
        same['edt'] &= got['edt'].tobytes() == want[0].tobytes()
    med = {k: float(np.median(v)) for k, v in t.items()}
    line = f'    {name:30s} {op:6s} {r:4.0f} mm   added {int(want[1][:, 2].sum()):8d} removed {int(want[1][:, 3].sum()):8d}'
    for k in routes:
        line += f'   {k} {med[k] * 1e3:9.2f} ms (min {min(t[k]) * 1e3:9.2f}, max {max(t[k]) * 1e3:9.2f})'
    if DEVICE is not None:
        line += '   ' + '   '.join(f'{k} / device {med[k] / med["device"]:7.2f}x' for k in ('statement', 'disc', 'edt'))
    print(line + '   equal to the statement: ' + ', '.join(f'{k} {v}' for k, v in same.items()), flush=True)
    return all(same.values())


print(f'label morphology, median of {N}; device = engine.label_morphology with upload and download, statement = morphology.label_morphology_statement, '
      f'disc = scipy binary_dilation / binary_erosion(border_value=1) per label, edt = scipy distance_transform_edt per label and a threshold')
ok = True
for name, (seg, values), sp in (('K = 117 planes  644 x 337', planes_case(117, (337, 644)), (1.5, 1.5)),
                                ('K =  18 planes  600 x 512', planes_case(18, (512, 600)), (0.8, 2.5)),
                                ('K =  18 label map 512 x 512', map_case(18, (512, 512)), (1.0, 1.0)),
                                ('K = 117 planes   53 x 133', planes_case(117, (133, 53)), (1.0, 1.0))):
    for r in (2.0, 10.0):
        for op in ('dilate', 'open'):
            ok &= run(name, seg, values, sp, r, op)
sys.exit(0 if ok else 1)
