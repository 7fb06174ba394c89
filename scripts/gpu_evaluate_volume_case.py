"""Wall time of the boundary distances of volumes, the whole call with its uploads and downloads (csrc/kernels_evaluate_volume.h behind
evaluate._device_volume_distances), in ONE process, the routes alternating:
    device      ts2d_volume_surface_distances, the plain form (tolerance 2 mm) and the profile form (also the 95th percentile and the sum)
    statement   evaluate.volume_surface_statement / volume_distance_profile_statement on the host - at the SMALL size only: its second pass
                is O(Z H H W) per label and direction in numpy, which at the large size takes hours
    scipy       what a user would write: per label and direction, inside the label's joint bounding box grown by one voxel,
                ``distance_transform_edt`` of the other border read at the own border, then the count within the tolerance, ``np.percentile``
                and ``mean``
Cases: a label-map stack 64 x 512 x 512 with 18 labels at 1.5 x 0.8 x 0.8 mm - one label that fills most of the volume and 17 organ-like
ellipsoids and boxes in it, speckle-free; the other side is the same anatomy moved and resized by a few voxels -, and the same at 16 x 128 x 128.
Every figure is the median of N with its minimum and maximum; the device route is warmed up first.  Equality is asserted in every round: at the
small size device and statement bit for bit; at both sizes the device's border counts and counts within the tolerance equal scipy's, and its
Hausdorff distance, 95th percentile and mean agree with scipy's to 1e-9 relative (scipy's transform is not the statement's arithmetic).

    timeout -k 10 1100 python scripts/gpu_evaluate_volume_case.py [N=5] >> profiles/r34_volume_distances_case.txt   (exit status 0 = complete and equal)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from scipy import ndimage

from totalsegmentator2d_amd import evaluate as E

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5
DEVICE = None if os.environ.get('TS2D_EVALUATE_HOST_ONLY') else 0            # (host only: the host routes, on a machine without a GPU)
SIZES = [s for s in os.environ.get('TS2D_EVALUATE_SIZES', 'large,small').split(',') if s]
QS, TOL, K = (95.0,), (2.0,), 18
SPACING = (1.5, 0.8, 0.8)


def label_map(shape, seed, jitter):
    """label 1: an ellipsoid over most of the volume; labels 2 ... 18: ellipsoids and boxes inside it, later ones painted over earlier ones"""
    rng = np.random.default_rng(seed)                                        # the same anatomy on both sides: the seed is shared, the jitter is not
    jit = np.random.default_rng(seed + 1000 * jitter)
    Z, H, W = shape
    zz, yy, xx = np.meshgrid(np.arange(Z, dtype=np.float32), np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij', sparse=True)
    m = np.zeros(shape, np.uint8)
    m[((zz - Z / 2) / (Z * 0.55)) ** 2 + ((yy - H / 2) / (H * 0.46)) ** 2 + ((xx - W / 2) / (W * 0.47)) ** 2 <= 1.0] = 1
    for v in range(2, K + 1):
        c = [rng.uniform(0.2, 0.8) * s for s in shape]
        r = [max(1.5, rng.uniform(0.04, 0.16) * s) for s in shape]
        box = rng.random() < 0.3
        if jitter:
            c = [ci + jit.integers(-2, 3) for ci in c]
            r = [ri + jit.uniform(-1.0, 1.0) for ri in r]
        if box:
            m[(abs(zz - c[0]) <= r[0]) & (abs(yy - c[1]) <= r[1]) & (abs(xx - c[2]) <= r[2])] = v
        else:
            m[((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1.0] = v
    return m


def with_scipy(a, b, values, profile):
    out = []
    cross = ndimage.generate_binary_structure(3, 1)
    for v in values:
        ma, mb = a == v, b == v
        box = ndimage.find_objects((ma | mb).astype(np.uint8))
        if not box or box[0] is None:
            out.append(None)
            continue
        sl = tuple(slice(max(0, s.start - 1), min(n, s.stop + 1)) for s, n in zip(box[0], a.shape))
        ma, mb = ma[sl], mb[sl]
        ba, bb = ma & ~ndimage.binary_erosion(ma, cross), mb & ~ndimage.binary_erosion(mb, cross)
        res = []
        for own, other in ((ba, bb), (bb, ba)):
            d = ndimage.distance_transform_edt(~other, sampling=SPACING)[own] if other.any() else np.full(int(own.sum()), np.inf)
            with np.errstate(invalid='ignore'):
                res.append((int(own.sum()), float(d.max()) if len(d) else None, int((d <= TOL[0]).sum()),
                            float(np.percentile(d, QS[0])) if profile and len(d) else None, float(d.mean()) if profile and len(d) else None))
        out.append(res)
    return out


def close(x, y):
    return x == y or (x is not None and y is not None and abs(x - y) <= 1e-9 * max(abs(y), 1e-300))


def agrees_with_scipy(dev, sci, profile):
    ok = True
    for k, res in enumerate(sci):
        for d in range(2):
            n, top, within, pct, mean = res[d] if res else (0, None, 0, None, None)
            ok &= int(dev['border'][k, d]) == n and int(dev['within'][k, d, 0]) == within
            ok &= close(float(np.sqrt(dev['d2_max'][k, d])) if n else None, top)
            if profile and n:
                ok &= close(float(E.percentile_of_ranks(dev['d2_rank'][k, d, 0, 0], dev['d2_rank'][k, d, 0, 1], dev['rank_weight'][k, d, 0])), pct)
                ok &= close(float(dev['dist_sum'][k, d] / n), mean)
    return bool(ok)


def dicts_equal(x, y):
    return all(x[f].dtype == y[f].dtype and x[f].tobytes() == y[f].tobytes() for f in x)


def case(name, shape, with_statement):
    a, b = label_map(shape, 34, 0), label_map(shape, 34, 1)
    values = list(range(1, K + 1))
    ok = True
    for form, qs in (('plain', None), ('profile', list(QS))):
        profile = qs is not None
        routes = {'scipy': lambda: with_scipy(a, b, values, profile)}
        if with_statement:
            routes['statement'] = lambda: E._distance_walk('case', a, E.LABELMAP, b, E.LABELMAP, values, SPACING, TOL, qs, volume=True)
        if DEVICE is not None:
            routes = dict({'device': lambda: E._device_volume_distances(a, E.LABELMAP, b, E.LABELMAP, values, shape, SPACING, TOL, qs, profile, DEVICE)}, **routes)
            routes['device']()                                               # warm-up
        t = {r: [] for r in routes}
        got, same = {}, True
        for _ in range(N):                                                   # the routes alternate
            for r, fn in routes.items():
                t0 = time.perf_counter(); got[r] = fn(); t[r].append(time.perf_counter() - t0)
            if DEVICE is not None:
                same &= agrees_with_scipy(got['device'], got['scipy'], profile)
                if with_statement:
                    same &= dicts_equal(got['device'], got['statement'])
            elif with_statement:
                same &= agrees_with_scipy(got['statement'], got['scipy'], profile)
        med = {r: float(np.median(v)) for r, v in t.items()}
        line = f'    {name:34s} {form:8s}'
        for r in routes:
            line += f'   {r} {med[r] * 1e3:10.2f} ms (min {min(t[r]) * 1e3:10.2f}, max {max(t[r]) * 1e3:10.2f})'
        if DEVICE is not None:
            line += f'   scipy / device {med["scipy"] / med["device"]:8.2f}x'
            if with_statement:
                line += f'   statement / device {med["statement"] / med["device"]:8.2f}x'
        print(line + f'   equal: {same}', flush=True)
        ok &= same
    return ok


print(f'boundary distances of volumes, label maps of {K} labels at {SPACING} mm, median of {N}; device = ts2d_volume_surface_distances, the whole call with '
      f'uploads and downloads; statement = evaluate.volume_*_statement (small size only); scipy = edt inside the joint box, np.percentile, mean; '
      f'plain = tolerance 2 mm; profile = also the 95th percentile and the sum', flush=True)
ok = True
if 'large' in SIZES:
    ok &= case('64 x 512 x 512', (64, 512, 512), False)
if 'small' in SIZES:
    ok &= case('16 x 128 x 128', (16, 128, 128), True)
sys.exit(0 if ok else 1)
