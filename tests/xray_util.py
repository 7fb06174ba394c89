"""TEST INFRASTRUCTURE for the synthetic radiograph: the definition of totalsegmentator2d_amd/xray.py once more as a scalar loop per ray, in
plain Python floats (IEEE doubles, every operation rounded on its own), sharing nothing with the module - not its tables, not its density, not
its detector size.  tests/test_xray_cpu.py holds the statements against it, tests/test_gpu_xray.py the device entries against the statements."""
import math

import numpy as np

from totalsegmentator2d_amd import nrrd

EXTENTS = [(5, 37, 66), (3, 2, 63), (1, 1, 1), (7, 9, 130)]                    # (nz, ny, nx) of the statement checks
GPU_EXTENTS = EXTENTS + [(66, 4, 5), (2, 1, 64), (2, 3, 65)]


def detector(shape, spacing, sdd=1800.0, sod=1500.0, parallel=False, du=None, dv=None, size=None):
    """(du, dv, nu, nv) as the issue states the defaults."""
    nz, ny, nx = shape
    sx, sy, sz = spacing
    if parallel:
        return sx, sz, nx, nz
    du, dv = sx if du is None else du, sz if dv is None else dv
    if size is not None:
        return du, dv, size[0], size[1]
    M = sdd / sod
    return du, dv, math.ceil(nx * sx * M / du), math.ceil(nz * sz * M / dv)


def per_ray(vol, spacing, sdd=1800.0, sod=1500.0, view='ap', parallel=False, du=None, dv=None, size=None, air=-1000.0, water=0.0, density_max=None,
            num=None):
    """The radiograph of ``vol`` [nz][ny][nx] as (float64 sums, float32 image), or with ``num`` the uint8 label planes [num][nv][nu]."""
    nz, ny, nx = vol.shape
    sx, sy, sz = (float(s) for s in spacing)
    du, dv, nu, nv = detector(vol.shape, (sx, sy, sz), sdd, sod, parallel, du, dv, size)
    Cx, Cy, Cz = (nx - 1) * sx / 2, (ny - 1) * sy / 2, (nz - 1) * sz / 2
    sign = 1.0 if view == 'ap' else -1.0
    Sy = Cy - sign * sod
    Yd = Sy + sign * sdd
    den = Yd - Sy
    scale = 1.0 / (water - air)
    sums = np.zeros((nv, nu), np.float64)
    xr = np.zeros((nv, nu), np.float32)
    planes = np.zeros((num or 1, nv, nu), np.uint8)

    def density(j, zz, xx):
        if not (0 <= zz < nz and 0 <= xx < nx):
            return 0.0
        d = (float(vol[zz, j, xx]) - air) * scale
        d = d if d > 0 else 0.0
        return density_max if density_max is not None and d > density_max else d

    for k in range(nv):
        V = Cz + (k - (nv - 1) / 2) * dv
        for i in range(nu):
            U = Cx + (i - (nu - 1) / 2) * du
            if parallel:
                a = b = 0.0
                cx, cz, step = float(i), float(k), sy
            else:
                a, b, cx, cz = (U - Cx) / sx, (V - Cz) / sz, Cx / sx, Cz / sz
                p, q = (U - Cx) / den, (V - Cz) / den
                step = sy * math.sqrt((1 + p * p) + q * q)
            acc = 0.0
            for j in range(ny):
                t = 0.0 if parallel else (j * sy - Sy) / den
                x, z = cx + t * a, cz + t * b
                if num is not None:
                    xi, zi = math.floor(x + 0.5), math.floor(z + 0.5)
                    if 0 <= xi < nx and 0 <= zi < nz and vol[zi, j, xi] != 0:
                        planes[int(vol[zi, j, xi]) - 1, k, i] = 1
                    continue
                if not (-1 < x < nx and -1 < z < nz):
                    continue
                x0, z0 = math.floor(x), math.floor(z)
                fx, fz = x - x0, z - z0
                r0 = density(j, z0, x0) * (1 - fx) + density(j, z0, x0 + 1) * fx
                r1 = density(j, z0 + 1, x0) * (1 - fx) + density(j, z0 + 1, x0 + 1) * fx
                acc += r0 * (1 - fz) + r1 * fz
            sums[k, i] = acc
            xr[k, i] = np.float32(acc * step)
    return planes if num is not None else (sums, xr)


def ct_volume(shape, dtype, seed):
    """Samples around air, water and bone, with the type's limits among them."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        v = rng.normal(-300.0, 600.0, shape).astype(dt)
        v.reshape(-1)[::7] = np.round(v.reshape(-1)[::7])
    elif dt.kind == 'u':
        v = rng.integers(0, min(np.iinfo(dt).max, 3000) + 1, shape).astype(dt)
    else:
        v = rng.integers(-1100, 2500, shape).astype(dt)
    if dt.kind != 'f' and v.size >= 4:
        flat = v.reshape(-1)
        flat[0], flat[-1] = np.iinfo(dt).min, np.iinfo(dt).max if dt.itemsize <= 2 else 30000
    return v


def label_volume(shape, num, seed, dtype=np.uint8, absent=()):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, num + 1, shape)
    v[rng.random(shape) < 0.5] = 0
    for a in absent:
        v[v == a] = 0
    return v.astype(dtype)


SPACING = (1.5, 0.75, 2.0)          # (sx, sy, sz) of the test volumes


def as_image(view, spacing=SPACING, flip=(False, False, False), order=(0, 1, 2)):
    """An image whose reoriented view [z][y][x] is ``view``: the array axes permuted by ``order`` and flipped, the direction matrix to match - so
    the device reads it through negative strides and a non-zero base."""
    view = np.asarray(view)
    D = np.zeros((3, 3))
    # image axis (sitk) a holds view axis (x=0, y=1, z=2) order[a]; a flipped axis runs against its physical direction
    arr = np.transpose(view, [2 - order[2 - k] for k in range(3)])      # numpy axis k holds sitk axis 2 - k, which shows view axis order[2 - k]
    sp = [None] * 3
    for a in range(3):
        phys = order[a]
        D[phys, a] = -1.0 if flip[a] else 1.0
        sp[a] = spacing[phys]
        if flip[a]:
            arr = np.flip(arr, axis=2 - a)
    return nrrd.Image(np.ascontiguousarray(arr), tuple(sp), (3.0, -7.0, 11.0), tuple(float(v) for v in D.reshape(-1)), 1, {'k': 'v'}, None)
