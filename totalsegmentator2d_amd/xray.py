"""Synthetic radiographs of a CT volume, and the matching perspective projection of a 3-D label volume.

The ``tsxr-*`` models of the reference were trained on synthetic radiographs of CT volumes; ``image.project(img, 'xr')`` refuses the mode here
as it does there, so the renderer has a module of its own and is switched on explicitly (``TS2D(synthetic_xr=...)``, ``ts2d --synthetic-xr``).
:func:`xr_tables`, :func:`synthetic_xr_statement` and :func:`project_labels_xr_statement` are the project's definition - written in numpy, they
are the host route and the oracle of the device route (C-ABI ``ts2d_project_xr``, ``ts2d_project_labels_xr``; ``csrc/kernels_project_xr.h``,
the tables in ``csrc/prep_plan.cpp``), which reproduces them bit for bit.

GEOMETRY.  The volume is taken in the reoriented view ``[z][y][x]`` of ``image._coronal_view``: extents ``(nz, ny, nx)``, spacings
``(sx, sy, sz)``, coordinates in index millimetres ``X = x sx``, ``Y = y sy``, ``Z = z sz``, centre ``C = ((nx - 1) sx / 2, (ny - 1) sy / 2,
(nz - 1) sz / 2)``.  Rays run along ``y`` as the coronal projections do, and the image keeps their handedness for both views: rows are ``v``
(along ``z``), columns ``u`` (along ``x``).  With ``g = +1`` for ``'ap'`` (source in front of the patient) and ``g = -1`` for ``'pa'`` the source
is ``S = (Cx, Cy - g sod, Cz)`` and the detector plane ``Yd = Sy + g sdd``; pixel ``(k, i)`` of the ``[nv][nu]`` image sits at
``U_i = Cx + (i - (nu - 1) / 2) du``, ``V_k = Cz + (k - (nv - 1) / 2) dv``.  ``parallel=True`` fixes ``nu = nx``, ``nv = nz``, ``du = sx``,
``dv = sz``: ray ``(k, i)`` then has constant ``x = i``, ``z = k``.

THE RADIOGRAPH is the plane-stepping form of the line integral: one bilinear sample per voxel plane ``y = j``, so every ray has exactly ``ny``
samples, added in the order ``j = 0 ... ny - 1`` for both views, in float64, every operation rounded on its own (no fused multiply-add).  The
result is the integral of the density in millimetres of water (``float32(sum * step)``); no exponential is applied.  The defaults of
:class:`XRGeometry` are the project's own: they were not matched to any other renderer's.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .nrrd import Image

XR_NONFINITE = 1                 # _lib.XR_NONFINITE: the status bit of ts2d_project_xr
MAX_PIXELS = 2 ** 31 - 1
# THE SIZE GATE.  A call of either entry costs 0.15 ... 0.21 ms however little it renders (allocation, seven small copies, the launches), the
# statements cost per plane: 30 us + 10 ns per detector pixel (radiograph), 13 us + 5 ns per pixel (labels), measured on the host of an MI355X
# (scripts/gpu_synthetic_xr_case.py, profiles/r38_synthetic_xr_case.txt; statement / device below).  The routes cross where the two meet.  At
# 80 x 6 pixels: the radiograph between 4 and 6 planes (0.94x, 1.35x), the labels between 8 and 12 (0.76 - 0.78x, 1.08 - 1.14x).  At 240 x 120
# pixels: the radiograph wins at one plane (1.58 - 1.66x), the labels between one and two (0.82 - 0.84x, 1.51 - 1.56x).  Below the crossing the
# statement is taken: ny * (3000 + pixels) < 14000, and for the labels ny * (2600 + pixels) < 34000.  From there on the device route lost
# nowhere: 5.6 - 5.9x at 66 x 37 x 5, 30 - 37x on the sample asset, 250 - 380x at 512 x 512 x 600.
_GATE = {'xr': (3000, 14000), 'labels': (2600, 34000)}


def host_is_faster(kind: str, g: dict) -> bool:
    """Is the statement the faster route for this resolved geometry (the size gate above)?  ``kind``: 'xr' or 'labels'."""
    per_plane, limit = _GATE[kind]
    return g['shape'][1] * (per_plane + g['nu'] * g['nv']) < limit


@dataclass(frozen=True)
class XRGeometry:
    """Where the source and the detector of a synthetic radiograph are, and how a sample becomes a density (the module's docstring)."""
    source_detector_mm: float = 1800.0            # sdd
    source_center_mm: float = 1500.0              # sod: source to the centre of the volume
    view: str = 'ap'                              # 'ap': source in front of the patient; 'pa': behind
    parallel: bool = False                        # parallel rays instead of a cone beam
    detector_spacing: Optional[Tuple[float, float]] = None      # (du, dv) in mm; None: (sx, sz)
    detector_size: Optional[Tuple[int, int]] = None             # (nu, nv); None: the volume's extent magnified, see resolve()
    air: float = -1000.0                          # sample value of density 0
    water: float = 0.0                            # sample value of density 1
    density_max: Optional[float] = None           # upper clip of the density; None: no clip

    def resolve(self, shape, spacing) -> dict:
        """The numbers of this geometry over a volume of extents ``shape`` = (nz, ny, nx) and spacings ``spacing`` = (sx, sy, sz): what the
        C entries take.  Raises ``ValueError``, by name, for what the module refuses."""
        nz, ny, nx = (int(v) for v in shape)
        sx, sy, sz = (float(v) for v in spacing)
        if min(nz, ny, nx) < 1:
            raise ValueError(f"synthetic_xr: extents nz {nz}, ny {ny}, nx {nx} below 1")
        view = str(self.view).lower().strip()
        if view not in ('ap', 'pa'):
            raise ValueError(f"synthetic_xr: view {self.view!r} is neither 'ap' nor 'pa'")
        sdd, sod = float(self.source_detector_mm), float(self.source_center_mm)
        parallel = bool(self.parallel)
        if parallel:
            du, dv, nu, nv = sx, sz, nx, nz
            if self.detector_spacing is not None and tuple(float(v) for v in self.detector_spacing) != (sx, sz):
                raise ValueError(f"synthetic_xr: parallel rays fix detector_spacing to (sx, sz) = {(sx, sz)}, found {tuple(self.detector_spacing)}")
            if self.detector_size is not None and tuple(int(v) for v in self.detector_size) != (nx, nz):
                raise ValueError(f"synthetic_xr: parallel rays fix detector_size to (nx, nz) = {(nx, nz)}, found {tuple(self.detector_size)}")
        else:
            du, dv = (sx, sz) if self.detector_spacing is None else (float(v) for v in self.detector_spacing)
        for name, v in (('spacing sx', sx), ('spacing sy', sy), ('spacing sz', sz), ('source_detector_mm', sdd), ('source_center_mm', sod),
                        ('detector_spacing du', du), ('detector_spacing dv', dv)):
            if not (math.isfinite(v) and v > 0):
                raise ValueError(f"synthetic_xr: {name} = {v} is not finite and positive")
        half = np.float64(ny - 1) * np.float64(sy) / np.float64(2)
        if not sod > half:
            raise ValueError(f"synthetic_xr: source_center_mm = {sod} puts the source inside the slab of plane centres (half depth {float(half)} mm)")
        if np.float64(sdd) - np.float64(sod) < half:
            raise ValueError(f"synthetic_xr: source_detector_mm - source_center_mm = {sdd - sod} puts the detector inside the slab of plane centres "
                             f"(half depth {float(half)} mm)")
        if not parallel:
            if self.detector_size is None:
                M = np.float64(sdd) / np.float64(sod)
                nu = int(np.ceil(np.float64(nx) * np.float64(sx) * M / np.float64(du)))
                nv = int(np.ceil(np.float64(nz) * np.float64(sz) * M / np.float64(dv)))
            else:
                nu, nv = (int(v) for v in self.detector_size)
        if nu < 1 or nv < 1:
            raise ValueError(f"synthetic_xr: detector_size nu {nu}, nv {nv} below 1")
        if nu * nv > MAX_PIXELS:
            raise ValueError(f"synthetic_xr: detector_size nu {nu} x nv {nv} is more than 2^31 - 1 pixels")
        air, water = float(self.air), float(self.water)
        if not (math.isfinite(air) and math.isfinite(water)):
            raise ValueError(f"synthetic_xr: air = {air}, water = {water} are not finite")
        if water == air:
            raise ValueError(f"synthetic_xr: water == air = {air}: no sample value has density 1")
        dmax = None if self.density_max is None else float(self.density_max)
        if dmax is not None and not dmax >= 0:
            raise ValueError(f"synthetic_xr: density_max = {dmax} is not a number >= 0")
        return {'shape': (nz, ny, nx), 'spacing': (sx, sy, sz), 'sdd': sdd, 'sod': sod, 'pa': int(view == 'pa'), 'parallel': int(parallel),
                'du': du, 'dv': dv, 'nu': nu, 'nv': nv, 'air': air, 'water': water, 'density_max': dmax}


def _geometry(geometry) -> XRGeometry:
    if geometry is None or geometry is True:
        return XRGeometry()
    if not isinstance(geometry, XRGeometry):
        raise TypeError(f"synthetic_xr: geometry is an XRGeometry, True or None, found {type(geometry).__name__}")
    return geometry


def xr_tables(shape, spacing, geometry=None) -> dict:
    """The float64 tables of the rays, every operation rounded on its own.  With ``den = Yd - Sy``:

    ``t[j] = (j sy - Sy) / den`` for ``j = 0 ... ny - 1`` (in ``(0, 1]``), ``a[i] = (U_i - Cx) / sx``, ``b[k] = (V_k - Cz) / sz``,
    ``cx[i] = Cx / sx``, ``cz[k] = Cz / sz`` (the same number in every entry), and the step length of ray ``(k, i)``
    ``step[k][i] = sy * sqrt((1 + p_i p_i) + q_k q_k)`` with ``p_i = (U_i - Cx) / den``, ``q_k = (V_k - Cz) / den``.
    Parallel rays: ``t = 0``, ``cx[i] = i``, ``cz[k] = k``, ``step = sy``.  Sample ``j`` of ray ``(k, i)`` lies at ``x = cx[i] + t[j] * a[i]``,
    ``z = cz[k] + t[j] * b[k]``.  Also ``u0`` / ``v0`` (``U_0``, ``V_0``) and the resolved numbers under ``'geometry'``."""
    g = _geometry(geometry).resolve(shape, spacing)
    f = np.float64
    nz, ny, nx = g['shape']
    sx, sy, sz = (f(v) for v in g['spacing'])
    nu, nv, du, dv = g['nu'], g['nv'], f(g['du']), f(g['dv'])
    Cx, Cy, Cz = f(nx - 1) * sx / f(2), f(ny - 1) * sy / f(2), f(nz - 1) * sz / f(2)
    sign = f(-1.0 if g['pa'] else 1.0)
    Sy = Cy - sign * f(g['sod'])
    Yd = Sy + sign * f(g['sdd'])
    den = Yd - Sy
    U = Cx + (np.arange(nu, dtype=f) - f(nu - 1) / f(2)) * du
    V = Cz + (np.arange(nv, dtype=f) - f(nv - 1) / f(2)) * dv
    a, b = (U - Cx) / sx, (V - Cz) / sz
    if g['parallel']:
        t = np.zeros(ny, f)
        cx, cz = np.arange(nu, dtype=f), np.arange(nv, dtype=f)
        step = np.full((nv, nu), sy, f)
    else:
        t = (np.arange(ny, dtype=f) * sy - Sy) / den
        cx, cz = np.full(nu, Cx / sx, f), np.full(nv, Cz / sz, f)
        p, q = (U - Cx) / den, (V - Cz) / den
        step = sy * np.sqrt((f(1) + p * p)[None, :] + (q * q)[:, None])
    return {'t': t, 'a': a, 'b': b, 'cx': cx, 'cz': cz, 'step': step, 'u0': float(U[0]), 'v0': float(V[0]), 'geometry': g}


def _density(plane: np.ndarray, g: dict) -> np.ndarray:
    """``max((float64(v) - air) * scale, 0)`` with ``scale = 1 / (water - air)`` computed once (a zero is ``+0.0``), then the upper clip."""
    scale = np.float64(1) / (np.float64(g['water']) - np.float64(g['air']))
    d = (plane.astype(np.float64) - np.float64(g['air'])) * scale
    d = np.where(d > 0, d, np.float64(0))
    if g['density_max'] is not None:
        d = np.where(d > np.float64(g['density_max']), np.float64(g['density_max']), d)
    return d


def synthetic_xr_statement(volume_view: np.ndarray, tables: dict, geometry=None) -> np.ndarray:
    """The float64 sums ``[nv][nu]`` of the radiograph of ``volume_view`` ``[nz][ny][nx]`` (the radiograph is ``float32(sum * tables['step'])``).

    For ``j = 0 ... ny - 1`` in that order: ``x = cx + t[j] * a``, ``z = cz + t[j] * b``, ``x0 = floor(x)``, ``fx = x - x0`` (likewise z),
    ``r0 = d[z0][x0] * (1 - fx) + d[z0][x0 + 1] * fx``, ``r1`` the same on row ``z0 + 1``, ``acc += r0 * (1 - fz) + r1 * fz``, where ``d`` is
    the density of plane ``j`` and ``+0.0`` outside it.  A sample with ``x`` outside ``(-1, nx)`` or ``z`` outside ``(-1, nz)`` adds nothing.
    ``geometry`` is not read again: the tables carry its resolved numbers.  A float volume with a non-finite sample raises ``ValueError``."""
    v = np.asarray(volume_view)
    g = tables['geometry']
    if v.ndim != 3 or tuple(v.shape) != tuple(g['shape']):
        raise ValueError(f"synthetic_xr: the view has shape {tuple(v.shape)}, the tables were made for {tuple(g['shape'])}")
    if np.issubdtype(v.dtype, np.floating) and not np.isfinite(v).all():
        raise ValueError("synthetic_xr: the volume holds a non-finite sample")
    nz, ny, nx = g['shape']
    t, a, b, cx, cz = (tables[k] for k in ('t', 'a', 'b', 'cx', 'cz'))
    acc = np.zeros((g['nv'], g['nu']), np.float64)
    pad = np.zeros((nz + 2, nx + 2), np.float64)                      # the plane's density inside a frame of +0.0
    with np.errstate(all='ignore'):
        for j in range(ny):
            x, z = cx + t[j] * a, cz + t[j] * b
            ix, kz = np.nonzero((x > -1) & (x < nx))[0], np.nonzero((z > -1) & (z < nz))[0]
            if not (ix.size and kz.size):
                continue
            x0, z0 = np.floor(x[ix]), np.floor(z[kz])
            fx, fz = x[ix] - x0, (z[kz] - z0)[:, None]
            xi, zi = x0.astype(np.intp) + 1, z0.astype(np.intp) + 1
            pad[1:-1, 1:-1] = _density(v[:, j, :], g)
            row0, row1 = pad[zi], pad[zi + 1]
            gx = np.float64(1) - fx
            r0 = row0[:, xi] * gx + row0[:, xi + 1] * fx
            r1 = row1[:, xi] * gx + row1[:, xi + 1] * fx
            acc[np.ix_(kz, ix)] += r0 * (np.float64(1) - fz) + r1 * fz
    return acc


def project_labels_xr_statement(label_view: np.ndarray, num: int, tables: dict) -> np.ndarray:
    """The perspective companion of ``evaluate.project_labels``: uint8 planes ``[num][nv][nu]``, plane ``L - 1`` is 1 where any sample of the ray
    has value ``L``.  The rays and the ``j`` loop are the radiograph's; the sample is the nearest voxel ``xi = floor(x + 0.5)``,
    ``zi = floor(z + 0.5)`` (the sum rounded first), and a sample outside the volume is skipped.  A volume sample outside ``0 ... num`` raises
    the ``ValueError`` of ``project_labels``; ``num`` runs from 1 to 255; a float volume raises."""
    from .evaluate import _check_num
    v = np.asarray(label_view)
    g = tables['geometry']
    num = _check_num(num)
    if v.ndim != 3 or tuple(v.shape) != tuple(g['shape']):
        raise ValueError(f"project_labels_xr: the view has shape {tuple(v.shape)}, the tables were made for {tuple(g['shape'])}")
    if not np.issubdtype(v.dtype, np.integer):
        raise ValueError(f"project_labels: a label volume has an integer type, found {v.dtype}")
    if v.size and (int(v.min()) < 0 or int(v.max()) > num):
        raise ValueError(f"project_labels: the volume holds samples outside 0 ... {num} (minimum {int(v.min())}, maximum {int(v.max())})")
    nz, ny, nx = g['shape']
    t, a, b, cx, cz = (tables[k] for k in ('t', 'a', 'b', 'cx', 'cz'))
    planes = np.zeros((num, g['nv'], g['nu']), np.uint8)
    with np.errstate(all='ignore'):
        for j in range(ny):
            x, z = (cx + t[j] * a) + np.float64(0.5), (cz + t[j] * b) + np.float64(0.5)
            ix, kz = np.nonzero((x >= 0) & (x < nx))[0], np.nonzero((z >= 0) & (z < nz))[0]
            if not (ix.size and kz.size):
                continue
            vals = v[:, j, :][np.ix_(np.floor(z[kz]).astype(np.intp), np.floor(x[ix]).astype(np.intp))].astype(np.intp)
            kk, ii = np.nonzero(vals)
            planes[vals[kk, ii] - 1, kz[kk], ix[ii]] = 1
    return planes


# ------------------------------------------------------------------------------------------------------------------ images
def _view(img: Image):
    """The reoriented view [z][y][x] of a scalar 3-D image (no copy of the voxels beyond ``ascontiguousarray``), its spacings (sx, sy, sz) and
    the reoriented origin and direction: what ``image._coronal_view`` hands the device, as an array."""
    from .image import _reorient_plan, _reoriented_geometry
    if img.dimension != 3 or img.components != 1:
        raise ValueError(f"synthetic_xr: a scalar 3-D volume is needed, found {img.components} components in {img.dimension}-D")
    perm, flips = _reorient_plan(img)
    view = np.transpose(np.ascontiguousarray(img.array), [2 - perm[2 - k] for k in range(3)])
    for k in range(3):
        if flips[k]:
            view = np.flip(view, axis=2 - k)
    origin, direction = _reoriented_geometry(img, perm, flips)
    return view, tuple(float(img.spacing[ax]) for ax in perm), origin, direction


def _detector_grid(tables: dict, spacing, origin, direction):
    """Spacing and origin of the detector image: (du, sy, dv), the reoriented origin moved by U_0 along the first direction column and by V_0
    along the third."""
    g = tables['geometry']
    D = np.asarray(direction, np.float64).reshape(3, 3)
    o = np.asarray(origin, np.float64) + D[:, 0] * tables['u0'] + D[:, 2] * tables['v0']
    return (g['du'], spacing[1], g['dv']), tuple(float(v) for v in o)


def device_renders(img: Image) -> bool:
    """Does ``ts2d_project_xr`` serve the volume?  A scalar 3-D volume of a sample type of the device projection, and a library with the symbol."""
    from . import engine
    from .image import _GPU_DTYPES
    return img.dimension == 3 and img.components == 1 and img.array.dtype.name in _GPU_DTYPES and engine.has_entry('ts2d_project_xr')


def device_projects_labels(img: Image) -> bool:
    """... and ``ts2d_project_labels_xr`` a label volume?  As above, of an integer type."""
    from . import engine
    from .image import _GPU_DTYPES
    return (img.dimension == 3 and img.components == 1 and img.array.dtype.name in _GPU_DTYPES and np.issubdtype(img.array.dtype, np.integer)
            and engine.has_entry('ts2d_project_labels_xr'))


def synthetic_xr(img: Image, geometry=None, device: Optional[int] = None) -> Image:
    """The synthetic radiograph of a CT volume: a float32 image of size ``(nu, 1, nv)`` on the detector's grid, in millimetres of water.
    ``device=None`` is the host route (the statements); with a device the entry ``ts2d_project_xr`` renders where the library has it, the
    sample type is served and the volume is past the size gate (:func:`host_is_faster`) - the bits are the same.  A non-finite sample raises ``ValueError`` on both routes."""
    from . import _lib, engine
    from .image import _coronal_view
    geometry = _geometry(geometry)
    view, spacing, origin, direction = _view(img)
    tables = xr_tables(view.shape, spacing, geometry)
    g = tables['geometry']
    if device is not None and not host_is_faster('xr', g) and device_renders(img):
        a, extents, strides, base, _, _ = _coronal_view(img)
        _, xr, status = engine.project_xr(a, extents, strides, base, g, device, want_sum=False)
        if status & _lib.XR_NONFINITE:
            raise ValueError("synthetic_xr: the volume holds a non-finite sample")
    else:
        xr = (synthetic_xr_statement(view, tables) * tables['step']).astype(np.float32)
    sp, o = _detector_grid(tables, spacing, origin, direction)
    return Image(np.ascontiguousarray(xr).reshape(g['nv'], 1, g['nu']), sp, o, direction, 1, dict(img.meta), img.space)


def project_labels_xr(img: Image, num: int, geometry=None, device: Optional[int] = None) -> Image:
    """The label projection of a 3-D label volume along the rays of :func:`synthetic_xr`, in the layout ``evaluate.project_labels`` returns, on
    the radiograph's grid.  ``device`` as in :func:`synthetic_xr` (C-ABI ``ts2d_project_labels_xr``)."""
    from . import _lib, engine
    from .evaluate import _check_num, _planes_image
    from .image import _coronal_view
    num = _check_num(num)
    geometry = _geometry(geometry)
    view, spacing, origin, direction = _view(img)
    tables = xr_tables(view.shape, spacing, geometry)
    g = tables['geometry']
    if device is not None and not host_is_faster('labels', g) and device_projects_labels(img):
        a, extents, strides, base, _, _ = _coronal_view(img)
        planes, status = engine.project_labels_xr(a, extents, strides, base, num, g, device)
        if status & _lib.LABELS_RANGE:
            raise ValueError(f"project_labels: the volume holds samples outside 0 ... {num}")
    else:
        planes = project_labels_xr_statement(view, num, tables)
    sp, o = _detector_grid(tables, spacing, origin, direction)
    return _planes_image(planes.reshape(num, g['nv'], 1, g['nu']), img, sp, o, direction)
