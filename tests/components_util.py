"""What the tests of the components (tests/test_components_cpu.py, tests/test_gpu_components.py) share: inputs, and two restatements of
``components.label_components_statement`` that are independent of it - a per-label loop of ``scipy.ndimage.label`` with the structure spelled
out, and a plain flood fill."""
from collections import deque

import numpy as np
from scipy import ndimage

STRUCTURES = {('full', 2): np.ones((3, 3), bool), ('faces', 2): np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool),
              ('full', 3): np.ones((3, 3, 3), bool),
              ('faces', 3): np.array([[[0, 0, 0], [0, 1, 0], [0, 0, 0]], [[0, 1, 0], [1, 1, 1], [0, 1, 0]], [[0, 0, 0], [0, 1, 0], [0, 0, 0]]], bool)}


def masks_of(seg, values):
    return [seg[k] > 0 for k in range(seg.shape[0])] if values is None else [seg == v for v in values]


def _finish(seg, values, pieces, keep_largest, min_voxels):
    """pieces: per label a list of sorted flat-index arrays.  -> (cleaned, counters, components) by the rule, spelled out."""
    out = seg.copy()
    counters, rows = [], []
    for k, comps in enumerate(pieces):
        sizes = [len(c) for c in comps]
        largest = max(sizes, default=0)
        gone_v = gone_c = 0
        target = out[k] if values is None else out
        flat = target.reshape(-1)
        assert np.shares_memory(flat, out)          # a view: writes reach `out`
        for c, s in zip(comps, sizes):
            rows.append((k, int(c[0]), s))
            if (keep_largest and s < largest) or (min_voxels is not None and s < min_voxels[k]):
                flat[c] = 0
                gone_v += s
                gone_c += 1
        counters.append((sum(sizes), len(comps), largest, gone_v, gone_c))
    rows.sort(key=lambda r: (r[0], -r[2], r[1]))
    return out, np.asarray(counters, np.int64).reshape(-1, 5), np.asarray(rows, np.int64).reshape(-1, 3)


def scipy_restatement(seg, values=None, connectivity='full', keep_largest=False, min_voxels=None):
    pieces = []
    for mask in masks_of(seg, values):
        lab, n = ndimage.label(mask, structure=STRUCTURES[connectivity, mask.ndim])
        flat = lab.reshape(-1)
        pieces.append([np.flatnonzero(flat == c) for c in range(1, n + 1)])
    return _finish(seg, values, pieces, keep_largest, min_voxels)


def flood_restatement(seg, values=None, connectivity='full', keep_largest=False, min_voxels=None):
    pieces = []
    for mask in masks_of(seg, values):
        shape = mask.shape
        offs = [o for o in np.ndindex(*(3,) * mask.ndim) if any(v != 1 for v in o)]
        offs = [tuple(v - 1 for v in o) for o in offs]
        if connectivity == 'faces':
            offs = [o for o in offs if sum(abs(v) for v in o) == 1]
        seen = np.zeros(shape, bool)
        comps = []
        for start in zip(*np.nonzero(mask)):
            if seen[start]:
                continue
            seen[start] = True
            queue, comp = deque([start]), []
            while queue:
                p = queue.popleft()
                comp.append(int(np.ravel_multi_index(p, shape)))
                for o in offs:
                    q = tuple(a + b for a, b in zip(p, o))
                    if all(0 <= v < s for v, s in zip(q, shape)) and mask[q] and not seen[q]:
                        seen[q] = True
                        queue.append(q)
            comps.append(np.sort(np.asarray(comp, np.int64)))
        pieces.append(comps)
    return _finish(seg, values, pieces, keep_largest, min_voxels)


def same(a, b):
    """Two (cleaned, counters, components) triples are the same bytes."""
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def random_case(rng, kind, spatial, K, density, values=None):
    """(seg, values): planes [K, *spatial] with values in {0, 1, 200}, or a label map of K values that are not 1 ... K, plus a stray value no label has."""
    if kind == 'planes':
        return ((rng.random((K,) + tuple(spatial)) < density) * rng.choice([1, 200], (K,) + tuple(spatial))).astype(np.uint8), None
    values = list(values) if values is not None else [int(v) for v in rng.choice(np.arange(2, 255), K, replace=False)]
    stray = next(v for v in range(1, 256) if v not in values)
    pick = np.asarray([0] + values + [stray], np.uint8)
    seg = np.where(rng.random(spatial) < density, pick[rng.integers(1, len(pick), spatial)], 0).astype(np.uint8)
    return seg, values


def serpentine(Z, H, W):
    """A one-voxel corridor that walks every second column of every second slice up and down; one voxel in the slices between joins them."""
    v = np.zeros((Z, H, W), np.uint8)
    for z in range(0, Z, 2):
        v[z, :, 0::2] = 1
        for x in range(1, W, 2):
            if x + 1 < W:
                v[z, H - 1 if (x // 2) % 2 == 0 else 0, x] = 1
        if z + 1 < Z:
            v[z + 1, 0, 0] = 1
    return v


def checkerboard(spatial, values):
    """Label (z + y + x) % len(values) everywhere: under 'full' every label is one piece (extents of at least 2 ... ), under 'faces' every voxel is one."""
    idx = np.indices(spatial).sum(axis=0) % len(values)
    return np.asarray(values, np.uint8)[idx]


def rings(spatial, values):
    """Concentric square rings around the centre of the last two axes, labels alternating."""
    H, W = spatial[-2:]
    y, x = np.indices((H, W))
    r = np.maximum(np.abs(y - H // 2), np.abs(x - W // 2)) % len(values)
    return np.broadcast_to(np.asarray(values, np.uint8)[r], spatial).copy()
