"""What the tests of the label morphology (tests/test_morphology_cpu.py, tests/test_gpu_morphology.py) share: a restatement of
``morphology.label_morphology_statement`` that is independent of its scan form - ``scipy.ndimage.binary_dilation`` / ``binary_erosion`` with the
disc built explicitly from the definition, and the label rules spelled out - and the inputs."""
import numpy as np
from scipy import ndimage

OPS = ('dilate', 'erode', 'open', 'close')
SPACINGS = (0.5, 0.7, 0.8, 1.0, 1.3, 2.5)


def explicit_disc(r, sy, sx, H, W):
    """Every offset two pixels of an H x W image can have, inside iff (|dy| sy)^2 + (|dx| sx)^2 <= r r: float64, each operation on its own."""
    r2 = np.float64(r) * np.float64(r)
    B = np.zeros((2 * H - 1, 2 * W - 1), bool)
    for dy in range(-(H - 1), H):
        for dx in range(-(W - 1), W):
            ry = np.float64(abs(dy)) * np.float64(sy)
            rx = np.float64(abs(dx)) * np.float64(sx)
            B[dy + H - 1, dx + W - 1] = ry * ry + rx * rx <= r2
    return B


def scipy_op(mask, op, B):
    """op of a boolean mask with structure B; the erosion ignores what is outside the image (border_value=1)."""
    def dil(m):
        return ndimage.binary_dilation(m, structure=B)

    def ero(m):
        return ndimage.binary_erosion(m, structure=B, border_value=1)
    return {'dilate': dil, 'erode': ero, 'open': lambda m: dil(ero(m)), 'close': lambda m: ero(dil(m))}[op](mask)


def restatement(seg, values, op, r, spacing_hw, select=None):
    """(out, counters) by the rules of the module docstring of morphology.py, on top of scipy_op."""
    planes = values is None
    K = seg.shape[0] if planes else len(values)
    H, W = seg.shape[-2:]
    B = explicit_disc(r, spacing_hw[0], spacing_hw[1], H, W)
    select = [True] * K if select is None else list(select)
    out = seg.copy()
    for k in range(K):
        if not select[k]:
            continue
        if planes:
            m = seg[k] > 0
            res = scipy_op(m, op, B)
            out[k][res & ~m] = 1
            out[k][~res] = 0
        else:
            m = seg == values[k]
            res = scipy_op(m, op, B)
            if op in ('dilate', 'close'):
                out[res & (out == 0)] = values[k]
            else:
                out[m & ~res] = 0
    counters = np.zeros((K, 4), np.int64)
    for k in range(K):
        a = seg[k] > 0 if planes else seg == values[k]
        b = out[k] > 0 if planes else out == values[k]
        counters[k] = (a.sum(), b.sum(), (b & ~a).sum(), (a & ~b).sum())
    return out, counters


def random_masks(n, seed, max_h=23, max_w=79):
    """n of (mask, r, sy, sx): 1 ... max_h x 1 ... max_w pixels, empty, sparse, dense and full, radii from 0 to far beyond the image."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        H, W = int(rng.integers(1, max_h + 1)), int(rng.integers(1, max_w + 1))
        sy, sx = (float(v) for v in rng.choice(SPACINGS, 2))
        r = float(rng.choice([0.0, 0.45, 0.8, 1.0, 1.5, 2.0, 2.5, 3.3, 5.0, 10.0, 1000.0]))
        density = (0.0, 0.02, 0.3, 0.9, 1.0)[i % 5]
        out.append((rng.random((H, W)) < density, r, sy, sx))
    return out


def same(a, b):
    """Two (out, counters) pairs are the same bytes."""
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def speckle_planes(rng, K, H, W, density):
    """uint8 planes [K, H, W] with bytes other than 1 where set."""
    return ((rng.random((K, H, W)) < density) * rng.integers(1, 256, (K, H, W))).astype(np.uint8)


def speckle_map(rng, values, H, W, density, others=()):
    """A label map over `values` and the unnamed non-zero values `others`, background with probability 1 - density."""
    pool = np.asarray(list(values) + list(others), np.uint8)
    return ((rng.random((H, W)) < density) * pool[rng.integers(0, len(pool), (H, W))]).astype(np.uint8)
