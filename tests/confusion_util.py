"""TEST INFRASTRUCTURE (never imported by the product) of tests/test_confusion_cpu.py and tests/test_gpu_confusion.py: random sides of both kinds
and the confusion matrix from first principles."""
import numpy as np

from totalsegmentator2d_amd import evaluate as E

PAIRINGS = [(E.PLANES, E.PLANES), (E.PLANES, E.LABELMAP), (E.LABELMAP, E.PLANES), (E.LABELMAP, E.LABELMAP)]
PLANE_BYTES = np.array([1, 127, 128, 255], np.uint8)          # a plane byte of 128 ... 255 would be a negative i8 if it reached the product raw


def stray_byte(values):
    """a byte that is neither 0 nor one of the values (a label map may hold such samples: they belong to no label); None where 255 values leave none"""
    return next((w for w in (3, 200, 255, 254, 77) + tuple(range(1, 256)) if w not in values), None)


def random_side(rng, kind, K, spatial, values, absent=(), stray=True, present=False):
    """One side with UNEQUAL label frequencies (every draw has its own): planes [K, *spatial] that overlap, their bytes 0, 1, 127, 128, 255; or a
    label map over `values` with - `stray` - bytes that are not among them.  The labels `absent` have no sample; `present`: every other label has
    at least one (where the samples suffice)."""
    spatial = tuple(spatial)
    n = int(np.prod(spatial))
    live = [k for k in range(K) if k not in absent]
    if kind == E.PLANES:
        x = (rng.random((K, n)) < rng.uniform(0.05, 0.5, (K, 1))).astype(np.uint8)
        if present:
            x[np.arange(K), rng.integers(0, n, K)] = 1
        x *= rng.choice(PLANE_BYTES, x.shape)
        x[list(absent)] = 0
        return x.reshape((K,) + spatial)
    pool = np.array([0] + [values[k] for k in live] + ([stray_byte(values)] if stray and stray_byte(values) is not None else []), np.uint8)
    weights = rng.uniform(0.2, 1.0, len(pool)) ** 3
    x = rng.choice(pool, n, p=weights / weights.sum())
    if present:
        at = rng.permutation(n)[:len(live)]
        x[at] = [values[k] for k in live][:len(at)]
    return x.reshape(spatial)


def plain_loop(a, kind_a, b, kind_b, values, K):
    """the matrix from first principles: every pair of rows by count_nonzero, the rows written out here and not taken from the module"""
    def rows(x, kind):
        m = [(x[k] != 0) if kind == E.PLANES else (x == values[k]) for k in range(K)]
        none = np.ones(m[0].shape, bool)
        for r in m:
            none &= ~r
        return [none] + m + [np.ones(m[0].shape, bool)]
    ra, rb = rows(a, kind_a), rows(b, kind_b)
    return np.array([[np.count_nonzero(x & y) for y in rb] for x in ra], np.int64)
