"""Randomised check of the packing and the dispatch of the batched sliding window (ts2d_engine_predict_tiled_batch: segment table with
several images per launch, row packing into chunks, per-image inf flag, full-batch dispatch) against ts2d_engine_predict_tiled on an engine
with 'sbk': 0, image by image, bit for bit.  Both entries run the same kernel pair and host code (a single image is a batch of one), so this
does not check the aggregation arithmetic - scripts/gpu_fuzz_sliding_window.py does, against the host restatement.  Each case
draws one network, patch, step, mirror axes and tile dtype and 1 ... 9 images of mixed extents (smaller and larger than the patch, pitches
that are and are not multiples of 4) that travel in ONE call on an engine with default options.
    python scripts/gpu_fuzz_tiled_batch.py SEED N"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cases
from totalsegmentator2d_amd import weights, prng
from totalsegmentator2d_amd import sliding_window as sw
from totalsegmentator2d_amd.engine import Engine

rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
for t in range(n):
    ns = int(rng.integers(2, 4))
    feats = [32] + [int(rng.choice([32, 64])) for _ in range(ns - 1)]
    arch = cases.unet(ns, feats, int(rng.integers(1, 9)), cin=int(rng.integers(1, 3)), nconv=1)
    dy, dx = arch.divisors
    patch = (dy * int(rng.integers(max(1, 16 // dy), 96 // dy + 1)), 32 * int(rng.integers(1, 4)))
    step = float(rng.choice([0.3, 0.5, 0.75, 1.0]))
    mirror = [None, (0,), (1,), (0, 1)][int(rng.integers(0, 4))]
    order = ['float', 'half'][int(rng.integers(0, 2))]
    gauss = sw.compute_gaussian(patch) if rng.random() < 0.8 else None
    images, tiles = [], []
    for i in range(int(rng.integers(1, 10))):
        shape = (int(rng.integers(5, 4 * patch[0])), int(rng.integers(5, 3 * patch[1])))
        padded, _ = sw.pad_nd_image(prng.normal_f32(2000 + t, i, (arch.input_channels, 1) + shape), patch)
        images.append(np.ascontiguousarray(padded[:, 0]))
        tiles.append([(y, x) for (_, y, x) in sw.tile_slicers(padded.shape[2:], patch, step, 1)])
    blob = weights.pack_blob(arch, weights.synthetic_state_dict(arch, 900 + 7 * t))
    with Engine(arch, blob, options={'sbk': 0}) as old, Engine(arch, blob) as new:
        old.set_tile_dtype(order); new.set_tile_dtype(order)
        b16, bseg = new.predict_tiled_batch(images, patch, tiles, mirror, gauss, want_logits=True, want_seg=True)
        same = True
        for i, (img, tl) in enumerate(zip(images, tiles)):
            a16, aseg = old.predict_tiled(img, patch, tl, mirror, gauss, want_logits=True, want_seg=True)
            same = same and np.array_equal(a16.view(np.uint16), b16[i].view(np.uint16)) and np.array_equal(aseg, bseg[i])
    rows = [len(tl) * (1 if mirror is None else 2 ** len(mirror)) for tl in tiles]
    print(f'{t:3d} stages={ns} feats={feats} K={arch.num_classes} cin={arch.input_channels} patch={patch} step={step} mirror={mirror} tile={order} '
          f'gauss={gauss is not None} images={[im.shape[1:] for im in images]} rows={rows}: {"identical" if same else "DIFFERENT"}', flush=True)
    assert same
print('all identical')
