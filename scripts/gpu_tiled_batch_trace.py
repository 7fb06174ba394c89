"""One batched sliding-window call beside the per-case calls it replaces, for a kernel trace: the canonical K = 26 net, 8 copies of the
preprocessed extent of sample_s0616 (644 x 512 padded, 2 tiles x 4 mirror passes each = 64 rows).
    rocprofv3 --kernel-trace --memory-copy-trace --stats -d OUT -- python scripts/gpu_tiled_batch_trace.py
In the trace, per round (two rounds, the second one warm): sw_gather / sw_aggregate run 9 times each - 8 launches over one image
(ts2d_engine_predict_tiled, one segment) and then one launch over all 8 (ts2d_engine_predict_tiled_batch, 8 segments).  Bytes the pair moves for these 8 cases (computed from the shapes, printed below): gather reads and writes
rows x C x ph x pw floats; aggregate reads rows x K x ph x pw floats and writes K x Hp x Wp halves + bytes per case."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from totalsegmentator2d_amd import prng, weights
from totalsegmentator2d_amd import sliding_window as sw
from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.engine import Engine

arch = UNetArch.canonical(num_classes=26)
blob = (np.random.default_rng(0).standard_normal(arch.n_params()) * 0.02).astype(np.float32)
patch, n = (512, 512), 8
img = prng.normal_f32(1, 999, (2, 644, 512))
tiles = [(y, x) for (_, y, x) in sw.tile_slicers((644, 512), patch, 0.5, 1)]
g = sw.compute_gaussian(patch)
rows, K, C = n * len(tiles) * 4, 26, 2
print(f'gather: {2 * rows * C * 512 * 512 * 4 / 1e6:.1f} MB; aggregate: {(rows * K * 512 * 512 * 4 + n * K * 644 * 512 * 3) / 1e6:.1f} MB for {n} cases ({rows} rows)')
with Engine(arch, blob) as e:
    for _ in range(2):                       # (the first round loads code objects and sizes the scratch)
        for _i in range(n):
            e.predict_tiled(img, patch, tiles, (0, 1), g, want_logits=True, want_seg=True)
        e.predict_tiled_batch([img] * n, patch, [tiles] * n, (0, 1), g, want_logits=True, want_seg=True)
