"""End-to-end per-case latency of TS2D.predict() with five canonical sub-models (K = 18/23/24/26/26, synthetic weights) on
the reference's sample_s0616.nrrd (2 tiles x 4 mirror passes per sub-model): the counterpart of the reference's
"0.5-0.9 s per case on an RTX 4090" (README.md:43-46)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from totalsegmentator2d_amd.arch import UNetArch
from totalsegmentator2d_amd.model import HIPModel
from totalsegmentator2d_amd.tool import TS2D

def _timed(f):
    t = time.time(); f(); return time.time() - t


groups = [('cardiac', 18), ('muscles', 23), ('organs', 24), ('ribs', 26), ('vertebrae', 26)]
models = {}
for i, (g, K) in enumerate(groups):
    arch = UNetArch.canonical(num_classes=K)
    blob = (np.random.default_rng(i).standard_normal(arch.n_params()) * 0.02).astype(np.float32)
    ds = {'channel_names': {'0': 'mean', '1': 'max'}, 'labels': {'background': 0, **{f'{g}_{j+1}': j + 1 for j in range(K)}},
          'file_ending': '.nrrd', 'multilabel': True}
    models[f'ts2d-v2-ep4000b2_{g}'] = HIPModel({'model': f'ts2d-v2-ep4000b2_{g}', 'revision': 1, 'param': {},
                                               'synthetic': {'arch': arch, 'blobs': [blob], 'patch_size': (512, 512), 'dataset_json': ds}})
t0 = time.time()
with TS2D(models=models) as ts:
    print(f'startup {time.time() - t0:.2f} s', flush=True)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'assets', 'sample_s0616.nrrd')
    segs = {}
    for conc in (False, True, False, True):
        ts.concurrent_models = conc
        best = None
        for it in range(4):
            t = time.time()
            res = ts.predict(path)
            dt = time.time() - t
            stages = {}
            for m, r in res.data['models'].items():
                ts_ = r['timestamps']
                for a, b in (('start', 'preprocessed'), ('preprocessed', 'predicted'), ('predicted', 'exported')):
                    stages[b] = stages.get(b, 0) + ts_[b] - ts_[a]
            if best is None or dt < best[0]:
                best = (dt, stages)
        segs[conc] = res.get_segmentation().array.copy()
        dt, stages = best
        print(f'sub-models {"concurrent" if conc else "serial    "}: best of 4: {dt * 1e3:.1f} ms per case  (summed over sub-models: preprocess {stages["preprocessed"] * 1e3:.1f}, '
              f'predict {stages["predicted"] * 1e3:.1f}, export {stages["exported"] * 1e3:.1f} ms); segmentation {res.get_segmentation().components} labels', flush=True)
    print('masks identical (concurrent vs serial):', bool(np.array_equal(segs[True], segs[False])))
    # the same case with the file already read (zlib-inflating the 3.5 MB float64 sample is ~23 ms of host time that no engine touches)
    from totalsegmentator2d_amd import nrrd
    img = nrrd.read(path)
    for conc in (False, True):
        ts.concurrent_models = conc
        best = min(_timed(lambda: ts.predict(img)) for _ in range(5))
        print(f'image in memory, sub-models {"concurrent" if conc else "serial    "}: best of 5: {best * 1e3:.1f} ms per case', flush=True)
    # ---- several cases at once: TS2D.predict_many (one engine batch per sub-model, ts2d_engine_predict_tiled_batch) against one predict per case,
    # in-memory copies of the sample, split and 16-bit modes, alternated in one process, best of 5 after warm-up.  Stage times are host-clock
    # spans summed over the sub-models (the cases of a batch share the `predicted` stamp: the predict span of a batched case is the batch's).
    def _stages(results):
        st = {}
        for res in results:
            for r in res.data['models'].values():
                t_ = r['timestamps']
                for a, b in (('start', 'preprocessed'), ('preprocessed', 'predicted'), ('predicted', 'exported')):
                    st[b] = st.get(b, 0) + t_[b] - t_[a]
        return st

    ts.concurrent_models = True
    for mode in ('split', 'f16'):
        for m in ts.models.values():
            for e in m._predictor.engines:
                e.set_precision(mode)
                e.set_tile_dtype('half' if mode == 'f16' else 'float')
        for n in (8, 16):
            imgs = [img] * n
            many = ts.predict_many(imgs)                                   # warm-up of both paths at this size
            single = [ts.predict(img) for _ in range(n)]
            flips = np.mean([(a.get_segmentation().array != b.get_segmentation().array).mean() for a, b in zip(many, single)])
            same = all(np.array_equal(many[0].get_segmentation().array, r.get_segmentation().array) for r in many[1:])
            tb = ts_ = None
            for _ in range(5):
                t = time.time(); many = ts.predict_many(imgs); dt = time.time() - t
                if tb is None or dt < tb[0]:
                    tb = (dt, _stages(many))
                t = time.time(); single = [ts.predict(x) for x in imgs]; dt = time.time() - t
                if ts_ is None or dt < ts_[0]:
                    ts_ = (dt, _stages(single))
            for label, (dt, st) in (('predict_many', tb), ('predict x n  ', ts_)):
                print(f'{mode:5s} {n:2d} cases {label}: best of 5: {dt * 1e3:7.1f} ms = {n / dt:6.1f} cases/s  (summed over cases and sub-models: preprocess '
                      f'{st["preprocessed"] * 1e3:.1f}, predict {st["predicted"] * 1e3:.1f}, export {st["exported"] * 1e3:.1f} ms)', flush=True)
            print(f'{mode:5s} {n:2d} cases: predict_many / predict = {ts_[0] / tb[0]:.2f}x cases/s; every case of the batch identical: {same}; '
                  f'mask bits differing from predict: {flips:.2e}', flush=True)
