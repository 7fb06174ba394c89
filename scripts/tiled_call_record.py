"""Call record of the sliding-window Python layer (engine.py, predictor.py) against a STUB of the C library: what each public method
hands to which C entry, in a pointer-free form, plus what it returns and what it raises.  No GPU and no built library needed.

    python scripts/tiled_call_record.py OUT.json [--signatures SIG.json]

The record of two commits is compared byte for byte (``cmp a.json b.json``): a refactor of the marshalling must leave it identical.  The
stub answers 0 to every ``ts2d_*`` call, fills every output it is handed with a pattern that depends on the call's ordinal (so that the
arrays a method returns are provably the ones it passed) and sets the inf flags to a fixed pattern when ``inf`` is on: image 1 of a call
with 3 images, fold 1 of an ensemble, every third flat call.  ``--signatures`` (needs the built library) also dumps restype / argtypes of
every symbol of the loaded library."""
import ctypes
import hashlib
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from totalsegmentator2d_amd import _lib
from totalsegmentator2d_amd.arch import UNetArch

REAL_LOAD = _lib.load


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def at(ptr, dtype, n):
    """n elements of dtype at a raw address, as a numpy view (None for a null pointer)."""
    if not ptr:
        return None
    buf = (ctypes.c_byte * (n * np.dtype(dtype).itemsize)).from_address(int(ptr))
    return np.frombuffer(buf, dtype=dtype, count=n)


def addr(p):
    if p is None:
        return 0
    if isinstance(p, int):
        return p
    if isinstance(p, ctypes.c_void_p):
        return p.value or 0
    return ctypes.cast(p, ctypes.c_void_p).value or 0


class Stub:
    """Stands in for the ctypes library object: every ts2d_* attribute is a recording function."""
    RECORDED = ('ts2d_engine_predict_tiled', 'ts2d_engine_predict_tiled_batch', 'ts2d_engine_predict_tiled_export',
                'ts2d_ensemble_predict_tiled_export', 'ts2d_engine_tiled_inf_flag')

    def __init__(self):
        self.calls, self.k_of, self.flag_of = [], {}, {}
        self.inf, self.ordinal, self.flat = False, 0, 0

    def reset(self, inf):
        self.calls, self.inf, self.ordinal, self.flat = [], inf, 0, 0
        self.flag_of = {h: 0 for h in self.flag_of}

    def __getattr__(self, name):
        if not name.startswith('ts2d_'):
            raise AttributeError(name)
        return lambda *a: self._call(name, a)

    # ------------------------------------------------------------------ outputs and descriptors
    def _fill(self, ptr, dtype, n):
        v = at(ptr, dtype, n)
        if v is None:
            return None
        pat = (np.arange(n, dtype=np.int64) * 7 + 13 * self.ordinal) % 251
        v[:] = (pat % 2).astype(dtype) if np.dtype(dtype) == np.uint8 else ((pat - 125) / 8.0).astype(dtype)
        return n

    def _image(self, K, C, image, Hp, Wp, n_tiles, ty, tx, l16, seg):
        px = at(image, np.float32, C * Hp * Wp)
        return {'image': None if px is None else {'shape': [C, Hp, Wp], 'dtype': 'float32', 'sha': sha(px)}, 'Hp': Hp, 'Wp': Wp,
                'n_tiles': n_tiles, 'tile_y': None if not ty else at(ty, np.int32, n_tiles).tolist(),
                'tile_x': None if not tx else at(tx, np.int32, n_tiles).tolist(),
                'logits_f16': self._fill(l16, np.float16, K * Hp * Wp), 'seg_u8': self._fill(seg, np.uint8, K * Hp * Wp)}

    def _descs(self, K, C, desc, exd, n):
        out = []
        for i in range(n):
            d = desc[i]
            r = self._image(K, C, d.image, d.Hp, d.Wp, d.n_tiles, d.tile_y, d.tile_x, d.logits_f16, d.seg_u8)
            d.inf_flag = int(self.inf and n == 3 and i == 1)
            if exd is not None:
                x = exd[i]
                m = K * max(x.out_h, 0) * max(x.out_w, 0)
                r['export'] = {'rect': [x.src_y, x.src_x, x.src_h, x.src_w, x.out_h, x.out_w], 'seg_u8': self._fill(x.seg_u8, np.uint8, m),
                               'logits_f32': self._fill(x.logits_f32, np.float32, m)}
            out.append(r)
        return out

    def _gauss(self, g, ph, pw):
        return None if not addr(g) else sha(at(addr(g), np.float16, ph * pw))

    # ------------------------------------------------------------------ the entries
    def _call(self, name, a):
        if name == 'ts2d_abi_version':
            return _lib.ABI_VERSION
        if name == 'ts2d_last_error':
            return b'stub'
        if name == 'ts2d_engine_create':
            d, out = a[0]._obj, a[4]._obj
            out.value = 1000 + len(self.k_of)
            self.k_of[out.value] = (int(d.num_classes), int(d.input_channels))
            self.flag_of[out.value] = 0
            return 0
        if name not in self.RECORDED:
            return 0
        self.ordinal += 1
        if name == 'ts2d_engine_tiled_inf_flag':
            h = addr(a[0])
            self.calls.append({'entry': name, 'engine': h - 1000})
            return self.flag_of[h]
        if name == 'ts2d_engine_predict_tiled':
            h, image, Hp, Wp, ph, pw, n_tiles, ty, tx, mask, g, l16, seg = a
            h = addr(h)
            K, C = self.k_of[h]
            self.flag_of[h] = int(self.inf and self.flat % 3 == 1)
            self.flat += 1
            self.calls.append({'entry': name, 'engine': h - 1000, 'patch': [ph, pw], 'mask': mask, 'gaussian': self._gauss(g, ph, pw),
                               'images': [self._image(K, C, image, Hp, Wp, n_tiles, ty, tx, l16, seg)]})
            return 0
        if name == 'ts2d_ensemble_predict_tiled_export':
            handles, n_eng, desc, exd, n, ph, pw, mask, g, full = a
            hs = [addr(handles[i]) for i in range(n_eng)]
        else:
            exd, full = None, None
            if name == 'ts2d_engine_predict_tiled_export':
                h, desc, exd, n, ph, pw, mask, g, full = a
            else:
                h, desc, n, ph, pw, mask, g = a
            hs = [addr(h)]
        K, C = self.k_of[hs[0]]
        for f, h in enumerate(hs):
            self.flag_of[h] = int(self.inf and len(hs) > 1 and f == 1)
        self.calls.append({'entry': name, 'engines': [h - 1000 for h in hs], 'n_images': n, 'patch': [ph, pw], 'mask': mask,
                           'gaussian': self._gauss(g, ph, pw), 'full_batch': full, 'exports': exd is not None,
                           'images': self._descs(K, C, desc, exd, n)})
        return 0


STUB = Stub()


def describe(x):
    """A returned value in a comparable form: arrays by shape / dtype / hash, torch tensors likewise, containers recursively."""
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, (list, tuple)):
        return [describe(v) for v in x]
    kind = 'torch' if type(x).__module__.startswith('torch') else 'numpy'
    a = x.numpy() if kind == 'torch' else np.asarray(x)
    return {'kind': kind, 'shape': list(a.shape), 'dtype': str(a.dtype), 'sha': sha(a)}


def run(records, name, fn, engines=(), inf=True):
    STUB.reset(inf)
    for e in engines:
        e.__dict__.pop('last_tiled_inf', None)
        e.__dict__.pop('last_tiled_inf_per_image', None)
    rec = {'scenario': name}
    try:
        rec['result'] = describe(fn())
    except Exception as ex:                   # the text of every refusal is part of the record
        rec['error'] = [type(ex).__name__, str(ex)]
    rec['calls'] = STUB.calls
    rec['inf'] = [[getattr(e, 'last_tiled_inf', 'unset'), getattr(e, 'last_tiled_inf_per_image', 'unset')] for e in engines]
    records.append(rec)


def arch_of(K=3, C=2):
    return UNetArch(input_channels=C, num_classes=K, n_stages=2, features_per_stage=(32, 32), kernel_sizes=((3, 3),) * 2,
                    strides=((1, 1), (2, 2)), n_conv_per_stage=(2, 2), n_conv_per_stage_decoder=(2,))


def tiles_for(hw, patch):
    return [(y, x) for y in sorted({0, hw[0] - patch[0]}) for x in sorted({0, hw[1] - patch[1]})]


def engine_matrix(records):
    from totalsegmentator2d_amd.engine import Engine, predict_tiled_export_ensemble
    arch, patch = arch_of(), (32, 32)
    es = [Engine(arch, None) for _ in range(3)]
    rng = np.random.default_rng(2024)
    extents = [(40, 32), (32, 48), (50, 70)]
    imgs = [rng.standard_normal((arch.input_channels,) + hw).astype(np.float32) for hw in extents]
    imgs[1] = np.asfortranarray(imgs[1])                       # a non-contiguous input: the marshaller makes the copy
    tiles = [tiles_for(hw, patch) for hw in extents]
    exps = [(4, 0, 30, 32, 45, 20), (0, 8, 32, 33, 32, 33), (1, 2, 48, 60, 17, 90)]
    gauss = np.linspace(0.1, 10, patch[0] * patch[1]).reshape(patch).astype(np.float64)     # converted to half by the marshaller
    sets = [[0], [0, 1, 2]]
    flags2, flags4 = list(itertools.product([False, True], repeat=2)), list(itertools.product([False, True], repeat=4))
    for axes, g, idx in itertools.product([None, (0,), (1,), (0, 1)], [None, gauss], sets):
        im, tl, ex = [imgs[i] for i in idx], [tiles[i] for i in idx], [exps[i] for i in idx]
        tag = f'axes={axes} g={g is not None} n={len(idx)}'
        for wl, ws in flags2:
            if len(idx) == 1:
                for i in range(3):
                    run(records, f'predict_tiled image={i} {tag} logits={wl} seg={ws}',
                        lambda: es[0].predict_tiled(imgs[i], patch, tiles[i], axes, g, want_logits=wl, want_seg=ws), es[:1])
            run(records, f'predict_tiled_batch {tag} logits={wl} seg={ws}',
                lambda: es[0].predict_tiled_batch(im, patch, tl, axes, g, want_logits=wl, want_seg=ws), es[:1])
        for (ws, wf, wl, wp), e, full in itertools.product(flags4, [ex, None], [True, False]):
            kw = dict(want_seg=ws, want_f32=wf, want_logits=wl, want_padded_seg=wp, full_batch=full)
            t = f'{tag} exports={e is not None} seg={ws} f32={wf} logits={wl} pseg={wp} full={full}'
            run(records, f'predict_tiled_export {t}', lambda: es[0].predict_tiled_export(im, patch, tl, e, axes, g, **kw), es[:1])
            for F in (1, 2, 3):
                run(records, f'ensemble F={F} {t}', lambda: predict_tiled_export_ensemble(es[:F], im, patch, tl, e, axes, g, **kw), es)
    # defaults of every keyword, and the refusals
    run(records, 'defaults predict_tiled', lambda: es[0].predict_tiled(imgs[0], patch, tiles[0]), es[:1])
    run(records, 'defaults predict_tiled_batch', lambda: es[0].predict_tiled_batch(imgs, patch, tiles), es[:1])
    run(records, 'defaults predict_tiled_export', lambda: es[0].predict_tiled_export(imgs, patch, tiles, exps), es[:1])
    run(records, 'defaults ensemble', lambda: predict_tiled_export_ensemble(es[:2], imgs, patch, tiles, exps), es)
    run(records, 'empty predict_tiled_batch', lambda: es[0].predict_tiled_batch([], patch, []), es[:1])
    run(records, 'empty predict_tiled_export', lambda: es[0].predict_tiled_export([], patch, [], []), es[:1])
    run(records, 'empty ensemble', lambda: predict_tiled_export_ensemble(es[:2], [], patch, [], None, want_seg=False, want_logits=True), es)
    wrong_c = rng.standard_normal((3, 40, 32)).astype(np.float32)
    flat, stack = imgs[0][0], imgs[0][:, None]
    entries = {'predict_tiled_batch': lambda im, tl, ex, **kw: es[0].predict_tiled_batch(im, patch, tl, **kw),
               'predict_tiled_export': lambda im, tl, ex, **kw: es[0].predict_tiled_export(im, patch, tl, ex, **kw),
               'ensemble': lambda im, tl, ex, **kw: predict_tiled_export_ensemble(es[:2], im, patch, tl, ex, **kw)}
    for bad_name, bad in (('channels', wrong_c), ('ndim2', flat), ('ndim4', stack)):
        run(records, f'illegal predict_tiled {bad_name}', lambda: es[0].predict_tiled(bad, patch, tiles[0]), es[:1])
        for name, fn in entries.items():
            run(records, f'illegal {name} {bad_name} at image 1', lambda: fn([imgs[0], bad, imgs[2]], [tiles[0]] * 3, [exps[0]] * 3), es)
    for name, fn in entries.items():
        run(records, f'illegal {name} tiles length', lambda: fn(imgs, tiles[:2], exps), es)
        run(records, f'illegal {name} exports length', lambda: fn(imgs, tiles, exps[:1]), es)
        run(records, f'illegal {name} both lengths', lambda: fn(imgs[:2], tiles, exps[:1]), es)
        if name == 'predict_tiled_batch':
            run(records, f'illegal {name} nothing requested', lambda: fn(imgs, tiles, None, want_logits=False, want_seg=False), es)
            run(records, f'illegal {name} nothing requested and lengths', lambda: fn(imgs, tiles[:1], None, want_logits=False), es)
            continue
        run(records, f'illegal {name} nothing resampled', lambda: fn(imgs, tiles, exps, want_seg=False, want_logits=True), es)
        run(records, f'illegal {name} resampled without exports', lambda: fn(imgs, tiles, None), es)
        run(records, f'illegal {name} f32 without exports', lambda: fn(imgs, tiles, None, want_seg=False, want_f32=True, want_logits=True), es)
        run(records, f'illegal {name} nothing without exports', lambda: fn(imgs, tiles, None, want_seg=False), es)
        run(records, f'illegal {name} nothing and lengths', lambda: fn(imgs, tiles[:1], None, want_seg=False), es)
    run(records, 'illegal predict_tiled nothing requested', lambda: es[0].predict_tiled(imgs[0], patch, tiles[0], want_logits=False), es[:1])
    run(records, 'illegal ensemble no engines', lambda: predict_tiled_export_ensemble([], imgs, patch, tiles, exps), es)
    run(records, 'illegal ensemble bad extent', lambda: predict_tiled_export_ensemble(es[:2], imgs[:1], patch, tiles[:1], [(0, 0, 8, 8, -3, 5)]), es)
    for e in es:
        e.close()


def predictor_matrix(records):
    from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor
    arch, patch = arch_of(), (32, 32)
    rng = np.random.default_rng(77)
    single = [rng.standard_normal((arch.input_channels, 1) + hw).astype(np.float32) for hw in [(50, 70), (20, 32), (40, 33)]]
    stack = rng.standard_normal((arch.input_channels, 3, 45, 40)).astype(np.float32)
    out3 = [(1, 61, 80), None, (50, 21)]
    try:
        import torch
        as_torch = torch.from_numpy(single[0].copy())
    except ImportError:
        as_torch = None
    for folds, mirror, gaussian in itertools.product((1, 2), (None, (0,), (0, 1)), (True, False)):
        p = HIPnnUNetPredictor(tile_step_size=0.5, use_mirroring=mirror is not None, use_gaussian=gaussian)
        p.manual_initialization(arch, [np.zeros(arch.n_params(), np.float32)] * folds, patch, inference_allowed_mirroring_axes=mirror)
        for inf in (False, True):
            tag = f'folds={folds} mirror={mirror} gaussian={gaussian} inf={inf}'
            go = lambda name, fn: run(records, f'predictor {name} {tag}', fn, p.engines, inf)
            for f in range(folds):
                go(f'sliding_window fold={f} single', lambda: p.predict_sliding_window_return_logits(single[0], f))
                go(f'sliding_window fold={f} stack', lambda: p.predict_sliding_window_return_logits(stack, f))
            go('logits single', lambda: p.predict_logits_from_preprocessed_data(single[0]))
            go('logits stack', lambda: p.predict_logits_from_preprocessed_data(stack))
            go('logits small', lambda: p.predict_logits_from_preprocessed_data(single[1]))
            go('logits_batch 1', lambda: p.predict_logits_from_preprocessed_data_batch(single[:1]))
            go('logits_batch 3', lambda: p.predict_logits_from_preprocessed_data_batch(single))
            go('logits_batch mixed', lambda: p.predict_logits_from_preprocessed_data_batch([single[0], stack, single[2]]))
            go('logits_batch empty', lambda: p.predict_logits_from_preprocessed_data_batch([]))
            go('seg single', lambda: p.predict_segmentation_from_preprocessed_data(single[0]))
            go('seg single out_shape', lambda: p.predict_segmentation_from_preprocessed_data(single[0], out_shape=(1, 61, 80)))
            go('seg single out_shape own', lambda: p.predict_segmentation_from_preprocessed_data(single[0], out_shape=(50, 70)))
            go('seg single out_shape bad', lambda: p.predict_segmentation_from_preprocessed_data(single[0], out_shape=(2, 50, 70)))
            go('seg stack', lambda: p.predict_segmentation_from_preprocessed_data(stack))
            go('seg_batch 1', lambda: p.predict_segmentation_from_preprocessed_data_batch(single[:1]))
            go('seg_batch 3', lambda: p.predict_segmentation_from_preprocessed_data_batch(single))
            go('seg_batch 3 out_shapes', lambda: p.predict_segmentation_from_preprocessed_data_batch(single, out_shapes=out3))
            go('seg_batch 3 out_shapes none', lambda: p.predict_segmentation_from_preprocessed_data_batch(single, out_shapes=[None] * 3))
            go('seg_batch 1 out_shapes', lambda: p.predict_segmentation_from_preprocessed_data_batch(single[:1], out_shapes=out3[:1]))
            go('seg_batch out_shapes length', lambda: p.predict_segmentation_from_preprocessed_data_batch(single, out_shapes=out3[:2]))
            go('seg_batch with stack', lambda: p.predict_segmentation_from_preprocessed_data_batch([single[0], stack]))
            go('seg_batch empty', lambda: p.predict_segmentation_from_preprocessed_data_batch([]))
            go('illegal logits ndim', lambda: p.predict_logits_from_preprocessed_data(single[0][0]))
            go('illegal logits_batch ndim at 1', lambda: p.predict_logits_from_preprocessed_data_batch([single[0], single[1][0]]))
            go('illegal logits channels', lambda: p.predict_logits_from_preprocessed_data(np.concatenate([single[0]] * 2)[:3]))
            go('illegal logits_batch channels at 1', lambda: p.predict_logits_from_preprocessed_data_batch([single[0], np.concatenate([single[1]] * 2)[:3]]))
            if as_torch is not None:
                go('logits torch', lambda: p.predict_logits_from_preprocessed_data(as_torch))
                go('logits_batch torch', lambda: p.predict_logits_from_preprocessed_data_batch([as_torch, single[1]]))
                go('seg torch', lambda: p.predict_segmentation_from_preprocessed_data(as_torch))
                go('seg_batch torch', lambda: p.predict_segmentation_from_preprocessed_data_batch([as_torch, single[1]]))
        p.close()
    # mirror axes the 2-D window cannot take: the assertion, on every route
    for folds in (1, 2):
        p = HIPnnUNetPredictor(use_mirroring=True)
        p.manual_initialization(arch, [np.zeros(arch.n_params(), np.float32)] * folds, patch, inference_allowed_mirroring_axes=(0, 1, 2))
        for name, fn in (('logits', lambda: p.predict_logits_from_preprocessed_data(single[0])),
                         ('logits_batch', lambda: p.predict_logits_from_preprocessed_data_batch(single)),
                         ('seg', lambda: p.predict_segmentation_from_preprocessed_data(single[0])),
                         ('seg out_shape', lambda: p.predict_segmentation_from_preprocessed_data(single[0], out_shape=(61, 80))),
                         ('seg_batch', lambda: p.predict_segmentation_from_preprocessed_data_batch(single)),
                         ('seg_batch out_shapes', lambda: p.predict_segmentation_from_preprocessed_data_batch(single, out_shapes=out3))):
            run(records, f'predictor illegal mirror axes {name} folds={folds}', fn, p.engines, False)
        p.close()


def signatures():
    _lib.load, _lib._lib = REAL_LOAD, None
    lib = _lib.load()
    out = {}
    for name in sorted(_lib.SYMBOLS):
        if not hasattr(lib, name):
            out[name] = 'absent'
            continue
        fn = getattr(lib, name)
        out[name] = [getattr(fn.restype, '__name__', repr(fn.restype)), None if fn.argtypes is None else [t.__name__ for t in fn.argtypes]]
    return out


def main():
    out = sys.argv[1]
    _lib.load = lambda: STUB
    records = []
    engine_matrix(records)
    predictor_matrix(records)
    with open(out, 'w') as f:
        json.dump(records, f, indent=0, sort_keys=True, default=lambda o: o.item() if hasattr(o, 'item') else str(o))
        f.write('\n')
    n_calls = sum(len(r['calls']) for r in records)
    print(f'{len(records)} scenarios, {n_calls} recorded library calls, {sum("error" in r for r in records)} refusals -> {out}')
    print('sha256', hashlib.sha256(open(out, 'rb').read()).hexdigest())
    if '--signatures' in sys.argv:
        sig = sys.argv[sys.argv.index('--signatures') + 1]
        with open(sig, 'w') as f:
            json.dump(signatures(), f, indent=0, sort_keys=True)
            f.write('\n')
        print('signatures sha256', hashlib.sha256(open(sig, 'rb').read()).hexdigest(), '->', sig)


if __name__ == '__main__':
    main()
