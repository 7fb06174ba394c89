"""Call record of the sliding-window Python layers (engine.py, predictor.py, model.py) against a STUB of the C library: what each public
method hands to which C entry, in a pointer-free form, plus what it returns and what it raises.  No GPU and no built library needed.
The sections: the matrix of r14 (the flat, batch, export and ensemble-export entries; first, and hashed on its own), the wrappers of the
newer tails (label maps, regions, probabilities, probabilities of stacks, the *_from_logits), the predictor's fast-path methods for a model
of each convention, the keywords they hand to ``_sliding_window_batch``, and ``HIPModel._run`` over a recording double of the predictor.

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
                'ts2d_ensemble_predict_tiled_export', 'ts2d_engine_tiled_inf_flag', 'ts2d_ensemble_predict_tiled_labelmap',
                'ts2d_ensemble_predict_tiled_regions', 'ts2d_ensemble_predict_tiled_probabilities', 'ts2d_ensemble_predict_tiled_probabilities_stack',
                'ts2d_labelmap_from_logits', 'ts2d_regions_from_logits', 'ts2d_probabilities_from_logits')
    RECT = ('src_y', 'src_x', 'src_h', 'src_w', 'out_h', 'out_w')
    PLACE = ('full_h', 'full_w', 'box_y', 'box_x')

    def __init__(self):
        self.calls, self.k_of, self.flag_of = [], {}, {}
        self.inf, self.ordinal, self.flat = False, 0, 0
        self.bases = []                        # arrays of a scenario's own: a pointer into one is recorded as (its index, the byte offset)

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

    def _where(self, ptr):
        """A pointer of a run view in a pointer-free form: which registered base array it lies in, and the byte offset from its start."""
        p = addr(ptr)
        if not p:
            return None
        for i, b in enumerate(self.bases):
            if b.ctypes.data <= p < b.ctypes.data + max(b.nbytes, 1):
                return [i, p - b.ctypes.data]
        return 'elsewhere'

    def _tails(self, name, K, xd, n, mode):
        """The per-image descriptors behind the TiledImage array of the newer entries, every output filled."""
        out = []
        for i in range(n):
            x = xd[i]
            r = {'rect': [getattr(x, f) for f in self.RECT]}
            if name.endswith('_probabilities'):
                r['place'] = [getattr(x, f) for f in self.PLACE]
                m = max(x.full_h, 0) * max(x.full_w, 0)
                r['prob_f32'] = self._fill(x.prob_f32, np.float32, K * m)
                r['decided_u8'] = self._fill(x.decided_u8, np.uint8, (K if mode == 0 else 1) * m)
            else:
                r['label_u8'] = self._fill(x.label_u8, np.uint8, max(x.out_h, 0) * max(x.out_w, 0))
            out.append(r)
        return out

    def _runs(self, K, rd, n_runs, mode):
        """The run descriptors of the stack probabilities: geometry, head strides, where each pointer lies, and every head of every view filled."""
        out = []
        for j in range(n_runs):
            x = rd[j]
            plane = max(x.n_slices, 0) * max(x.full_h, 0) * max(x.full_w, 0)
            r = {'rect': [getattr(x, f) for f in self.RECT], 'place': [getattr(x, f) for f in self.PLACE], 'first_image': x.first_image,
                 'n_slices': x.n_slices, 'prob_head_stride': x.prob_head_stride, 'decided_head_stride': x.decided_head_stride,
                 'prob_at': self._where(x.prob_f32), 'decided_at': self._where(x.decided_u8)}
            r['prob_f32'] = [self._fill((x.prob_f32 or 0) + 4 * k * x.prob_head_stride if x.prob_f32 else None, np.float32, plane) for k in range(K)]
            r['decided_u8'] = [self._fill(x.decided_u8 + k * x.decided_head_stride if x.decided_u8 else None, np.uint8, plane)
                               for k in range(K if mode == 0 else 1)]
            out.append(r)
        return out

    def _from_logits(self, name, a):
        device, lg, K, H, W, rect, oh, ow = a[:8]
        rec = {'entry': name, 'device': device, 'logits': {'shape': [K, H, W], 'sha': sha(at(lg, np.float16, K * H * W))},
               'rect': list(rect._obj), 'out': [oh, ow]}
        if name == 'ts2d_probabilities_from_logits':
            fh, fw, by, bx, mode, order, prob, dec = a[8:]
            m = max(fh, 0) * max(fw, 0)
            rec.update(place=[fh, fw, by, bx], mode=mode, order=None if not order else at(order, np.uint8, K).tolist(),
                       prob_f32=self._fill(prob, np.float32, K * m), decided_u8=self._fill(dec, np.uint8, (K if mode == 0 else 1) * m))
        else:
            order, out = (a[8], a[9]) if name == 'ts2d_regions_from_logits' else (None, a[8])
            rec.update(order=None if not order else at(order, np.uint8, K).tolist(), label_u8=self._fill(out, np.uint8, max(oh, 0) * max(ow, 0)))
        self.calls.append(rec)
        return 0

    def _ensemble(self, name, a):
        """ts2d_ensemble_predict_tiled_labelmap, _regions, _probabilities and _probabilities_stack."""
        handles, n_eng, desc = a[:3]
        mode = order = n_order = rd = n_runs = xd = None
        if name.endswith('_stack'):
            n, rd, n_runs, ph, pw, mask, g, full, mode, order, n_order = a[3:]
        else:
            xd, n, ph, pw, mask, g, full = a[3:10]
            if name.endswith('_regions'):
                order, n_order = a[10:]
            elif name.endswith('_probabilities'):
                mode, order, n_order = a[10:]
        hs = [addr(handles[i]) for i in range(n_eng)]
        K, C = self.k_of[hs[0]]
        for f, h in enumerate(hs):
            self.flag_of[h] = int(self.inf and len(hs) > 1 and f == 1)
        rec = {'entry': name, 'engines': [h - 1000 for h in hs], 'n_images': n, 'patch': [ph, pw], 'mask': mask, 'gaussian': self._gauss(g, ph, pw),
               'full_batch': full, 'mode': mode, 'n_order': n_order, 'order': None if not order else at(order, np.uint8, n_order).tolist(),
               'images': self._descs(K, C, desc, None, n)}
        if rd is not None:
            rec['n_runs'], rec['runs'] = n_runs, self._runs(K, rd, n_runs, mode)
        else:
            rec['tails'] = self._tails(name, K, xd, n, mode)
        self.calls.append(rec)
        return 0

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
        if name.endswith('_from_logits'):
            return self._from_logits(name, a)
        if name.startswith('ts2d_ensemble_') and name != 'ts2d_ensemble_predict_tiled_export':
            return self._ensemble(name, a)
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


def tail_matrix(records):
    """The wrappers of the newer tails: label maps, regions, probabilities, the probabilities of stacks and the three *_from_logits."""
    from totalsegmentator2d_amd import engine as E
    arch, patch = arch_of(), (32, 32)
    K = arch.num_classes
    es = [E.Engine(arch, None) for _ in range(2)]
    rng = np.random.default_rng(32)
    extents = [(40, 32), (32, 48), (50, 70)]
    imgs = [rng.standard_normal((arch.input_channels,) + hw).astype(np.float32) for hw in extents]
    imgs[2] = np.asfortranarray(imgs[2])
    tiles = [tiles_for(hw, patch) for hw in extents]
    rects = [(4, 0, 30, 32, 45, 20), (0, 8, 32, 33, 32, 33), (1, 2, 48, 60, 17, 90)]
    prects = [r + (r[4] + 5 + i, r[5] + 2, 3 + i, 1) for i, r in enumerate(rects)]
    gauss = np.linspace(0.1, 10, patch[0] * patch[1]).reshape(patch).astype(np.float64)
    order = (3, 1, 2)
    modes = [('multilabel', None), ('labelmap', None), ('regions', order)]
    for F, axes, g, idx in itertools.product((1, 2), [None, (0, 1)], [None, gauss], [[0], [0, 1, 2]]):
        im, tl, rc, prc = ([x[i] for i in idx] for x in (imgs, tiles, rects, prects))
        tag = f'F={F} axes={axes} g={g is not None} n={len(idx)}'
        for wl, full in itertools.product([False, True], repeat=2):
            t = f'{tag} logits={wl} full={full}'
            run(records, f'labelmap {t}', lambda: E.predict_tiled_labelmap_ensemble(es[:F], im, patch, tl, rc, axes, g, want_logits=wl, full_batch=full), es)
            run(records, f'regions {t}', lambda: E.predict_tiled_regions_ensemble(es[:F], im, patch, tl, rc, order, axes, g, want_logits=wl, full_batch=full), es)
            for (mode, co), wd in itertools.product(modes, [False, True]):
                run(records, f'probabilities {mode} decided={wd} {t}',
                    lambda: E.predict_tiled_probabilities_ensemble(es[:F], im, patch, tl, prc, mode, co, axes, g, want_decided=wd, want_logits=wl, full_batch=full), es)
    # the probabilities of stacks: 5 images of one extent in runs of 2 + 3 out of two volumes (a view with a head stride), then 1 + 1 + 3 of three
    stack = [rng.standard_normal((arch.input_channels, 40, 32)).astype(np.float32) for _ in range(5)]
    stl = [tiles[0]] * 5
    ten = prects[0]
    fh, fw = ten[6], ten[7]
    for F, (mode, co), wl, full, dec in itertools.product((1, 2), modes, [False, True], [False, True], [False, True]):
        heads = (K,) if mode == 'multilabel' else ()

        def go(split, z0):
            vols = [np.zeros((K, z0 + n + 1, fh, fw), np.float32) for n in split]
            decs = [np.zeros(heads + (z0 + n + 1, fh, fw), np.uint8) for n in split]
            STUB.bases = vols + decs
            runs, first = [], 0
            for v, d, n in zip(vols, decs, split):
                runs.append((first, n, ten, v[:, z0:z0 + n], (d[:, z0:z0 + n] if heads else d[z0:z0 + n]) if dec else None))
                first += n
            lg = E.predict_tiled_probabilities_stack_ensemble(es[:F], stack, patch, stl, runs, mode, co, (0,), gauss, want_logits=wl, full_batch=full)
            return [lg, vols, decs]
        for split, z0 in (([2, 3], 1), ([1, 1, 3], 0), ([5], 2)):
            run(records, f'stack probabilities F={F} {mode} logits={wl} full={full} decided={dec} split={split} z0={z0}', lambda: go(split, z0), es)
    STUB.bases = []
    # the *_from_logits wrappers
    lg = rng.standard_normal((K, 40, 36)).astype(np.float16)
    for rect, out_hw in (((2, 3, 30, 31), (45, 20)), ((0, 0, 40, 36), (40, 36))):
        run(records, f'labelmap_from_logits {rect}', lambda: E.labelmap_from_logits(lg, rect, out_hw))
        run(records, f'labelmap_from_logits {rect} device 1 f32 in', lambda: E.labelmap_from_logits(lg.astype(np.float32), rect, out_hw, device=1))
        run(records, f'regions_from_logits {rect}', lambda: E.regions_from_logits(lg, rect, out_hw, order, device=2))
        for (mode, co), wd in itertools.product(modes, [False, True]):
            run(records, f'probabilities_from_logits {rect} {mode} decided={wd}',
                lambda: E.probabilities_from_logits(lg, rect, out_hw, (out_hw[0] + 4, out_hw[1] + 9), (1, 2), mode, co, want_decided=wd, device=wd))
    # defaults, the empty call, the refusals
    run(records, 'defaults labelmap', lambda: E.predict_tiled_labelmap_ensemble(es, imgs, patch, tiles, rects), es)
    run(records, 'defaults regions', lambda: E.predict_tiled_regions_ensemble(es, imgs, patch, tiles, rects, order), es)
    run(records, 'defaults probabilities', lambda: E.predict_tiled_probabilities_ensemble(es, imgs, patch, tiles, prects, 'labelmap'), es)
    run(records, 'empty labelmap', lambda: E.predict_tiled_labelmap_ensemble(es, [], patch, [], []), es)
    run(records, 'empty regions', lambda: E.predict_tiled_regions_ensemble(es, [], patch, [], [], order), es)
    run(records, 'empty probabilities', lambda: E.predict_tiled_probabilities_ensemble(es, [], patch, [], [], 'multilabel'), es)
    run(records, 'empty stack probabilities', lambda: E.predict_tiled_probabilities_stack_ensemble(es, [], patch, [], [], 'multilabel'), es)
    calls = {'labelmap': lambda e, im, tl, rc, **kw: E.predict_tiled_labelmap_ensemble(e, im, patch, tl, rc, **kw),
             'regions': lambda e, im, tl, rc, co=order, **kw: E.predict_tiled_regions_ensemble(e, im, patch, tl, rc, co, **kw),
             'probabilities': lambda e, im, tl, rc, mode='regions', co=order, **kw: E.predict_tiled_probabilities_ensemble(
                 e, im, patch, tl, None if rc is None else [r + (99, 99, 0, 0) for r in rc], mode, co, **kw)}
    flat, wrong_c = imgs[0][0], rng.standard_normal((3, 40, 32)).astype(np.float32)
    for name, fn in calls.items():
        run(records, f'illegal {name} no engines', lambda: fn([], imgs, tiles, rects), es)
        run(records, f'illegal {name} no engines and no rects', lambda: fn([], imgs, tiles, None), es)
        run(records, f'illegal {name} no rects', lambda: fn(es, imgs, tiles, None), es)
        run(records, f'illegal {name} tiles length', lambda: fn(es, imgs, tiles[:2], rects), es)
        run(records, f'illegal {name} rects length', lambda: fn(es, imgs, tiles, rects[:1]), es)
        run(records, f'illegal {name} ndim at image 1', lambda: fn(es, [imgs[0], flat, imgs[2]], tiles, rects), es)
        run(records, f'illegal {name} channels at image 2', lambda: fn(es, [imgs[0], imgs[1], wrong_c], tiles, rects), es)
        run(records, f'illegal {name} bad extent', lambda: fn(es[:1], imgs[:1], tiles[:1], [(0, 0, 8, 8, -3, 5)]), es)
        if name != 'labelmap':
            run(records, f'illegal {name} class value', lambda: fn(es, imgs, tiles, rects, co=(1, 256, 2)), es)
            run(records, f'illegal {name} class value and no rects', lambda: fn(es, imgs, tiles, None, co=(1, -1, 2)), es)
            run(records, f'{name} short class order', lambda: fn(es, imgs, tiles, rects, co=(1, 2)), es)
    run(records, 'illegal probabilities mode', lambda: calls['probabilities'](es, imgs, tiles, rects, mode='softmax'), es)
    run(records, 'illegal probabilities mode and no engines', lambda: calls['probabilities']([], imgs, tiles, rects, mode='softmax'), es)
    run(records, 'illegal probabilities regions without order', lambda: calls['probabilities'](es, imgs, tiles, rects, co=None), es)
    run(records, 'illegal probabilities short rects', lambda: E.predict_tiled_probabilities_ensemble(es, imgs, patch, tiles, rects, 'multilabel'), es)
    vol, dvol = np.zeros((K, 5, fh, fw), np.float32), np.zeros((5, fh, fw), np.uint8)
    ro = vol.copy()
    ro.flags.writeable = False
    sruns = lambda prob, dec, n=5, r=ten: [(0, n, r, prob, dec)]
    scall = lambda e, runs, mode='labelmap', co=None, st=stack, tl=stl: E.predict_tiled_probabilities_stack_ensemble(e, st, patch, tl, runs, mode, co)
    for name, fn in (('no engines', lambda: scall([], sruns(vol, dvol))), ('mode', lambda: scall(es, sruns(vol, dvol), 'softmax')),
                     ('regions without order', lambda: scall(es, sruns(vol, dvol), 'regions')),
                     ('tiles length', lambda: scall(es, sruns(vol, dvol), tl=stl[:2])),
                     ('channels at image 3', lambda: scall(es, sruns(vol, dvol), st=stack[:3] + [wrong_c] + stack[4:])),
                     ('prob dtype', lambda: scall(es, sruns(vol.astype(np.float64), dvol))), ('prob shape', lambda: scall(es, sruns(vol[:, :4], dvol))),
                     ('prob read-only', lambda: scall(es, sruns(ro, dvol))), ('prob a list', lambda: scall(es, sruns(vol.tolist(), dvol))),
                     ('prob not dense', lambda: scall(es, sruns(np.zeros((K, 5, fh, 2 * fw), np.float32)[..., ::2], dvol))),
                     ('decided heads', lambda: scall(es, sruns(vol, np.zeros((K, 5, fh, fw), np.uint8)))),
                     ('decided without heads', lambda: scall(es, sruns(vol, dvol), 'multilabel')),
                     ('decided dtype at run 1', lambda: scall(es, [(0, 2, ten, vol[:, :2], dvol[:2]), (2, 3, ten, vol[:, 2:], dvol[2:].astype(np.int8))])),
                     ('short rect', lambda: scall(es, sruns(vol, dvol, r=ten[:6]))), ('bad extent', lambda: scall(es, sruns(vol[:, :, :0], None, r=ten[:6] + (-1, fw, 0, 0)))),
                     ('slices the library refuses', lambda: scall(es, sruns(vol[:, :2], dvol[:2], n=2)))):
        run(records, f'illegal stack probabilities {name}', fn, es)
    for name, fn in (('labelmap ndim', lambda: E.labelmap_from_logits(lg[0], (0, 0, 4, 4), (4, 4))),
                     ('regions ndim', lambda: E.regions_from_logits(lg[None], (0, 0, 4, 4), (4, 4), order)),
                     ('regions class value', lambda: E.regions_from_logits(lg, (0, 0, 4, 4), (4, 4), (1, 2, 300))),
                     ('regions ndim and class value', lambda: E.regions_from_logits(lg[0], (0, 0, 4, 4), (4, 4), (1, 2, 300))),
                     ('regions no order', lambda: E.regions_from_logits(lg, (0, 0, 4, 4), (4, 4), None)),
                     ('probabilities order the mode ignores', lambda: E.probabilities_from_logits(lg, (0, 0, 4, 4), (4, 4), (4, 4), (0, 0), 'labelmap', (1, 2))),
                     ('regions order length', lambda: E.regions_from_logits(lg, (0, 0, 4, 4), (4, 4), (1, 2))),
                     ('probabilities ndim', lambda: E.probabilities_from_logits(lg[0], (0, 0, 4, 4), (4, 4), (4, 4), (0, 0), 'labelmap')),
                     ('probabilities ndim and mode', lambda: E.probabilities_from_logits(lg[0], (0, 0, 4, 4), (4, 4), (4, 4), (0, 0), 'softmax')),
                     ('probabilities mode', lambda: E.probabilities_from_logits(lg, (0, 0, 4, 4), (4, 4), (4, 4), (0, 0), 'softmax')),
                     ('probabilities regions without order', lambda: E.probabilities_from_logits(lg, (0, 0, 4, 4), (4, 4), (4, 4), (0, 0), 'regions')),
                     ('probabilities order length', lambda: E.probabilities_from_logits(lg, (0, 0, 4, 4), (4, 4), (4, 4), (0, 0), 'regions', (1, 2))),
                     ('probabilities short rect', lambda: E.probabilities_from_logits(lg, (0, 0, 4), (4, 4), (4, 4), (0, 0), 'labelmap')),
                     ('labelmap negative extent', lambda: E.labelmap_from_logits(lg, (0, 0, 4, 4), (-4, 4))),
                     ('probabilities negative extent', lambda: E.probabilities_from_logits(lg, (0, 0, 4, 4), (4, 4), (-4, 4), (0, 0), 'multilabel'))):
        run(records, f'illegal from_logits {name}', fn)
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


CONVENTIONS = {
    'multilabel': None,                                         # (manual_initialization's own default: K foreground labels, multilabel)
    'labelmap': {'labels': {'background': 0, 'a': 1, 'b': 2}},
    'regions': {'labels': {'background': 0, 'whole': [1, 2, 3], 'core': [2, 3], 'inner': [3]}, 'regions_class_order': [1, 2, 3]}}


def dataset_json_of(convention, arch):
    extra = CONVENTIONS[convention]
    return None if extra is None else dict({'channel_names': {str(i): f'ch{i}' for i in range(arch.input_channels)}, 'file_ending': '.nrrd'}, **extra)


def fast_path_matrix(records):
    """The fast-path methods of the predictor behind the newer tails: label maps / regions, probabilities, stacks and their probabilities, for a
    model of each convention."""
    from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor
    arch, patch = arch_of(), (32, 32)
    rng = np.random.default_rng(3232)
    single = [rng.standard_normal((arch.input_channels, 1) + hw).astype(np.float32) for hw in [(50, 70), (20, 32), (40, 33)]]
    stacks = [rng.standard_normal((arch.input_channels,) + zhw).astype(np.float32) for zhw in [(3, 45, 40), (4, 33, 50)]]
    mixed = [stacks[0], single[0], stacks[1]]
    out3 = [(1, 61, 80), None, (50, 21)]
    full3, box3 = [(70, 90), None, (1, 60, 30)], [(5, 7), None, (0, 10, 9)]
    sout3 = [(3, 50, 44), None, (4, 33, 50)]
    sfull3, sbox3 = [(6, 60, 50), None, (4, 40, 52)], [(2, 4, 5), None, (0, 7, 2)]
    for convention, folds in itertools.product(CONVENTIONS, (1, 2)):
        p = HIPnnUNetPredictor(tile_step_size=0.5, use_mirroring=True, use_gaussian=True)
        p.manual_initialization(arch, [np.zeros(arch.n_params(), np.float32)] * folds, patch, dataset_json=dataset_json_of(convention, arch),
                                inference_allowed_mirroring_axes=(0, 1))
        for inf, budget in ((False, None), (True, None), (False, 60000)):
            if budget is not None:
                p.stack_call_bytes = budget                     # a call boundary falls inside a volume
            tag = f'{convention} folds={folds} inf={inf} budget={budget}'
            go = lambda name, fn: run(records, f'fast {name} {tag}', fn, p.engines, inf)
            if budget is None:
                for m, extra in (('labelmap', {}), ('segmentation', {}), ('probabilities', {}),
                                 ('probabilities', {'full_shape': (70, 90), 'box': (5, 7)}), ('probabilities', {'full_shape': (1, 70, 90), 'box': (0, 5, 7)})):
                    one = getattr(p, f'predict_{m}_from_preprocessed_data')
                    t = f'{m} {sorted(extra)}'
                    go(f'{t} single', lambda: one(single[0], **extra))
                    go(f'{t} single out_shape', lambda: one(single[0], out_shape=(1, 61, 80), **extra))
                    go(f'{t} single out_shape own', lambda: one(single[0], out_shape=(50, 70), **extra))
                    go(f'{t} single out_shape bad', lambda: one(single[0], out_shape=(2, 50, 70), **extra))
                    go(f'{t} single stack', lambda: one(stacks[0], **extra))
                    go(f'{t} single ndim', lambda: one(single[0][0], **extra))
                go('probabilities single box leaves', lambda: p.predict_probabilities_from_preprocessed_data(single[0], full_shape=(50, 70), box=(1, 0)))
                go('probabilities single box negative', lambda: p.predict_probabilities_from_preprocessed_data(single[0], full_shape=(60, 80), box=(-1, 0)))
                go('probabilities single full 3-D', lambda: p.predict_probabilities_from_preprocessed_data(single[0], full_shape=(2, 60, 80)))
                for m in ('labelmap', 'segmentation', 'probabilities'):
                    many = getattr(p, f'predict_{m}_from_preprocessed_data_batch')
                    go(f'{m} batch 1', lambda: many(single[:1]))
                    go(f'{m} batch 3', lambda: many(single))
                    go(f'{m} batch 3 out_shapes', lambda: many(single, out_shapes=out3))
                    go(f'{m} batch 3 out_shapes none', lambda: many(single, out_shapes=[None] * 3))
                    go(f'{m} batch out_shapes length', lambda: many(single, out_shapes=out3[:2]))
                    go(f'{m} batch out_shapes bad at 2', lambda: many(single, out_shapes=out3[:2] + [(0, 5)]))
                    go(f'{m} batch out_shapes short and malformed', lambda: many(single, out_shapes=[('a', 'b')]))      # (the segmentation method converts first)
                    go(f'{m} batch with stack', lambda: many([single[0], stacks[0]]))
                    go(f'{m} batch empty', lambda: many([]))
                    go(f'{m} batch empty out_shapes length', lambda: many([], out_shapes=[None]))
                many = p.predict_probabilities_from_preprocessed_data_batch
                go('probabilities batch 3 placed', lambda: many(single, out3, full3, box3))
                go('probabilities batch 3 placed one call per image', lambda: many(single, out3, full3, box3, one_call=False))
                go('probabilities batch 3 one call per image', lambda: many(single, one_call=False))
                go('probabilities batch boxes only', lambda: many(single, boxes=[(0, 0)] * 3))
                go('probabilities batch full_shapes length', lambda: many(single, full_shapes=full3[:1]))
                go('probabilities batch boxes length', lambda: many(single, None, full3, box3[:2]))
                go('probabilities batch box leaves at 1', lambda: many(single, None, None, [None, (1, 1), None]))
                go('stack single', lambda: p.predict_stack_from_preprocessed_data(stacks[0]))
                go('stack single out_shape', lambda: p.predict_stack_from_preprocessed_data(stacks[0], out_shape=sout3[0]))
                go('stack single out_shape bad Z', lambda: p.predict_stack_from_preprocessed_data(stacks[0], out_shape=(2, 50, 44)))
                go('stack single out_shape 2-D', lambda: p.predict_stack_from_preprocessed_data(stacks[0], out_shape=(50, 44)))
                go('stack single slice', lambda: p.predict_stack_from_preprocessed_data(single[2]))
                go('stack single ndim', lambda: p.predict_stack_from_preprocessed_data(stacks[0][0]))
                go('stack probabilities single', lambda: p.predict_stack_probabilities_from_preprocessed_data(stacks[0]))
                go('stack probabilities single placed', lambda: p.predict_stack_probabilities_from_preprocessed_data(stacks[0], sout3[0], sfull3[0], sbox3[0]))
                go('stack probabilities single box leaves', lambda: p.predict_stack_probabilities_from_preprocessed_data(stacks[0], None, (3, 45, 40), (1, 0, 0)))
                go('stack probabilities single full 2-D', lambda: p.predict_stack_probabilities_from_preprocessed_data(stacks[0], None, (45, 40)))
                go('stack probabilities single out_shape bad', lambda: p.predict_stack_probabilities_from_preprocessed_data(stacks[0], (50, 44)))
                go('stack probabilities single ndim', lambda: p.predict_stack_probabilities_from_preprocessed_data(stacks[0][0]))
            go('stack batch mixed', lambda: p.predict_stack_from_preprocessed_data_batch(mixed))
            go('stack batch mixed out_shapes', lambda: p.predict_stack_from_preprocessed_data_batch(mixed, sout3))
            go('stack probabilities batch mixed', lambda: p.predict_stack_probabilities_from_preprocessed_data_batch(mixed))
            go('stack probabilities batch mixed placed', lambda: p.predict_stack_probabilities_from_preprocessed_data_batch(mixed, sout3, sfull3, sbox3))
            if budget is None:
                go('stack batch out_shapes length', lambda: p.predict_stack_from_preprocessed_data_batch(mixed, sout3[:2]))
                go('stack batch out_shapes bad at 0', lambda: p.predict_stack_from_preprocessed_data_batch(mixed, [(4, 50, 44)] + sout3[1:]))
                go('stack batch empty', lambda: p.predict_stack_from_preprocessed_data_batch([]))
                go('stack batch empty out_shapes length', lambda: p.predict_stack_from_preprocessed_data_batch([], [None]))
                go('stack batch ndim at 1', lambda: p.predict_stack_from_preprocessed_data_batch([stacks[0], single[0][0]]))
                go('stack probabilities batch boxes length', lambda: p.predict_stack_probabilities_from_preprocessed_data_batch(mixed, None, sfull3, sbox3[:2]))
                go('stack probabilities batch box leaves at 2', lambda: p.predict_stack_probabilities_from_preprocessed_data_batch(mixed, None, None, [None, None, (1, 0, 0)]))
                go('stack probabilities batch empty', lambda: p.predict_stack_probabilities_from_preprocessed_data_batch([]))
                go('stack probabilities batch empty length', lambda: p.predict_stack_probabilities_from_preprocessed_data_batch([], [None]))
        p.close()
    # what the guards refuse whatever the inputs: mirror axes the 2-D window cannot take, a 3-D plan, folds without engines, more engines than folds
    for convention, folds in itertools.product(CONVENTIONS, (1, 2)):
        for kind in ('mirror axes', '3-D plan', 'no engines', 'an engine too many'):
            p = HIPnnUNetPredictor(use_mirroring=True)
            p.manual_initialization(arch, [np.zeros(arch.n_params(), np.float32)] * folds, patch, dataset_json=dataset_json_of(convention, arch),
                                    inference_allowed_mirroring_axes=(0, 1, 2) if kind == 'mirror axes' else (0, 1))
            engines = list(p.engines)
            if kind == '3-D plan':
                p.configuration_manager.patch_size = [16, 32, 32]
            elif kind == 'no engines':
                p.engines = []
            elif kind == 'an engine too many':
                p.engines = engines + engines[:1]
            for name, fn in (('labelmap', lambda: p.predict_labelmap_from_preprocessed_data(single[0])),
                             ('labelmap batch', lambda: p.predict_labelmap_from_preprocessed_data_batch(single, out3)),
                             ('segmentation', lambda: p.predict_segmentation_from_preprocessed_data(single[0])),
                             ('segmentation batch', lambda: p.predict_segmentation_from_preprocessed_data_batch(single, out3)),
                             ('probabilities', lambda: p.predict_probabilities_from_preprocessed_data(single[0], (61, 80))),
                             ('probabilities batch', lambda: p.predict_probabilities_from_preprocessed_data_batch(single)),
                             ('stack', lambda: p.predict_stack_from_preprocessed_data(stacks[0])),
                             ('stack batch', lambda: p.predict_stack_from_preprocessed_data_batch(mixed, sout3)),
                             ('stack probabilities', lambda: p.predict_stack_probabilities_from_preprocessed_data(stacks[0])),
                             ('stack probabilities batch', lambda: p.predict_stack_probabilities_from_preprocessed_data_batch(mixed))):
                if kind == '3-D plan' and not name.startswith('stack'):
                    continue                                    # (the single-slice methods have no such guard: they would tile in 3-D)
                run(records, f'fast guard {kind}: {name} {convention} folds={folds}', fn, engines, False)
            p.engines = engines
            p.close()


def window_keywords_matrix(records):
    """Which keywords each public method hands to ``_sliding_window_batch`` - the method tests/batch_util.py and tests/host_predictor.py override, some
    of them without the newer keywords: a keyword that is passed although it has its default breaks those doubles."""
    from totalsegmentator2d_amd.predictor import HIPnnUNetPredictor
    arch, patch = arch_of(), (32, 32)
    seen = []

    class Recording(HIPnnUNetPredictor):
        def _sliding_window_batch(self, list_of_data, fold=0, **kw):
            seen.append({'inputs': [list(np.shape(d)) for d in list_of_data], 'fold': fold, 'keywords': {k: repr(v) for k, v in sorted(kw.items())}})
            pair = 'probabilities' in kw
            one = lambda d: np.zeros((arch.num_classes,) + tuple(np.shape(d)[1:]), np.uint8 if kw.get('want_seg') or pair else np.float16)
            return [(one(d), one(d).astype(np.float32)) if pair else one(d) for d in list_of_data]
    single = [np.zeros((arch.input_channels, 1) + hw, np.float32) for hw in [(50, 70), (20, 32)]]
    stack = np.zeros((arch.input_channels, 3, 45, 40), np.float32)
    for convention, folds in itertools.product(CONVENTIONS, (1, 2)):
        p = Recording()
        p.manual_initialization(arch, [np.zeros(arch.n_params(), np.float32)] * folds, patch, dataset_json=dataset_json_of(convention, arch))
        for name, fn in (('logits', lambda: p.predict_logits_from_preprocessed_data(single[0])), ('logits stack', lambda: p.predict_logits_from_preprocessed_data(stack)),
                         ('logits batch', lambda: p.predict_logits_from_preprocessed_data_batch(single + [stack])),
                         ('window', lambda: p.predict_sliding_window_return_logits(stack, folds - 1)),
                         ('segmentation', lambda: p.predict_segmentation_from_preprocessed_data(single[0])),
                         ('segmentation out_shape', lambda: p.predict_segmentation_from_preprocessed_data(single[0], (61, 80))),
                         ('segmentation batch', lambda: p.predict_segmentation_from_preprocessed_data_batch(single)),
                         ('segmentation batch out_shapes', lambda: p.predict_segmentation_from_preprocessed_data_batch(single, [(61, 80), None])),
                         ('labelmap', lambda: p.predict_labelmap_from_preprocessed_data(single[0])),
                         ('labelmap out_shape', lambda: p.predict_labelmap_from_preprocessed_data(single[0], (61, 80))),
                         ('labelmap batch', lambda: p.predict_labelmap_from_preprocessed_data_batch(single)),
                         ('labelmap batch out_shapes', lambda: p.predict_labelmap_from_preprocessed_data_batch(single, [(61, 80), None])),
                         ('probabilities', lambda: p.predict_probabilities_from_preprocessed_data(single[0], None, (60, 80), (1, 2))),
                         ('probabilities batch', lambda: p.predict_probabilities_from_preprocessed_data_batch(single)),
                         ('probabilities batch per image', lambda: p.predict_probabilities_from_preprocessed_data_batch(single, [(61, 80), None], one_call=False))):
            del seen[:]
            rec = {'scenario': f'window keywords {name} {convention} folds={folds}', 'calls': []}
            try:
                rec['result'] = describe(fn())
            except Exception as ex:
                rec['error'] = [type(ex).__name__, str(ex)]
            rec['window'] = list(seen)
            records.append(rec)
        p.close()


FAST_METHODS = {    # the fast-path methods of a predictor: the keywords of the single-case method (the batch method's are their plurals)
    'predict_segmentation_from_preprocessed_data': ('out_shape',), 'predict_labelmap_from_preprocessed_data': ('out_shape',),
    'predict_probabilities_from_preprocessed_data': ('out_shape', 'full_shape', 'box'), 'predict_stack_from_preprocessed_data': ('out_shape',),
    'predict_stack_probabilities_from_preprocessed_data': ('out_shape', 'full_shape', 'box')}
WINDOW_KEYWORDS = ('out_shapes', 'labelmap', 'regions', 'probabilities')
PLURAL = {'out_shape': 'out_shapes', 'full_shape': 'full_shapes', 'box': 'boxes'}


def recording_predictor(convention, arch, calls, lacks=(), answers_none=(), raises=None, patch=(32, 32), transpose=(0, 1, 2)):
    """A double of the predictor for ``HIPModel._run``: every method records its call and answers arrays whose shape tells the method and the
    input apart.  ``lacks``: names of methods, or ``method:keyword`` / ``_sliding_window_batch:keyword``, that this predictor does not have;
    ``answers_none``: methods that answer None (the batch method: for the whole batch); ``raises``: a method that raises 'input 1: boom'."""
    from types import SimpleNamespace

    def answer(method, i, d, pair):
        a = np.full((1 + i, len(method) % 7 + 1) + tuple(np.shape(d)[1:]), i, np.uint8)
        return (a, a.astype(np.float32)) if pair else a

    def make(method, keywords, batch):
        names = [PLURAL[k] if batch else k for k in keywords if f'{method}:{k}' not in lacks]
        pair = 'probabilities' in method

        def body(self, data, **kw):
            assert set(kw) <= set(names), (method, kw)
            calls.append({'method': method + ('_batch' if batch else ''), 'inputs': [list(np.shape(d)) for d in (data if batch else [data])],
                          'keywords': {k: repr(v) for k, v in sorted(kw.items())}})
            if raises == method:
                raise RuntimeError('input 1: boom')
            if method in answers_none:
                return None
            return [answer(method, i, d, pair) for i, d in enumerate(data)] if batch else answer(method, 0, data, pair)
        # (a real signature: the model probes the keywords with inspect)
        src = f"lambda self, data{''.join(f', {n}=None' for n in names)}: body(self, data{''.join(f', {n}={n}' for n in names)})"
        return eval(src, {'body': lambda self, data, **kw: body(self, data, **{k: v for k, v in kw.items() if v is not None})})
    members = {}
    for method, keywords in FAST_METHODS.items():
        if method not in lacks:
            members[method], members[method + '_batch'] = make(method, keywords, False), make(method, keywords, True)
    members['predict_logits_from_preprocessed_data'] = make('predict_logits_from_preprocessed_data', (), False)
    members['predict_logits_from_preprocessed_data_batch'] = make('predict_logits_from_preprocessed_data', (), True)
    window = [k for k in WINDOW_KEYWORDS if f'_sliding_window_batch:{k}' not in lacks]
    if '_sliding_window_batch' not in lacks:
        members['_sliding_window_batch'] = eval(f"lambda self, list_of_data, fold=0{''.join(f', {k}=None' for k in window)}: None")
    p = type('RecordingPredictor', (), members)()
    p.dataset_json = dataset_json_of(convention, arch) or {
        'channel_names': {str(i): f'ch{i}' for i in range(arch.input_channels)}, 'labels': {'background': 0, 'a': 1, 'b': 2, 'c': 3},
        'file_ending': '.nrrd', 'multilabel': True}
    p.configuration_manager = SimpleNamespace(patch_size=list(patch), spacing=[1.5, 1.5])
    p.plans_manager = SimpleNamespace(plans={}, transpose_forward=list(transpose), transpose_backward=list(transpose))
    p.verbose, p.engines = False, []
    return p


def model_matrix(records):
    """``HIPModel._run`` over a recording double of the predictor: which predictor method each case reaches, with which keywords, what the export
    step receives, which error names which input."""
    from totalsegmentator2d_amd import model as M
    arch = arch_of()
    C = arch.input_channels
    box = lambda at, shape: [[a, a + s] for a, s in zip(at, shape)]
    cases = {'on': (np.zeros((C, 1, 40, 48), np.float32), {'shape_after_cropping_and_before_resampling': (1, 40, 48), 'shape_before_cropping': (1, 50, 60),
                                                           'bbox_used_for_cropping': box((0, 3, 5), (1, 40, 48))}),
             'off': (np.zeros((C, 1, 40, 48), np.float32), {'shape_after_cropping_and_before_resampling': (1, 55, 66), 'shape_before_cropping': (1, 60, 70),
                                                            'bbox_used_for_cropping': box((0, 2, 1), (1, 55, 66))}),
             'stack': (np.zeros((C, 3, 40, 48), np.float32), {'shape_after_cropping_and_before_resampling': (3, 55, 66), 'shape_before_cropping': (5, 60, 70),
                                                              'bbox_used_for_cropping': box((1, 2, 1), (3, 55, 66))}),
             'bare': (np.zeros((C, 1, 33, 32), np.float32), {'shape_before_cropping': (1, 33, 32), 'bbox_used_for_cropping': box((0, 0, 0), (1, 33, 32))})}
    switches = ('device_threshold', 'device_labelmap', 'device_regions', 'device_probabilities', 'device_stack', 'device_stack_probabilities')
    variants = [('full', {})] + [(f'lacks {m}', {'lacks': (m,)}) for m in list(FAST_METHODS) + ['_sliding_window_batch']] \
        + [(f'lacks {m}:{k}', {'lacks': (f'{m}:{k}',)}) for m, kws in FAST_METHODS.items() for k in kws] \
        + [(f'lacks _sliding_window_batch:{k}', {'lacks': (f'_sliding_window_batch:{k}',)}) for k in WINDOW_KEYWORDS] \
        + [(f'none from {m}', {'answers_none': (m,)}) for m in FAST_METHODS] + [('none from all', {'answers_none': tuple(FAST_METHODS)})] \
        + [(f'raises in {m}', {'raises': m}) for m in list(FAST_METHODS) + ['predict_logits_from_preprocessed_data']] \
        + [('3-D plan', {'patch': (16, 32, 32)}), ('transposed plan', {'transpose': (1, 0, 2)})]
    exported = []

    def export(logits, props, cm, pm, dataset_json, ofile, **more):
        exported.append({'logits': describe(list(logits) if isinstance(logits, tuple) else logits), 'ofile': ofile,
                         'more': {k: (describe(v) if k == 'probabilities' else v if isinstance(v, bool) else 'set') for k, v in sorted(more.items())}})
        return len(exported)
    real_export, M.export_prediction_from_logits = M.export_prediction_from_logits, export
    try:
        for convention, batched, probs, (vname, variant) in itertools.product(CONVENTIONS, (False, True), (False, True), variants):
            for off in (None,) + (switches if vname == 'full' else ()):
                for names in (('on', 'off', 'stack', 'bare'), ('off',), ('stack', 'on')):
                    calls = []
                    m = M.HIPModel({'synthetic': {'arch': arch, 'blobs': [], 'patch_size': (32, 32), 'dataset_json': recording_predictor(convention, arch, []).dataset_json}})
                    m._predictor = recording_predictor(convention, arch, calls, **variant)
                    m._preprocess_input = lambda img: (None, cases[img][0], dict(cases[img][1]))
                    if off is not None:
                        setattr(m, off, False)
                    del exported[:]
                    stamps = {}
                    rec = {'scenario': f'model {convention} batched={batched} probabilities={probs} predictor={vname} off={off} cases={names}'}
                    try:
                        rec['result'] = m._run({n: n for n in names}, None, True, batched, stamps, save_probabilities=probs)
                    except Exception as ex:
                        rec['error'] = [type(ex).__name__, str(ex)]
                    rec['calls'], rec['exported'] = calls, list(exported)
                    rec['stamps'] = {n: sorted(s) for n, s in sorted(stamps.items())}
                    records.append(rec)
    finally:
        M.export_prediction_from_logits = real_export


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
    dump = lambda recs: json.dumps(recs, indent=0, sort_keys=True, default=lambda o: o.item() if hasattr(o, 'item') else str(o)) + '\n'
    count = lambda recs: (f'{len(recs)} scenarios, {sum(len(r["calls"]) for r in recs)} recorded library calls, '
                          f'{sum("error" in r for r in recs)} refusals')
    print('r14 part:', count(records), 'sha256', hashlib.sha256(dump(records).encode()).hexdigest())      # (the whole record of r14's script)
    n14 = len(records)
    for part in (tail_matrix, fast_path_matrix, window_keywords_matrix, model_matrix):
        n0 = len(records)
        part(records)
        print(f'{part.__name__}:', count(records[n0:]))
    with open(out, 'w') as f:
        f.write(dump(records))
    print(f'{count(records)} -> {out}')
    print('sha256', hashlib.sha256(open(out, 'rb').read()).hexdigest())
    if '--signatures' in sys.argv:
        sig = sys.argv[sys.argv.index('--signatures') + 1]
        with open(sig, 'w') as f:
            json.dump(signatures(), f, indent=0, sort_keys=True)
            f.write('\n')
        print('signatures sha256', hashlib.sha256(open(sig, 'rb').read()).hexdigest(), '->', sig)


if __name__ == '__main__':
    main()
