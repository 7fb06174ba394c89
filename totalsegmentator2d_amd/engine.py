"""``Engine`` - Python handle on one HIP engine (one sub-model / fold on one GPU).

Thin wrapper over the C-ABI (include/ts2d_engine.h).  It replaces ``nnUNetPredictor.network`` (built at reference
``ts2d/core/inference/nnu.py:164-165``, called inside ``predict_logits_from_preprocessed_data``, reference
``ts2d/core/inference/prediction_worker.py:209``).  torch is optional: numpy host arrays always work, torch CUDA
tensors are consumed zero-copy through their ``data_ptr()``.
"""
from __future__ import annotations

import ctypes
import weakref
from typing import Dict, Optional, Tuple

import numpy as np

from . import _lib
from .arch import UNetArch


def _desc(arch: UNetArch) -> _lib.ArchDesc:
    arch.validate()
    d = _lib.ArchDesc()
    d.input_channels, d.num_classes, d.n_stages = arch.input_channels, arch.num_classes, arch.n_stages
    for i, f in enumerate(arch.features_per_stage):
        d.features[i] = int(f)
    for i, c in enumerate(arch.n_conv_per_stage):       # (ignored by ts2d_engine_create_residual)
        d.n_conv_enc[i] = int(c)
    for i, c in enumerate(arch.n_conv_per_stage_decoder):
        d.n_conv_dec[i] = int(c)
    d.norm_eps, d.leaky_slope = arch.norm_eps, arch.leaky_slope
    for i, st in enumerate(arch.strides):
        d.strides[i][0], d.strides[i][1] = int(st[0]), int(st[1])
    return d


def _residual_desc(arch: UNetArch) -> _lib.ResidualDesc:
    r = _lib.ResidualDesc()
    for i, b in enumerate(arch.n_blocks_per_stage):
        r.n_blocks[i] = int(b)
    return r


def _is_torch(x) -> bool:
    return type(x).__module__.startswith('torch') and hasattr(x, 'data_ptr')


def set_precision_opted_in(e: 'Engine', mode):
    """``e.set_precision(mode)`` for a caller who has NAMED the mode (``HIPnnUNetPredictor(precision=...)``, ``SubModelSet(precision=...)``):
    the 16-bit mode of a residual-encoder engine is opt-in at the C-ABI (option ``"resf16"``), and naming ``'f16'`` is the opt-in."""
    if mode in ('f16', _lib.PRECISION_F16) and e.arch.encoder == 'residual':
        try:
            e.set_option('resf16', 1)
        except RuntimeError as err:
            if 'unknown option' not in str(err):
                raise
            raise RuntimeError(f"{_lib.LIB_PATH} was built before the option 'resf16': rebuild it to run a ResidualEncoderUNet in the 16-bit mode") from err
    e.set_precision(mode)


class Engine:
    default_options: Dict[str, int] = {}     # dispatch options every new handle starts with (empty in the product; test modules that address
                                             # the large-batch kernels at small B set {'sbk': 0})

    def __init__(self, arch: UNetArch, blob: Optional[np.ndarray], device: int = 0, options: Optional[Dict[str, int]] = None):
        """blob: fp32 weight blob (:func:`weights.pack_blob`) or None for a replica to be filled by broadcast.
        options: kernel-dispatch options (:meth:`set_option`), e.g. ``{'upc': 0}`` - tests and A/B scripts."""
        self.lib = _lib.load()
        self.arch = arch
        self.device = int(device)
        self._keep = False           # one buffer per activation: switched on by the USER (keep_activations)
        self._auto_keep = False      # ... or by debug_tensor, until the next forward (which returns to the shared arena)
        self._last = None            # (weak reference to the input, logits?, mask?) of the last forward: debug_tensor re-runs it with
                                     # private buffers.  Weak: a production call must not pin the caller's batch in HBM.
        self._ran = False            # a forward has run on this handle (distinguishes "no forward yet" from "its input is gone")
        self._ws_need = {}           # (B, H, W) -> workspace_bytes under the CURRENT mode / options / keep flag (cleared when those change)
        self._h = ctypes.c_void_p()
        d = _desc(arch)
        if blob is not None:
            blob = np.ascontiguousarray(blob, dtype=np.float32)
        ptr, n = (blob.ctypes.data, blob.size) if blob is not None else (None, 0)
        if arch.encoder == 'residual':
            if not hasattr(self.lib, 'ts2d_engine_create_residual'):
                raise RuntimeError(f"{_lib.LIB_PATH} was built before ts2d_engine_create_residual: rebuild it to run a ResidualEncoderUNet")
            r = _residual_desc(arch)
            _lib.check(self.lib.ts2d_engine_create_residual(ctypes.byref(d), ctypes.byref(r), ptr, n, self.device, ctypes.byref(self._h)),
                       'ts2d_engine_create_residual')
        else:
            _lib.check(self.lib.ts2d_engine_create(ctypes.byref(d), ptr, n, self.device, ctypes.byref(self._h)), 'ts2d_engine_create')
        for k, v in {**Engine.default_options, **(options or {})}.items():
            self.set_option(k, v)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self.lib.ts2d_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ weights
    def load_weights(self, blob: np.ndarray):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        _lib.check(self.lib.ts2d_engine_load_weights(self._h, blob.ctypes.data, blob.size), 'ts2d_engine_load_weights')

    def weight_buffer(self) -> Tuple[int, int]:
        """(device pointer, bytes) of the packed weight arena - the RCCL broadcast payload."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _lib.check(self.lib.ts2d_engine_weight_buffer(self._h, ctypes.byref(p), ctypes.byref(n)), 'ts2d_engine_weight_buffer')
        return int(p.value), int(n.value)

    def weights_ready(self):
        _lib.check(self.lib.ts2d_engine_weights_ready(self._h), 'ts2d_engine_weights_ready')

    def set_precision(self, mode):
        """'exact' (fp32 MFMA), 'split' (fp16 hi/lo x3 MFMA, fp32-equivalent accuracy; the default) or 'f16' (fp16 storage,
        one fp16 MFMA product, fp32 accumulate/statistics: BASELINE configs 3/5, outside the fp32 parity tolerance).  A residual-encoder
        engine refuses 'f16' (RuntimeError naming the mode) and keeps the mode it had, unless its option ``'resf16'`` is set
        (:func:`set_precision_opted_in` does both)."""
        m = {'exact': _lib.PRECISION_F32_EXACT, 'split': _lib.PRECISION_F32_SPLIT_F16X3, 'f16': _lib.PRECISION_F16}.get(mode, mode)
        _lib.check(self.lib.ts2d_engine_set_precision(self._h, int(m)), 'ts2d_engine_set_precision')
        self._ws_need.clear()

    def set_option(self, name: str, value: int):
        """Kernel-dispatch option of this handle (C-ABI ts2d_engine_set_option, include/ts2d_engine.h lists the names): picks
        between two parity-tested kernels for the ops it names; takes effect at the next forward."""
        _lib.check(self.lib.ts2d_engine_set_option(self._h, name.encode(), int(value)), f'ts2d_engine_set_option({name})')
        self._ws_need.clear()

    def set_tile_dtype(self, mode):
        """Blend order of :meth:`predict_tiled`: 'float' (reference CPU path: fp32 tile, one rounding into the half buffer;
        the default) or 'half' (CUDA autocast path: half tile, half product, half sum)."""
        m = {'float': 0, 'half': 1}.get(mode, mode)
        _lib.check(self.lib.ts2d_engine_set_tile_dtype(self._h, int(m)), 'ts2d_engine_set_tile_dtype')

    def keep_activations(self, on: bool = True):
        """One buffer per activation (C-ABI ts2d_engine_set_keep_activations) instead of liveness-based sharing; needed to read
        intermediate tensors back with :meth:`debug_tensor` (which switches it on itself and re-runs the last forward)."""
        _lib.check(self.lib.ts2d_engine_set_keep_activations(self._h, int(bool(on))), 'ts2d_engine_set_keep_activations')
        self._ws_need.clear()
        self._keep = bool(on)
        self._auto_keep = False

    # ------------------------------------------------------------------ forward
    def reserve(self, B: int, H: int, W: int):
        _lib.check(self.lib.ts2d_engine_reserve(self._h, B, H, W), 'ts2d_engine_reserve')

    def workspace_bytes(self, B: int, H: int, W: int) -> int:
        """Bytes of activation workspace :meth:`reserve` would allocate for (B, H, W) in the current precision mode.
        (The C-ABI call re-plans every op; the answer is remembered until the mode, an option or the keep flag changes -
        ``SubModelSet.forward_masks`` asks before every run.)"""
        key = (int(B), int(H), int(W))
        if key not in self._ws_need:
            n = ctypes.c_size_t()
            _lib.check(self.lib.ts2d_engine_workspace_bytes(self._h, B, H, W, ctypes.byref(n)), 'ts2d_engine_workspace_bytes')
            self._ws_need[key] = int(n.value)
        return self._ws_need[key]

    def set_workspace(self, dev_ptr: Optional[int], n_bytes: int = 0):
        """Run inside caller-owned device memory (C-ABI ts2d_engine_set_workspace; None: back to the engine's own allocation).
        Engines sharing one workspace must be driven on one stream."""
        _lib.check(self.lib.ts2d_engine_set_workspace(self._h, ctypes.c_void_p(dev_ptr) if dev_ptr else None, int(n_bytes)),
                   'ts2d_engine_set_workspace')

    def forward(self, x, logits=True, mask=False, out_logits=None, out_mask=None, stream: int = 0, _debug_rerun: bool = False):
        """x: [B,C,H,W] fp32, numpy (host) or torch CUDA tensor (device, zero-copy).
        Returns (logits or None, packed mask or None) of the same kind as x."""
        K = self.arch.num_classes
        if self._auto_keep and not _debug_rerun:      # debug_tensor left private buffers behind: a production call returns to the shared arena
            _lib.check(self.lib.ts2d_engine_set_keep_activations(self._h, 0), 'ts2d_engine_set_keep_activations')
            self._ws_need.clear()
            self._auto_keep = False
        self._ran = True
        try:
            self._last = (weakref.ref(x), logits, mask)
        except TypeError:
            self._last = None
        if _is_torch(x):
            import torch
            if not x.is_cuda:
                raise RuntimeError("torch input must live on the GPU (pass numpy for host data)")
            x = x.contiguous()
            if x.dtype != torch.float32:
                raise RuntimeError(f"input must be float32, found {x.dtype}")
            B, C, H, W = x.shape
            self._check_shape(C, W, mask)
            if logits and out_logits is None:
                out_logits = torch.empty((B, K, H, W), dtype=torch.float32, device=x.device)
            if mask and out_mask is None:
                out_mask = torch.empty((B, K, H, W // 32), dtype=torch.int32, device=x.device)
            side = None
            if stream == 0:
                # Order the kernels with the caller's torch work.  A non-default current stream is used directly; torch's DEFAULT
                # stream has the null handle, which the C-ABI reads as "the engine's own stream" - so run on a side stream that
                # waits for the current stream and make the current stream wait for it afterwards (no host synchronisation).
                cur = torch.cuda.current_stream(x.device)
                if cur.cuda_stream != 0:
                    stream = cur.cuda_stream
                else:
                    if getattr(self, '_side_stream', None) is None:
                        self._side_stream = torch.cuda.Stream(device=x.device)
                    side = self._side_stream
                    side.wait_stream(cur)
                    stream = side.cuda_stream
                    for t in (x, out_logits if logits else None, out_mask if mask else None):
                        if t is not None:
                            t.record_stream(side)
            _lib.check(self.lib.ts2d_engine_forward(
                self._h, x.data_ptr(), B, H, W, out_logits.data_ptr() if logits else None,
                out_mask.data_ptr() if mask else None, 1, ctypes.c_void_p(stream)), 'ts2d_engine_forward')
            if side is not None:
                torch.cuda.current_stream(x.device).wait_stream(side)
            return (out_logits if logits else None), (out_mask if mask else None)
        x = np.ascontiguousarray(x, dtype=np.float32)
        B, C, H, W = x.shape
        self._check_shape(C, W, mask)
        if logits and out_logits is None:
            out_logits = np.empty((B, K, H, W), dtype=np.float32)
        if mask and out_mask is None:
            out_mask = np.empty((B, K, H, W // 32), dtype=np.uint32)
        _lib.check(self.lib.ts2d_engine_forward(
            self._h, x.ctypes.data, B, H, W, out_logits.ctypes.data if logits else None,
            out_mask.ctypes.data if mask else None, 0, None), 'ts2d_engine_forward')
        return (out_logits if logits else None), (out_mask if mask else None)

    def check(self):
        """Synchronise the last forward and raise RuntimeError if it produced inf / NaN logits, naming the first layer whose
        output is non-finite (C-ABI ts2d_engine_check).  numpy forwards and predict_tiled run it themselves."""
        _lib.check(self.lib.ts2d_engine_check(self._h), 'ts2d_engine_check')

    def predict_tiled(self, image: np.ndarray, patch, tiles, mirror_axes=None, gaussian: Optional[np.ndarray] = None,
                      want_logits: bool = True, want_seg: bool = False):
        """Device-side sliding window for one padded 2-D image [C,Hp,Wp] (C-ABI ts2d_engine_predict_tiled).
        tiles: [(y, x), ...] in upstream order; gaussian: float16 [ph,pw] or None.  Returns (float16 [K,Hp,Wp] or None,
        uint8 [K,Hp,Wp] or None)."""
        desc, _, mask, g, keep, outs = self._tiled_args(None, [image], [tiles], None, mirror_axes, gaussian, False, False, want_logits, want_seg)
        d = desc[0]                  # (the one entry without descriptors: it makes its own call, _tiled_call serves the others)
        _lib.check(self.lib.ts2d_engine_predict_tiled(self._h, d.image, d.Hp, d.Wp, int(patch[0]), int(patch[1]), d.n_tiles, d.tile_y, d.tile_x,
                                                      mask, g, d.logits_f16, d.seg_u8), 'ts2d_engine_predict_tiled')
        _read_tiled_inf([self], None, 0, engine_flags=True)                          # upstream's inf check, done on the device
        del keep
        return (outs[2][0] if want_logits else None), (outs[3][0] if want_seg else None)

    def predict_tiled_batch(self, images, patch, tiles, mirror_axes=None, gaussian: Optional[np.ndarray] = None,
                            want_logits: bool = True, want_seg: bool = False):
        """Device-side sliding window for N padded 2-D images as ONE engine batch (C-ABI ts2d_engine_predict_tiled_batch).
        images: list of [C,Hp,Wp] arrays (extents may differ); tiles: one [(y, x), ...] list per image, upstream order.  Patch, mirror
        axes and gaussian are shared.  Returns (list of float16 [K,Hp,Wp] or None, list of uint8 [K,Hp,Wp] or None).
        The network takes the full-batch dispatch whatever the batch: an image's bytes do not depend on its batch-mates, its position
        or the batch size, and equal :meth:`predict_tiled` on an engine with ``options={'sbk': 0}`` bit for bit.
        Sets ``last_tiled_inf`` (the OR over the images) and ``last_tiled_inf_per_image``."""
        outs = _tiled_call('predict_tiled_batch', 'ts2d_engine_predict_tiled_batch', [self], False, images, patch, tiles, None, mirror_axes, gaussian,
                           (False, False, want_logits, want_seg), spell=lambda desc, n, common, keep: (desc, n) + common)
        return outs[2], outs[3]

    def predict_tiled_export(self, images, patch, tiles, exports, mirror_axes=None, gaussian: Optional[np.ndarray] = None,
                             want_seg: bool = True, want_f32: bool = False, want_logits: bool = False, want_padded_seg: bool = False,
                             full_batch: bool = True):
        """:meth:`predict_tiled_batch` followed, on the device, by the export's order-1 resample-back and threshold (C-ABI
        ts2d_engine_predict_tiled_export).  exports: one ``(src_y, src_x, src_h, src_w, out_h, out_w)`` per image - the rectangle of the
        padded prediction that is the case, and the extent it is resampled to.  Returns ``(seg, f32, logits, padded_seg)``: lists of
        uint8 [K,out_h,out_w] (``float32(value) > 1.5 * 2^-24`` of the resampled logits), float32 [K,out_h,out_w] (those logits),
        float16 [K,Hp,Wp] and uint8 [K,Hp,Wp] (what :meth:`predict_tiled_batch` returns), each None unless asked for.
        ``full_batch``: the full-batch dispatch of :meth:`predict_tiled_batch` (an image's bytes do not depend on its batch-mates);
        False: the size-dependent dispatch of :meth:`predict_tiled`.  The resampled values equal
        ``preprocess.resize_linear_f64`` of the float16 logits bit for bit.  Sets ``last_tiled_inf`` / ``last_tiled_inf_per_image``."""
        return _tiled_call('predict_tiled_export', 'ts2d_engine_predict_tiled_export', [self], False, images, patch, tiles, exports, mirror_axes,
                           gaussian, (want_seg, want_f32, want_logits, want_padded_seg), full_batch=full_batch)

    def _tiled_args(self, what, images, tiles, exports, mirror_axes, gaussian, want_seg, want_f32, want_logits, want_padded_seg, kind: str = 'export'):
        """Argument preparation of every tiled call (`what` names the calling method in a message): the ``TiledImage`` array, the
        descriptor array of the tail ``kind`` (``_TAILS``; None without ``exports``: no resample-back), the mirror mask, the address of the
        half gaussian (or None), the arrays all of these point into - they must outlive the call - and the output lists ``(seg, f32,
        logits, padded_seg)`` the call fills, each None unless asked for.  ``seg`` / ``f32`` are the uint8 / float32 output of the kind:
        'export' [K,out_h,out_w] both; 'labelmap' ONE uint8 plane [out_h,out_w], the label map; 'probabilities' (``exports`` of ten
        numbers: the six, then ``full_h, full_w, box_y, box_x``) the float32 probabilities [K,full_h,full_w] and the decided uint8 map
        [full_h,full_w] - [K,full_h,full_w] of 'probabilities_multilabel'.  'runs': the outputs are described apart from the images
        (:func:`predict_tiled_probabilities_stack_ensemble`): no ``exports``, and no output of these lists need be asked for.
        ``what`` None is the one image of :meth:`predict_tiled`: its messages carry no ``image i: `` and everything but the channel
        count is left to the library (or to the unpacking of the shape) to refuse."""
        struct, u8_field, f32_field, u8_heads, full_extent = _TAILS[kind]
        one = what is None
        if len(images) != len(tiles) or (exports is not None and len(exports) != len(images)):
            raise RuntimeError(f"{len(images)} images but {len(tiles)} tile lists" + ("" if exports is None else f" and {len(exports)} exports"))
        if exports is None:
            if want_seg or want_f32:
                raise RuntimeError(f"{what}: the resampled outputs need exports")
            if not (want_logits or want_padded_seg or one or kind == 'runs'):
                raise RuntimeError(f"{what}: neither logits nor segmentation requested")
        elif not (want_seg or want_f32):
            raise RuntimeError(f"{what}: neither the resampled segmentation nor the resampled logits requested")
        K = self.arch.num_classes
        keep = []                    # every array the descriptors point into stays alive until the call returns
        n = max(len(images), 1)
        desc, exd = (_lib.TiledImage * n)(), (None if exports is None else (struct * n)())
        seg, f32, out16, pseg = [], [], [], []
        for i, (image, tl) in enumerate(zip(images, tiles)):
            at = '' if one else f'image {i}: '
            image = np.ascontiguousarray(image, dtype=np.float32)
            if image.ndim != 3 and not one:
                raise RuntimeError(f"{at}expected [C,Hp,Wp], found shape {image.shape}")
            C, Hp, Wp = image.shape
            if C != self.arch.input_channels:
                raise RuntimeError(f"{at}input has {C} channels, the model expects {self.arch.input_channels}")
            ty = np.ascontiguousarray([t[0] for t in tl], dtype=np.int32)
            tx = np.ascontiguousarray([t[1] for t in tl], dtype=np.int32)
            out16.append(np.empty((K, Hp, Wp), dtype=np.float16) if want_logits else None)
            pseg.append(np.empty((K, Hp, Wp), dtype=np.uint8) if want_padded_seg else None)
            keep += [image, ty, tx]
            d = desc[i]
            d.image, d.Hp, d.Wp, d.n_tiles = image.ctypes.data, Hp, Wp, len(tl)
            d.tile_y, d.tile_x = ty.ctypes.data, tx.ctypes.data
            d.logits_f16 = out16[i].ctypes.data if want_logits else None
            d.seg_u8 = pseg[i].ctypes.data if want_padded_seg else None
            if exports is None:
                continue
            x = exd[i]
            x.src_y, x.src_x, x.src_h, x.src_w, x.out_h, x.out_w = six = tuple(int(v) for v in exports[i][:6])
            extent = six[4:]
            if full_extent:
                x.full_h, x.full_w, x.box_y, x.box_x = four = tuple(int(v) for v in exports[i][6:])
                extent = four[:2]
            extent = tuple(max(v, 0) for v in extent)                              # (a bad extent is the library's to reject, by name)
            seg.append(np.empty(((K,) if u8_heads else ()) + extent, dtype=np.uint8) if want_seg else None)
            f32.append(np.empty((K,) + extent, dtype=np.float32) if want_f32 else None)
            setattr(x, u8_field, seg[i].ctypes.data if want_seg else None)
            if f32_field:
                setattr(x, f32_field, f32[i].ctypes.data if want_f32 else None)
        mask = 0
        for a in (mirror_axes or ()):
            mask |= 1 << int(a)
        g = None if gaussian is None else np.ascontiguousarray(gaussian, dtype=np.float16)
        keep.append(g)
        outs = (seg if want_seg else None), (f32 if want_f32 else None), (out16 if want_logits else None), (pseg if want_padded_seg else None)
        return desc, exd, mask, (None if g is None else g.ctypes.data), keep, outs

    def _check_shape(self, C, W, mask):
        if C != self.arch.input_channels:
            raise RuntimeError(f"input has {C} channels, the model expects {self.arch.input_channels}")
        if mask and W % 32:
            raise RuntimeError("packed mask output needs W % 32 == 0")

    # ------------------------------------------------------------------ profiling
    def set_profiling(self, on: bool):
        _lib.check(self.lib.ts2d_engine_set_profiling(self._h, int(on)), 'ts2d_engine_set_profiling')

    def op_times(self) -> Dict[str, float]:
        """ms per launch of the LAST forward (HIP events on the launch stream), program order."""
        n = self.lib.ts2d_engine_num_ops(self._h)
        ms = (ctypes.c_float * max(n, 1))()
        _lib.check(self.lib.ts2d_engine_op_times(self._h, ms, n), 'ts2d_engine_op_times')
        return {self.lib.ts2d_engine_op_name(self._h, i).decode(): float(ms[i]) for i in range(n)}

    def op_kernels(self) -> dict:
        """op name -> name of the kernel that served it in the last profiled forward."""
        n = self.lib.ts2d_engine_num_ops(self._h)
        return {self.lib.ts2d_engine_op_name(self._h, i).decode(): self.lib.ts2d_engine_op_kernel(self._h, i).decode() for i in range(n)}

    def op_ksplit(self) -> dict:
        """op name -> split-K factor it ran with in the last profiled forward (1: no split; an op composed into its consumer has no entry)."""
        n = self.lib.ts2d_engine_num_ops(self._h)
        return {self.lib.ts2d_engine_op_name(self._h, i).decode(): int(self.lib.ts2d_engine_op_ksplit(self._h, i)) for i in range(n)}

    def debug_tensor(self, name: str, capacity: int = 1 << 26) -> np.ndarray:
        """Test accessor: activation `name` of the last forward as torch would hold it (NCHW, norm+act applied).  Activations
        share buffers by liveness: the first call switches the engine to private buffers and runs the last forward again - on the
        SAME input object, which the engine holds only weakly: keep a reference to the array / tensor you passed to forward()
        (``e.forward(x[None])`` or ``e.forward(a.astype(np.float32))`` leave nothing to re-run), or call ``keep_activations(True)``
        before the forward.  With the first block fused into the second (split mode) ``enc0.c0`` is not materialised: create the
        engine with ``options={'fuse0': 0}`` to read it."""
        if not (self._keep or self._auto_keep):
            if not self._ran:
                raise RuntimeError("debug_tensor: no forward has run on this engine")
            x = self._last[0]() if self._last is not None else None
            if x is None:
                raise RuntimeError("debug_tensor: the input of the last forward has been garbage-collected (the engine holds it weakly so "
                                   "that a production call does not pin the batch): keep a reference to the object passed to forward(), "
                                   "or call keep_activations(True) before the forward")
            _lib.check(self.lib.ts2d_engine_set_keep_activations(self._h, 1), 'ts2d_engine_set_keep_activations')
            self._ws_need.clear()
            self._auto_keep = True
            self.forward(x, logits=self._last[1], mask=self._last[2], _debug_rerun=True)
            if _is_torch(x):
                import torch
                torch.cuda.synchronize(x.device)
        out = np.empty(capacity, dtype=np.float32)
        dims = (ctypes.c_int32 * 4)()
        _lib.check(self.lib.ts2d_engine_debug_tensor(self._h, name.encode(), out.ctypes.data, out.size, ctypes.byref(dims)),
                   'ts2d_engine_debug_tensor')
        shp = tuple(int(d) for d in dims)
        return out[:int(np.prod(shp))].reshape(shp).copy()

    def materialised(self, name: str) -> bool:
        """Test accessor: False if the last forward composed the op that produces `name` into its consumer (a transposed conv
        folded into the next block, ``csrc/kernels_upc.h``; the first block recomputed inside the second), so that the tensor was
        never written.  Like :meth:`debug_tensor` it re-runs the last forward: keep a reference to its input."""
        try:
            self.debug_tensor(name)
            return True
        except RuntimeError as ex:
            if 'not materialised' in str(ex):
                return False
            raise

    def device_bytes(self) -> int:
        return int(self.lib.ts2d_engine_device_bytes(self._h))


# The tails of a tiled call by kind: the descriptor struct of an image (None: none), its uint8 and its float32 output field, whether the uint8
# output has the K heads in front (the float32 one always has), whether both are of the full extent (the descriptor then has ten numbers).
_TAILS = {'export': (_lib.TiledExport, 'seg_u8', 'logits_f32', True, False),
          'labelmap': (_lib.TiledLabelmap, 'label_u8', None, False, False),
          'probabilities': (_lib.TiledProbabilities, 'decided_u8', 'prob_f32', False, True),
          'probabilities_multilabel': (_lib.TiledProbabilities, 'decided_u8', 'prob_f32', True, True),
          'runs': (None, None, None, False, False)}


def _tiled_call(what, name, engines, ensemble: bool, images, patch, tiles, exports, mirror_axes, gaussian, wants, kind: str = 'export',
                full_batch=None, need: Optional[str] = None, extra=None, spell=None):
    """THE call of every tiled entry ``name`` that takes descriptors, for the method ``what``: the engines check, what the method needs of ``exports`` (``need``: the
    words of the refusal where they are None), its trailing arguments (``extra()`` -> ``(arguments, what they point into)``), the entry,
    :meth:`Engine._tiled_args` with ``wants = (seg, f32, logits, padded_seg)`` and ``kind``, the fold handles of an ``ensemble`` entry (else the
    one engine's), the call, the inf flags and the keep-alive.  The arguments between the handles and the trailing ones are ``desc, exd, n, ph, pw,
    mask, g`` and ``full_batch`` unless None, or what ``spell(desc, n, (ph, pw, mask, g), keep)`` returns.  Returns the four output lists."""
    engines = list(engines)
    if not engines:
        raise RuntimeError(f"{what}: no engines")
    if need is not None and exports is None:
        raise RuntimeError(f"{what}: {need}")
    tail, keep_tail = extra() if extra else ((), None)
    fn = _entry(name, engines[0].lib)
    desc, exd, mask, g, keep, outs = engines[0]._tiled_args(what, images, tiles, exports, mirror_axes, gaussian, *wants, kind=kind)
    n, common = len(images), (int(patch[0]), int(patch[1]), mask, g)
    head = ((ctypes.c_void_p * len(engines))(*[e._h for e in engines]), len(engines)) if ensemble else (engines[0]._h,)
    args = spell(desc, n, common, keep) if spell else (desc, exd, n) + common + (() if full_batch is None else (int(bool(full_batch)),))
    _lib.check(fn(*head, *args, *tail), name)
    _read_tiled_inf(engines, desc, n, engine_flags=ensemble)
    del keep, keep_tail
    return outs


def _order_args(order):
    """The trailing ``class_order, n_order`` of an entry -> ``(arguments, the array they point into)``."""
    return ((None, 0) if order is None else (order.ctypes.data, int(order.size))), order


def _from_logits(kind, logits_f16, rect, out_hw, device, class_order=None, prob=None):
    """The marshalling of the three ``<kind>_from_logits`` wrappers (C-ABI ``ts2d_<kind>_from_logits``), ``kind`` 'labelmap', 'regions' (with its
    ``class_order``) or 'probabilities' (with ``prob = (mode, full_hw, box_yx, want_decided)``, and the ``class_order`` of its regions mode).
    Returns the label map, or ``(probabilities, decided)``."""
    what = kind + '_from_logits'
    lg = np.ascontiguousarray(logits_f16, dtype=np.float16)
    if lg.ndim != 3:
        raise RuntimeError(f"expected [K,H,W], found shape {lg.shape}")
    K, code, order = lg.shape[0], None, None
    if prob is not None:
        code, order = _prob_mode(prob[0], class_order, what)
    elif kind == 'regions':
        order = _class_order_u8(class_order, what)
    if order is not None and order.size != K:
        raise RuntimeError(f"{what}: {order.size} class values for {K} heads")
    oh, ow = (int(v) for v in out_hw)
    if prob is None:
        out = result = np.empty((max(oh, 0), max(ow, 0)), dtype=np.uint8)
        tail = (() if order is None else (order.ctypes.data,)) + (out.ctypes.data,)
    else:
        fh, fw = (int(v) for v in prob[1])
        by, bx = (int(v) for v in prob[2])
        full = (max(fh, 0), max(fw, 0))
        out = np.empty((K,) + full, dtype=np.float32)
        dec = np.empty(((K,) if code == _lib.PROB_MULTILABEL else ()) + full, dtype=np.uint8) if prob[3] else None
        tail = (fh, fw, by, bx, code, None if order is None else order.ctypes.data, out.ctypes.data, None if dec is None else dec.ctypes.data)
        result = (out, dec)
    r = (ctypes.c_int32 * 4)(*[int(v) for v in rect])
    _lib.check(_entry('ts2d_' + what)(int(device), lg.ctypes.data, K, lg.shape[1], lg.shape[2], ctypes.byref(r), oh, ow, *tail), 'ts2d_' + what)
    return result


def predict_tiled_export_ensemble(engines, images, patch, tiles, exports, mirror_axes=None, gaussian: Optional[np.ndarray] = None,
                                  want_seg: bool = True, want_f32: bool = False, want_logits: bool = False, want_padded_seg: bool = False,
                                  full_batch: bool = True):
    """:meth:`Engine.predict_tiled_export` for a fold ensemble (C-ABI ts2d_ensemble_predict_tiled_export): ``engines`` are the folds, in
    fold order; each runs the sliding window that method runs, the device takes the mean of their float16 logits (upstream's
    ``prediction += fold; prediction /= n`` bit for bit - :func:`predictor.fold_mean_f16` is the statement in numpy) and every output is
    that of the mean.  Same arguments and the same ``(seg, f32, logits, padded_seg)`` as there; ``exports`` may be None (no
    resample-back: ``want_seg`` / ``want_f32`` must be off and ``want_logits`` or ``want_padded_seg`` on).  One engine: that method's
    bytes.  Sets ``last_tiled_inf_per_image`` on the first engine (per image the OR over the folds: upstream checks every fold's
    array) and ``last_tiled_inf`` on every engine (that fold's own)."""
    return _tiled_call('predict_tiled_export_ensemble', 'ts2d_ensemble_predict_tiled_export', engines, True, images, patch, tiles, exports, mirror_axes,
                       gaussian, (want_seg, want_f32, want_logits, want_padded_seg), full_batch=full_batch)


def predict_tiled_labelmap_ensemble(engines, images, patch, tiles, rects, mirror_axes=None, gaussian: Optional[np.ndarray] = None,
                                    want_logits: bool = False, full_batch: bool = True):
    """:func:`predict_tiled_export_ensemble` for a LABEL-MAP model (C-ABI ts2d_ensemble_predict_tiled_labelmap): the same sliding window
    per fold and the same mean (one engine: no mean), then per image the resample-back of the half logits to its extent and the argmax
    over the heads on the device (csrc/kernels_labelmap.h).  rects: one ``(src_y, src_x, src_h, src_w, out_h, out_w)`` per image.
    Returns ``(labels, logits)``: lists of uint8 [out_h,out_w] - ``export.labelmap_statement`` of the half logits, byte for byte - and
    of float16 [K,Hp,Wp] (those logits; None unless asked for).  Sets the inf flags as :func:`predict_tiled_export_ensemble` does."""
    outs = _tiled_call('predict_tiled_labelmap_ensemble', 'ts2d_ensemble_predict_tiled_labelmap', engines, True, images, patch, tiles, rects, mirror_axes,
                       gaussian, (True, False, want_logits, False), 'labelmap', full_batch, need='the label maps need their rectangles and extents')
    return outs[0], outs[2]


def labelmap_from_logits(logits_f16: np.ndarray, rect, out_hw, device: int = 0) -> np.ndarray:
    """The label-map kernel on half planes of the caller's (C-ABI ts2d_labelmap_from_logits): float16 [K,H,W], ``rect = (y, x, h, w)``
    inside it, resampled to ``out_hw`` and decided over the heads -> uint8 [out_h,out_w] = ``export.labelmap_statement``."""
    return _from_logits('labelmap', logits_f16, rect, out_hw, device)


def _class_order_u8(class_order, what: str) -> np.ndarray:
    """The class-order table of a region-based model as the K bytes the library takes; a value outside uint8 is refused here."""
    order = [int(c) for c in class_order]
    if any(c < 0 or c > 255 for c in order):
        raise RuntimeError(f"{what}: a class value outside 0..255 does not fit the uint8 output plane: {order}")
    return np.array(order, dtype=np.uint8)


def predict_tiled_regions_ensemble(engines, images, patch, tiles, rects, class_order, mirror_axes=None, gaussian: Optional[np.ndarray] = None,
                                   want_logits: bool = False, full_batch: bool = True):
    """:func:`predict_tiled_labelmap_ensemble` for a REGION-BASED model (C-ABI ts2d_ensemble_predict_tiled_regions): the same sliding
    window per fold, the same mean, the same descriptors, then per image the resample-back of the half logits, the export's predicate
    ``sigmoid(float32 v) > 0.5`` per head and the painting in order on the device (csrc/kernels_regions.h).  ``class_order``: one class
    value (0..255) per head, ``regions_class_order`` of the model's ``dataset.json``.  Returns ``(labels, logits)``: lists of uint8
    [out_h,out_w] - ``export.regions_statement`` of the half logits, byte for byte - and of float16 [K,Hp,Wp] (None unless asked for)."""
    what = 'predict_tiled_regions_ensemble'
    outs = _tiled_call(what, 'ts2d_ensemble_predict_tiled_regions', engines, True, images, patch, tiles, rects, mirror_axes, gaussian,
                       (True, False, want_logits, False), 'labelmap', full_batch, need='the maps need their rectangles and extents',
                       extra=lambda: _order_args(_class_order_u8(class_order, what)))
    return outs[0], outs[2]


def regions_from_logits(logits_f16: np.ndarray, rect, out_hw, class_order, device: int = 0) -> np.ndarray:
    """The region kernel on half planes of the caller's (C-ABI ts2d_regions_from_logits): float16 [K,H,W], ``rect = (y, x, h, w)`` inside
    it, resampled to ``out_hw``, thresholded per head and painted in order -> uint8 [out_h,out_w] = ``export.regions_statement``."""
    return _from_logits('regions', logits_f16, rect, out_hw, device, class_order)


def _prob_mode(mode, class_order, what: str):
    """``mode`` of ``export.PROBABILITY_MODES`` -> (TS2D_PROB_*, the class-order bytes of a regions call or None)."""
    from .export import PROBABILITY_MODES
    if mode not in PROBABILITY_MODES:
        raise RuntimeError(f"{what}: mode must be one of {PROBABILITY_MODES}, found {mode!r}")
    if mode != 'regions':
        return PROBABILITY_MODES.index(mode), None
    if class_order is None:
        raise RuntimeError(f"{what}: the regions mode needs the class order")
    return _lib.PROB_REGIONS, _class_order_u8(class_order, what)


def has_entry(*names: str, tolerant: bool = True) -> bool:
    """Does the engine library have every one of these entries?  The ONE lookup behind the ``has_*`` / ``device_*`` probes of the package: a
    library built before an optional entry (``_lib.OPTIONAL``) still loads, and the callers keep the host route.  ``tolerant``: no library built,
    or one that does not load, is False too (else that is ``_lib.load``'s error)."""
    try:
        return all(hasattr(_lib.load(), n) for n in names)
    except Exception:
        if tolerant:
            return False
        raise


def _entry(name: str, lib=None):
    """The entry ``name`` of the library (``lib``: an engine's own handle of it), or the error that says what to do about a library without it."""
    lib = _lib.load() if lib is None else lib
    if not hasattr(lib, name):
        raise RuntimeError(f"{name}: this libts2d_engine.so was built before the entry; rebuild it, or keep the host route")
    return getattr(lib, name)


def has_probabilities() -> bool:
    """Does the loaded library have the probabilities entries?  (A library built before them still loads: the callers keep the host route.)"""
    return has_entry('ts2d_ensemble_predict_tiled_probabilities', tolerant=False)


def predict_tiled_probabilities_ensemble(engines, images, patch, tiles, rects, mode, class_order=None, mirror_axes=None,
                                         gaussian: Optional[np.ndarray] = None, want_decided: bool = True, want_logits: bool = False,
                                         full_batch: bool = True):
    """:func:`predict_tiled_labelmap_ensemble` with the export's PROBABILITIES (C-ABI ts2d_ensemble_predict_tiled_probabilities): the same
    sliding window per fold and the same mean, then per image ONE kernel (csrc/kernels_prob.h) that resamples the half logits back,
    applies the non-linearity of ``mode`` (``export.PROBABILITY_MODES``: sigmoid for 'multilabel' and 'regions', softmax for 'labelmap'),
    writes the planes of the pre-crop extent with the fill around the box and decides the model's map on the logits in the same pass.
    rects: one ``(src_y, src_x, src_h, src_w, out_h, out_w, full_h, full_w, box_y, box_x)`` per image; ``class_order``: the regions mode's.
    Returns ``(probabilities, decided, logits)``: lists of float32 [K,full_h,full_w] - ``export.probabilities_statement`` of the half
    logits to within a few float32 units - of uint8 [full_h,full_w] ([K,full_h,full_w] multilabel; None unless ``want_decided``) - inside
    the box byte for byte what the label-map / regions / threshold routes give, 0 outside - and of float16 [K,Hp,Wp] (None unless asked)."""
    what = 'predict_tiled_probabilities_ensemble'

    def extra():
        code, order = _prob_mode(mode, class_order, what)
        return (code,) + _order_args(order)[0], order
    outs = _tiled_call(what, 'ts2d_ensemble_predict_tiled_probabilities', engines, True, images, patch, tiles, rects, mirror_axes, gaussian,
                       (bool(want_decided), True, want_logits, False), 'probabilities_multilabel' if mode == 'multilabel' else 'probabilities',
                       full_batch, need='the probabilities need their rectangles and extents', extra=extra)
    return outs[1], outs[0], outs[2]


def has_stack_probabilities() -> bool:
    """Does the loaded library have the probabilities entry for slice stacks?  (One built before it still loads: the callers keep the host route.)"""
    return has_entry('ts2d_ensemble_predict_tiled_probabilities_stack', tolerant=False)


def predict_tiled_probabilities_stack_ensemble(engines, images, patch, tiles, runs, mode, class_order=None, mirror_axes=None,
                                               gaussian: Optional[np.ndarray] = None, want_logits: bool = False, full_batch: bool = True):
    """:func:`predict_tiled_probabilities_ensemble` for SLICE STACKS (C-ABI ts2d_ensemble_predict_tiled_probabilities_stack): the outputs are
    described per RUN - consecutive images that are consecutive slices of one volume and share one geometry - and are written IN PLACE into
    arrays of the caller's.  runs: one ``(first_image, n_slices, rect, prob, decided)`` each, covering the images once and in order;
    ``rect`` the ten numbers of that function; ``prob`` a float32 view [K, n_slices, full_h, full_w] of the caller's [K, Z0, full_h, full_w]
    (``volume[:, z:z + n_slices]``: any stride between the heads, dense below it); ``decided`` the like uint8 view, [K, n_slices, ...] of a
    multilabel model and [n_slices, ...] otherwise, or None.  Every slice gets the bytes the per-image function gives it.  Returns the list
    of float16 [K,Hp,Wp] logits (None unless ``want_logits``).  Sets the inf flags as :func:`predict_tiled_export_ensemble` does."""
    what = 'predict_tiled_probabilities_stack_ensemble'
    engines = list(engines)

    def extra():
        code, order = _prob_mode(mode, class_order, what)
        return (code,) + _order_args(order)[0], order

    def spell(desc, n_images, common, keep):           # the run descriptors go between the images and the patch
        K = engines[0].arch.num_classes
        rd = (_lib.TiledProbabilitiesRun * max(len(runs), 1))()
        for r, (first, n, rect, prob, dec) in enumerate(runs):
            x = rd[r]
            (x.src_y, x.src_x, x.src_h, x.src_w, x.out_h, x.out_w, x.full_h, x.full_w, x.box_y, x.box_x) = (int(v) for v in rect)
            x.first_image, x.n_slices = int(first), int(n)
            for name, a, dt, heads in (('prob', prob, np.float32, True), ('decided', dec, np.uint8, mode == 'multilabel')):
                if a is None and name == 'decided':
                    continue
                tail = (int(n), max(x.full_h, 0), max(x.full_w, 0))              # (a bad extent is the library's to reject, by name)
                if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != ((K,) if heads else ()) + tail or not a.flags.writeable \
                        or not a[0 if heads else slice(None)].flags.c_contiguous or (heads and a.strides[0] % a.itemsize):
                    raise RuntimeError(f"{what}: run {r}: {name} must be a writeable {np.dtype(dt).name} view {((K,) if heads else ()) + tail}, dense below the heads")
                stride = a.strides[0] // a.itemsize if heads else 0
                if name == 'prob':
                    x.prob_f32, x.prob_head_stride = a.ctypes.data, stride
                else:
                    x.decided_u8, x.decided_head_stride = a.ctypes.data, stride
                keep.append(a)
        keep.append(rd)
        return (desc, n_images, rd, len(runs)) + common + (int(bool(full_batch)),)
    return _tiled_call(what, 'ts2d_ensemble_predict_tiled_probabilities_stack', engines, True, images, patch, tiles, None, mirror_axes, gaussian,
                       (False, False, want_logits, False), 'runs', extra=extra, spell=spell)[2]


def probabilities_from_logits(logits_f16: np.ndarray, rect, out_hw, full_hw, box_yx, mode, class_order=None, want_decided: bool = True,
                              device: int = 0):
    """The probabilities kernel on half planes of the caller's (C-ABI ts2d_probabilities_from_logits): float16 [K,H,W], ``rect = (y, x, h, w)``
    inside it, resampled to ``out_hw``, placed at ``box_yx`` of ``full_hw`` -> ``(float32 [K,full_h,full_w], decided uint8 or None)``."""
    return _from_logits('probabilities', logits_f16, rect, out_hw, device, class_order, (mode, full_hw, box_yx, want_decided))


def has_keep_largest_components() -> bool:
    """Does the engine library have ``ts2d_keep_largest_components``?  False with no library built, one that does not load, or one built
    before the entry: the callers keep the host route (postprocess.apply_postprocessing)."""
    return has_entry('ts2d_keep_largest_components')


def keep_largest_components(seg: np.ndarray, tables, backgrounds, device: int = 0):
    """nnU-Net's largest-component postprocessing on the device (C-ABI ts2d_keep_largest_components, csrc/kernels_post_cc.h): uint8
    [Z,H,W] (or [H,W]: Z = 1), per step a 256-byte membership table and a background byte (``PostprocessingPlan.compiled``).  Returns
    ``(seg_out, stats, status)``: a new array - ``postprocess.keep_largest_components_statement`` byte for byte - the int64
    [n_steps, 4] counters (mask voxels, components, largest size, voxels removed) and 0; or ``(None, None, CC_GIVE_UP)`` where a bounded
    loop of the labelling reached its cap: the caller takes the host route."""
    src = np.asarray(seg)
    if src.dtype != np.uint8 or src.ndim not in (2, 3):
        raise RuntimeError(f"keep_largest_components: expected uint8 [Z,H,W] or [H,W], found {src.dtype} {src.shape}")
    fn = _entry('ts2d_keep_largest_components')
    out = np.array(src, dtype=np.uint8, order='C')            # (a copy: the entry works in place)
    z, h, w = ((1,) + out.shape)[-3:]
    n = len(tables)
    steps = (_lib.CcStep * max(n, 1))()
    for k in range(n):
        t = np.ascontiguousarray(tables[k], dtype=np.uint8)
        if t.shape != (256,):
            raise RuntimeError(f"keep_largest_components: step {k}: the membership table has shape {t.shape}, not (256,)")
        ctypes.memmove(steps[k].member, t.ctypes.data, 256)
        steps[k].background = int(backgrounds[k])
    stats = np.zeros((n, 4), dtype=np.int64)
    status = ctypes.c_int(0)
    _lib.check(fn(int(device), out.ctypes.data, z, h, w, ctypes.cast(steps, ctypes.c_void_p), n, stats.ctypes.data,
                                                ctypes.byref(status)), 'ts2d_keep_largest_components')
    if status.value:
        return None, None, int(status.value)
    return out, stats, 0


def visual_labels(planes: np.ndarray, spacing_hw, palette: np.ndarray, out_hw, device: int = 0) -> np.ndarray:
    """The label visual on the device (C-ABI ts2d_visual_labels, csrc/kernels_visual.h): uint8 planes [K, H, W] (K = 1: a label map; K > 1:
    flattened to 1 + the index of the last non-zero plane), nearest resample to the smaller of ``spacing_hw``, colour ``palette[v % n]`` (uint8
    [n, 3]), 0 and outside black.  ``out_hw``: the output extents (``visual.uniform_extent`` per axis).  Returns uint8 [h, w, 3] -
    ``visual.label_rgb`` of the statement byte for byte."""
    src = np.ascontiguousarray(planes, dtype=np.uint8)
    pal = np.ascontiguousarray(palette, dtype=np.uint8)
    if src.ndim != 3 or pal.ndim != 2 or pal.shape[1] != 3:
        raise RuntimeError(f"visual_labels: expected uint8 planes [K,H,W] and a palette [n,3], found {src.shape} and {pal.shape}")
    k, h, w = src.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = np.empty((max(oh, 0), max(ow, 0), 3), np.uint8)
    _lib.check(_entry('ts2d_visual_labels')(int(device), src.ctypes.data, k, h, w, float(spacing_hw[0]), float(spacing_hw[1]), pal.ctypes.data,
                                                  pal.shape[0], oh, ow, out.ctypes.data), 'ts2d_visual_labels')
    return out


def visual_grey(plane: np.ndarray, spacing_hw, cubic: bool, lo, hi, out_hw, device: int = 0):
    """The grey visual on the device (C-ABI ts2d_visual_grey): one plane [H, W] of type uint8, int16, uint16, int32 or float32, nearest or
    order-3 resample to the smaller of ``spacing_hw``, window ``lo ... hi`` to 0 ... 255 (None: the minimum / maximum of the resampled plane).
    Returns ``(uint8 [h, w], (lo, hi) as used)`` - ``visual.window_u8`` of the statement byte for byte - or None where the entry set a status bit
    (a non-finite float32 sample): the caller takes the host route."""
    from .visual import DEVICE_DTYPES
    src = np.ascontiguousarray(plane)
    if src.ndim != 2 or src.dtype.name not in DEVICE_DTYPES:
        raise RuntimeError(f"visual_grey: expected a plane [H,W] of type {sorted(DEVICE_DTYPES)}, found {src.dtype} {src.shape}")
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = np.empty((max(oh, 0), max(ow, 0)), np.uint8)
    used = np.zeros(2, np.float64)
    status = ctypes.c_int(0)
    _lib.check(_entry('ts2d_visual_grey')(int(device), src.ctypes.data, DEVICE_DTYPES[src.dtype.name], src.shape[0], src.shape[1],
                                                float(spacing_hw[0]), float(spacing_hw[1]), 1 if cubic else 0, 0.0 if lo is None else float(lo),
                                                0.0 if hi is None else float(hi), int(lo is None), int(hi is None), oh, ow, out.ctypes.data,
                                                used.ctypes.data, ctypes.byref(status)), 'ts2d_visual_grey')
    if status.value:
        return None
    return out, (float(used[0]), float(used[1]))


def _label_side(who: str, seg: np.ndarray, kind: int, values, z: int, h: int, w: int):
    """``(values as uint8 or None, K)`` of the label side of a statistics call: C-contiguous uint8 planes [K, Z, H, W] or one label map
    [Z, H, W] with ``values`` [K]."""
    if seg.dtype != np.uint8 or not seg.flags['C_CONTIGUOUS']:
        raise RuntimeError(f"{who}: expected a C-contiguous uint8 segmentation, found {seg.dtype} {seg.shape}")
    if kind == _lib.STATS_LABELMAP:
        vals = np.ascontiguousarray(values, dtype=np.uint8)
        if seg.size != z * h * w:
            raise RuntimeError(f"{who}: a label map of {seg.size} samples for {z} x {h} x {w}")
        return vals, int(vals.size)
    k = int(seg.shape[0])
    if seg.size != k * z * h * w:
        raise RuntimeError(f"{who}: planes of {seg.size} samples for {k} x {z} x {h} x {w}")
    return None, k


def label_statistics(seg: np.ndarray, kind: int, values, shape_zhw, intensities: Optional[np.ndarray] = None, max_scratch_bytes: int = 0,
                     device: int = 0):
    """The per-label statistics on the device (C-ABI ts2d_label_statistics, csrc/kernels_stats.h).  ``seg``: C-contiguous uint8, planes
    [K, Z, H, W] (``kind`` = ``_lib.STATS_PLANES``) or one label map [Z, H, W] with ``values`` [K] (``_lib.STATS_LABELMAP``); ``intensities``:
    float32 [C, Z, H, W] or None.  Returns ``(int64 [K, 10], float64 [K, C, 6])`` in the layout of include/ts2d_engine.h - the statement's
    numbers bit for bit - or None where the entry set a status bit (a non-finite intensity under a label): the caller takes the host route."""
    fn = _entry('ts2d_label_statistics')
    z, h, w = (int(v) for v in shape_zhw)
    vals, k = _label_side('label_statistics', seg, kind, values, z, h, w)
    c = 0
    if intensities is not None:
        if intensities.dtype != np.float32 or not intensities.flags['C_CONTIGUOUS'] or intensities.size % (z * h * w):
            raise RuntimeError(f"label_statistics: expected C-contiguous float32 intensities [C, {z}, {h}, {w}], found {intensities.dtype} {intensities.shape}")
        c = intensities.size // (z * h * w)
    out_int = np.zeros((k, _lib.STATS_INTS), np.int64)
    out_f64 = np.zeros((k, c, _lib.STATS_F64S), np.float64)
    status = ctypes.c_int(0)
    _lib.check(fn(int(device), seg.ctypes.data, int(kind), vals.ctypes.data if vals is not None else None, k, z, h, w,
                                         intensities.ctypes.data if c else None, c, int(max_scratch_bytes), out_int.ctypes.data,
                                         out_f64.ctypes.data if c else None, ctypes.byref(status)), 'ts2d_label_statistics')
    if status.value:
        return None
    return out_int, out_f64


def label_percentiles(seg: np.ndarray, kind: int, values, shape_zhw, intensities: np.ndarray, percentiles, max_scratch_bytes: int = 0,
                      device: int = 0):
    """The samples under every label at the sorted positions of percentiles, on the device (C-ABI ts2d_label_percentiles,
    csrc/kernels_stats_select.h).  ``seg``, ``kind``, ``values``, ``shape_zhw``: as :func:`label_statistics`; ``intensities``: float32
    [C, Z, H, W], C >= 1; ``percentiles``: 1 ... 8 floats in 0 ... 100.  Returns ``(count int64 [K], rank_value float32 [K, C, P, 2],
    rank_weight float64 [K, P])`` - ``statistics.label_percentiles_statement``'s bit for bit - or None where the entry set a status bit (a
    non-finite intensity under a label): the caller takes the host route."""
    fn = _entry('ts2d_label_percentiles')
    z, h, w = (int(v) for v in shape_zhw)
    vals, k = _label_side('label_percentiles', seg, kind, values, z, h, w)
    if intensities is None or intensities.dtype != np.float32 or not intensities.flags['C_CONTIGUOUS'] or intensities.size % (z * h * w):
        raise RuntimeError(f"label_percentiles: expected C-contiguous float32 intensities [C, {z}, {h}, {w}]")
    c = intensities.size // (z * h * w)
    qs = np.ascontiguousarray(percentiles, dtype=np.float64).reshape(-1)
    p = int(qs.size)
    count = np.zeros(k, np.int64)
    rank_value = np.zeros((k, c, p, 2), np.float32)
    rank_weight = np.zeros((k, p), np.float64)
    status = ctypes.c_int(0)
    _lib.check(fn(int(device), seg.ctypes.data, int(kind), vals.ctypes.data if vals is not None else None, k, z, h, w, intensities.ctypes.data, c,
                  qs.ctypes.data, p, int(max_scratch_bytes), count.ctypes.data, rank_value.ctypes.data, rank_weight.ctypes.data,
                  ctypes.byref(status)), 'ts2d_label_percentiles')
    if status.value:
        return None
    return count, rank_value, rank_weight


COMPONENTS_FIRST_CAPACITY = 65536      # rows of the list on the first call of label_components; more components than that cost one more call


def components_state_bytes(shape_zhw) -> int:
    """The labelling state of ONE label of ``ts2d_label_components`` (of a whole label map): class, parent, count and the run words."""
    z, h, w = (int(v) for v in shape_zhw)
    return 9 * z * h * w + 8 * z * h * ((w + 63) // 64)


def statistics_chunk_labels(shape_zhw, n_labels: int, n_channels: int, max_scratch_bytes: int = 0):
    """``(labels per chunk, what set it)`` of ``ts2d_label_statistics`` (csrc/stats_plan.cpp: ``st_plan``, spelled again): ``'budget'`` - the row
    partials of a chunk, ``rows * (20 + 16 C)`` bytes a label, stay at or below ``max_scratch_bytes`` (0: 256 MiB); ``'slot_cap'`` - a channel
    partial's slot is an int32, so a chunk has at most ``(2^31 - 1) // (rows * max(C, 1))`` labels; ``'labels'`` - all K fit.  0 labels: the entry
    refuses."""
    z, h, _ = (int(v) for v in shape_zhw)
    rows, c = z * h, int(n_channels)
    by_budget = (int(max_scratch_bytes) or 256 << 20) // (rows * (20 + 16 * c))
    by_slots = (2 ** 31 - 1) // (rows * max(c, 1))
    return min((by_budget, 'budget'), (by_slots, 'slot_cap'), (int(n_labels), 'labels'), key=lambda t: t[0])


def percentiles_chunk_labels(shape_zhw, n_labels: int, n_channels: int, n_percentiles: int, max_scratch_bytes: int = 0):
    """:func:`statistics_chunk_labels` for ``ts2d_label_percentiles`` (``ls_plan``): a label's state is ``C * 2 P * 1040 + rows * 20`` bytes and
    the slot of a row partial, ``label * rows + row``, is an int32."""
    z, h, _ = (int(v) for v in shape_zhw)
    rows = z * h
    by_budget = (int(max_scratch_bytes) or 256 << 20) // (int(n_channels) * 2 * int(n_percentiles) * 1040 + rows * 20)
    return min((by_budget, 'budget'), ((2 ** 31 - 1) // rows, 'slot_cap'), (int(n_labels), 'labels'), key=lambda t: t[0])


def label_components(seg: np.ndarray, kind: int, values, shape_zhw, connectivity: int = 0, keep_largest: bool = False, min_voxels=None,
                     want_seg: bool = True, want_list: bool = True, max_scratch_bytes: int = 0, device: int = 0, capacity: Optional[int] = None):
    """The components of every label at once on the device (C-ABI ts2d_label_components, csrc/kernels_components.h).  ``seg``, ``kind``,
    ``values``, ``shape_zhw``: as :func:`label_statistics`; ``connectivity``: ``_lib.COMP_FULL`` or ``_lib.COMP_FACES``; ``min_voxels``: None
    or K non-negative integers.  Returns ``(cleaned or None, counters int64 [K, 5], components int64 [N, 3] or None)`` -
    ``components.label_components_statement``'s byte for byte - or None where the entry gave up (TS2D_COMP_GIVE_UP): the caller takes the host
    route.  The list is asked for with ``capacity`` rows (default :data:`COMPONENTS_FIRST_CAPACITY`); where there are more components the entry
    is called once more with their exact number, never a third time."""
    fn = _entry('ts2d_label_components')
    z, h, w = (int(v) for v in shape_zhw)
    vals, k = _label_side('label_components', seg, kind, values, z, h, w)
    mv = None
    if min_voxels is not None:
        mv = np.ascontiguousarray([min(int(v), 2 ** 63 - 1) for v in min_voxels], dtype=np.int64)
        if mv.shape != (k,):
            raise RuntimeError(f"label_components: min_voxels has {mv.size} entries for {k} labels")
    counters = np.zeros((k, _lib.COMP_COUNTERS), np.int64)
    cap = (COMPONENTS_FIRST_CAPACITY if capacity is None else int(capacity)) if want_list else 0
    for _ in range(2):
        out = np.empty_like(seg) if want_seg else None
        rows = np.zeros((cap, 3), np.int64) if want_list else None
        total = ctypes.c_int64(0)
        status = ctypes.c_int(0)
        _lib.check(fn(int(device), seg.ctypes.data, int(kind), vals.ctypes.data if vals is not None else None, k, z, h, w, int(connectivity),
                      int(bool(keep_largest)), mv.ctypes.data if mv is not None else None, int(max_scratch_bytes),
                      out.ctypes.data if want_seg else None, counters.ctypes.data, rows.ctypes.data if want_list else None, cap,
                      ctypes.byref(total), ctypes.byref(status)), 'ts2d_label_components')
        if status.value & _lib.COMP_GIVE_UP:
            return None
        if not want_list:
            return out, counters, None
        if not status.value & _lib.COMP_LIST_FULL:
            return out, counters, rows[:total.value].copy()
        cap = int(total.value)
    raise RuntimeError(f"ts2d_label_components: {total.value} components did not fit a list of as many rows")


def label_morphology(seg: np.ndarray, kind: int, values, shape_hw, spacing_hw, op: int, radius: float, select=None, max_scratch_bytes: int = 0,
                     device: int = 0):
    """Grow, shrink, open or close every label on the device (C-ABI ts2d_label_morphology, csrc/kernels_morph.h).  ``seg``: C-contiguous uint8,
    planes [K, H, W] (``kind`` = ``_lib.STATS_PLANES``) or one label map [H, W] with ``values`` [K] (``_lib.STATS_LABELMAP``); ``spacing_hw``:
    the spacings of a row step and a column step; ``op``: ``_lib.MORPH_*``; ``radius`` in the unit of the spacing; ``select``: None or K
    booleans.  Returns ``(out of the shape of seg, counters int64 [K, 4])`` - ``morphology.label_morphology_statement``'s byte for byte."""
    fn = _entry('ts2d_label_morphology')
    h, w = (int(v) for v in shape_hw)
    vals, k = _label_side('label_morphology', seg, kind, values, 1, h, w)
    sel = None
    if select is not None:
        sel = np.ascontiguousarray([1 if s else 0 for s in select], dtype=np.uint8)
        if sel.shape != (k,):
            raise RuntimeError(f"label_morphology: select has {sel.size} entries for {k} labels")
    out = np.empty_like(seg)
    counters = np.zeros((k, _lib.MORPH_COUNTERS), np.int64)
    _lib.check(fn(int(device), seg.ctypes.data, int(kind), vals.ctypes.data if vals is not None else None, k, h, w, float(spacing_hw[0]),
                  float(spacing_hw[1]), int(op), float(radius), sel.ctypes.data if sel is not None else None, int(max_scratch_bytes),
                  out.ctypes.data, counters.ctypes.data), 'ts2d_label_morphology')
    return out, counters


def project_labels_coronal(buffer: np.ndarray, extents, strides, base: int, num: int, device: int = 0):
    """The label projection on the device (C-ABI ts2d_project_labels_coronal, csrc/kernels_evaluate.h).  ``buffer``: the volume's C-contiguous
    integer samples; ``extents`` (nz, ny, nx), ``strides`` (sz, sy, sx) and ``base`` in elements: the reoriented view of
    ``image._coronal_view``.  Returns ``(uint8 [num, nz, nx], status)``; with a status bit (``_lib.LABELS_RANGE``) the planes are no result."""
    from .image import _GPU_DTYPES
    fn = _entry('ts2d_project_labels_coronal')
    if buffer.dtype.name not in _GPU_DTYPES or not np.issubdtype(buffer.dtype, np.integer) or not buffer.flags['C_CONTIGUOUS']:
        raise RuntimeError(f"project_labels_coronal: expected a C-contiguous int16, uint8, uint16 or int32 volume, found {buffer.dtype}")
    nz, ny, nx = (int(v) for v in extents)
    sz, sy, sx = (int(v) for v in strides)
    planes = np.zeros((int(num), nz, nx), np.uint8)
    status = np.zeros(1, np.int32)
    _lib.check(fn(int(device), buffer.ctypes.data, buffer.size, _GPU_DTYPES[buffer.dtype.name], nz, ny, nx, sz, sy, sx, int(base), int(num),
                  planes.ctypes.data, status.ctypes.data), 'ts2d_project_labels_coronal')
    return planes, int(status[0])


def _xr_args(what: str, buffer: np.ndarray, extents, strides, base: int, g: dict, device: int, integer: bool):
    """The view and the geometry of the two radiograph entries as their leading arguments.  ``g``: ``xray.XRGeometry.resolve``."""
    from .image import _GPU_DTYPES
    if buffer.dtype.name not in _GPU_DTYPES or (integer and not np.issubdtype(buffer.dtype, np.integer)) or not buffer.flags['C_CONTIGUOUS']:
        raise RuntimeError(f"{what}: expected a C-contiguous {'int16, uint8, uint16 or int32' if integer else 'int16, uint8, float32, uint16 or int32'} "
                           f"volume, found {buffer.dtype}")
    nz, ny, nx = (int(v) for v in extents)
    sz, sy, sx = (int(v) for v in strides)
    return [int(device), buffer.ctypes.data, buffer.size, _GPU_DTYPES[buffer.dtype.name], nz, ny, nx, sz, sy, sx, int(base),
            float(g['spacing'][0]), float(g['spacing'][1]), float(g['spacing'][2]), float(g['sdd']), float(g['sod']), int(g['pa']), int(g['parallel']),
            float(g['du']), float(g['dv']), int(g['nu']), int(g['nv'])]


def project_xr(buffer: np.ndarray, extents, strides, base: int, g: dict, device: int = 0, want_sum: bool = True, want_xr: bool = True):
    """The synthetic radiograph on the device (C-ABI ts2d_project_xr, csrc/kernels_project_xr.h).  ``buffer``, ``extents``, ``strides``, ``base``:
    the reoriented view of ``image._coronal_view``; ``g``: the resolved geometry (``xray.XRGeometry.resolve``).  Returns ``(float64 [nv, nu] sums or
    None, float32 [nv, nu] radiograph or None, status)``; with a status bit (``_lib.XR_NONFINITE``) the arrays are no result."""
    fn = _entry('ts2d_project_xr')
    args = _xr_args('project_xr', buffer, extents, strides, base, g, device, integer=False)
    nu, nv = int(g['nu']), int(g['nv'])
    out_sum = np.zeros((nv, nu), np.float64) if want_sum else None
    out_xr = np.zeros((nv, nu), np.float32) if want_xr else None
    status = np.zeros(1, np.int32)
    clip = g['density_max'] is not None
    _lib.check(fn(*args, float(g['air']), float(g['water']), int(clip), float(g['density_max']) if clip else 0.0,
                  out_sum.ctypes.data if want_sum else None, out_xr.ctypes.data if want_xr else None, status.ctypes.data), 'ts2d_project_xr')
    return out_sum, out_xr, int(status[0])


def project_labels_xr(buffer: np.ndarray, extents, strides, base: int, num: int, g: dict, device: int = 0):
    """The label projection along the radiograph's rays on the device (C-ABI ts2d_project_labels_xr).  Arguments as :func:`project_xr`.  Returns
    ``(uint8 [num, nv, nu], status)``; with a status bit (``_lib.LABELS_RANGE``) the planes are no result."""
    fn = _entry('ts2d_project_labels_xr')
    args = _xr_args('project_labels_xr', buffer, extents, strides, base, g, device, integer=True)
    planes = np.zeros((int(num), int(g['nv']), int(g['nu'])), np.uint8)
    status = np.zeros(1, np.int32)
    _lib.check(fn(*args, int(num), planes.ctypes.data, status.ctypes.data), 'ts2d_project_labels_xr')
    return planes, int(status[0])


def _evaluate_sides(what: str, a: np.ndarray, kind_a: int, b: np.ndarray, kind_b: int, values, n: int):
    """(K, values as uint8 or None) of the two sides of a scoring entry: C-contiguous uint8, planes [K, n samples] or one label map."""
    for x in (a, b):
        if x.dtype != np.uint8 or not x.flags['C_CONTIGUOUS']:
            raise RuntimeError(f"{what}: expected C-contiguous uint8 segmentations, found {x.dtype} {x.shape}")
    vals = None if values is None else np.ascontiguousarray(values, dtype=np.uint8)
    ks = [int(x.shape[0]) for x, kind in ((a, kind_a), (b, kind_b)) if kind == _lib.STATS_PLANES] + ([int(vals.size)] if vals is not None else [])
    if not ks or len(set(ks)) != 1:
        raise RuntimeError(f"{what}: the sides and the values differ in their number of labels: {ks}")
    for x, kind in ((a, kind_a), (b, kind_b)):
        if x.size != (ks[0] if kind == _lib.STATS_PLANES else 1) * n:
            raise RuntimeError(f"{what}: a segmentation of {x.size} samples for {ks[0] if kind == _lib.STATS_PLANES else 1} x {n}")
    return ks[0], vals


def label_overlap(a: np.ndarray, kind_a: int, b: np.ndarray, kind_b: int, values, shape_zhw, device: int = 0) -> np.ndarray:
    """The overlap counts on the device (C-ABI ts2d_label_overlap).  ``a``, ``b``: C-contiguous uint8, each planes [K, Z, H, W]
    (``_lib.STATS_PLANES``) or one label map [Z, H, W] with ``values`` [K] (``_lib.STATS_LABELMAP``).  Returns int64 [K, 3] = n_a, n_b, n_both."""
    fn = _entry('ts2d_label_overlap')
    z, h, w = (int(v) for v in shape_zhw)
    k, vals = _evaluate_sides('label_overlap', a, kind_a, b, kind_b, values, z * h * w)
    out = np.zeros((k, 3), np.int64)
    _lib.check(fn(int(device), a.ctypes.data, int(kind_a), b.ctypes.data, int(kind_b), vals.ctypes.data if vals is not None else None, k, z, h, w,
                  out.ctypes.data), 'ts2d_label_overlap')
    return out


def label_confusion(a: np.ndarray, kind_a: int, b: np.ndarray, kind_b: int, values, shape_zhw, device: int = 0) -> np.ndarray:
    """The confusion matrix on the device (C-ABI ts2d_label_confusion, csrc/kernels_confusion.h).  ``a``, ``b``, ``values`` as in
    :func:`label_overlap`; ``a`` and ``b`` may be the same array.  Returns int64 [K + 2, K + 2], row = side a, column = side b: row 0 "none of
    the labels", row 1 + k label k, row K + 1 every sample (``evaluate.confusion_statement``)."""
    fn = _entry('ts2d_label_confusion')
    z, h, w = (int(v) for v in shape_zhw)
    k, vals = _evaluate_sides('label_confusion', a, kind_a, b, kind_b, values, z * h * w)
    out = np.zeros((k + 2, k + 2), np.int64)
    _lib.check(fn(int(device), a.ctypes.data, int(kind_a), b.ctypes.data, int(kind_b), vals.ctypes.data if vals is not None else None, k, z, h, w,
                  out.ctypes.data), 'ts2d_label_confusion')
    return out


def _surface_call(what: str, a, kind_a, b, kind_b, values, shape_hw, spacing_hw, tol_sq, device):
    """What the two boundary-distance wrappers prepare alike for the entry ``ts2d_<what>``: ``(entry, its arguments up to T, K, out_i, out_f,
    the arrays those arguments point into)``."""
    fn = _entry('ts2d_' + what)
    h, w = (int(v) for v in shape_hw)
    k, vals = _evaluate_sides(what, a, kind_a, b, kind_b, values, h * w)
    tol = np.ascontiguousarray(tol_sq, dtype=np.float64)
    t = int(tol.size)
    out_i = np.zeros((k, 2, 1 + t), np.int64)
    out_f = np.zeros((k, 2), np.float64)
    head = (int(device), a.ctypes.data, int(kind_a), b.ctypes.data, int(kind_b), vals.ctypes.data if vals is not None else None, k, h, w,
            float(spacing_hw[0]), float(spacing_hw[1]), tol.ctypes.data if t else None, t)
    return fn, head, k, out_i, out_f, (vals, tol)


def surface_distances(a: np.ndarray, kind_a: int, b: np.ndarray, kind_b: int, values, shape_hw, spacing_hw, tol_sq, max_scratch_bytes: int = 0,
                      device: int = 0):
    """The boundary distances of 2-D planes on the device (C-ABI ts2d_surface_distances).  ``a``, ``b`` as in :func:`label_overlap` with Z = 1;
    ``tol_sq``: the squared tolerances, float64 [T].  Returns ``(int64 [K, 2, 1 + T], float64 [K, 2])`` in the layout of include/ts2d_engine.h."""
    fn, head, _, out_i, out_f, keep = _surface_call('surface_distances', a, kind_a, b, kind_b, values, shape_hw, spacing_hw, tol_sq, device)
    _lib.check(fn(*head, int(max_scratch_bytes), out_i.ctypes.data, out_f.ctypes.data), 'ts2d_surface_distances')
    del keep
    return out_i, out_f


def surface_profile_scratch_per_label(shape_hw, n_percentiles: int, want_sum: bool) -> int:
    """The scratch bytes ts2d_surface_distance_profile needs per label (include/ts2d_engine.h): what ``max_scratch_bytes`` is divided by."""
    h, w = (int(v) for v in shape_hw)
    p = int(n_percentiles)
    return 6 * h * w + (16 * h * w + 4096 * p if p else 0) + (16 * h if want_sum else 0)


def surface_distance_profile(a: np.ndarray, kind_a: int, b: np.ndarray, kind_b: int, values, shape_hw, spacing_hw, tol_sq, percentiles,
                             want_sum: bool, max_scratch_bytes: int = 0, device: int = 0):
    """:func:`surface_distances` and the distance profile in one call (C-ABI ts2d_surface_distance_profile).  ``percentiles``: float64 [P] in
    0 ... 100.  Returns ``(int64 [K, 2, 1 + T], float64 [K, 2], sums float64 [K, 2] or None, ranks float64 [K, 2, P, 2], weights float64
    [K, 2, P])`` in the layout of include/ts2d_engine.h."""
    fn, head, k, out_i, out_f, keep = _surface_call('surface_distance_profile', a, kind_a, b, kind_b, values, shape_hw, spacing_hw, tol_sq, device)
    pct = np.ascontiguousarray(percentiles, dtype=np.float64)
    p = int(pct.size)
    out_sum = np.zeros((k, 2), np.float64) if want_sum else None
    out_rank = np.zeros((k, 2, p, 2), np.float64)
    out_weight = np.zeros((k, 2, p), np.float64)
    _lib.check(fn(*head, pct.ctypes.data if p else None, p, 1 if want_sum else 0, int(max_scratch_bytes), out_i.ctypes.data, out_f.ctypes.data,
                  out_sum.ctypes.data if want_sum else None, out_rank.ctypes.data if p else None, out_weight.ctypes.data if p else None),
               'ts2d_surface_distance_profile')
    del keep
    return out_i, out_f, out_sum, out_rank, out_weight


def volume_scratch_per_label(box_zhw, n_percentiles: int, want_sum: bool) -> int:
    """The scratch bytes ts2d_volume_surface_distances needs for a label whose joint box has the extents ``box_zhw`` (include/ts2d_engine.h):
    what ``max_scratch_bytes`` bounds per chunk of labels."""
    z, h, w = (int(v) for v in box_zhw)
    return z * h * w * (22 + (16 if n_percentiles else 0)) + (16 * z * h if want_sum else 0)


def volume_surface_distances(a: np.ndarray, kind_a: int, b: np.ndarray, kind_b: int, values, shape_zhw, spacing_zhw, tol_sq, percentiles=(),
                             want_sum: bool = False, max_scratch_bytes: int = 0, device: int = 0):
    """The boundary distances of volumes on the device, with their profile on request (C-ABI ts2d_volume_surface_distances).  ``a``, ``b`` as in
    :func:`label_overlap`; ``tol_sq``: the squared tolerances, float64 [T]; ``percentiles``: float64 [P] in 0 ... 100 (none, and no
    ``want_sum``: the plain form).  Returns ``(int64 [K, 2, 1 + T], float64 [K, 2], sums float64 [K, 2] or None, ranks float64 [K, 2, P, 2],
    weights float64 [K, 2, P])`` in the layout of include/ts2d_engine.h."""
    fn = _entry('ts2d_volume_surface_distances')
    z, h, w = (int(v) for v in shape_zhw)
    k, vals = _evaluate_sides('volume_surface_distances', a, kind_a, b, kind_b, values, z * h * w)
    tol = np.ascontiguousarray(tol_sq, dtype=np.float64)
    pct = np.ascontiguousarray(percentiles, dtype=np.float64)
    t, p = int(tol.size), int(pct.size)
    out_i = np.zeros((k, 2, 1 + t), np.int64)
    out_f = np.zeros((k, 2), np.float64)
    out_sum = np.zeros((k, 2), np.float64) if want_sum else None
    out_rank = np.zeros((k, 2, p, 2), np.float64)
    out_weight = np.zeros((k, 2, p), np.float64)
    _lib.check(fn(int(device), a.ctypes.data, int(kind_a), b.ctypes.data, int(kind_b), vals.ctypes.data if vals is not None else None, k, z, h, w,
                  float(spacing_zhw[0]), float(spacing_zhw[1]), float(spacing_zhw[2]), tol.ctypes.data if t else None, t,
                  pct.ctypes.data if p else None, p, 1 if want_sum else 0, int(max_scratch_bytes), out_i.ctypes.data, out_f.ctypes.data,
                  out_sum.ctypes.data if want_sum else None, out_rank.ctypes.data if p else None, out_weight.ctypes.data if p else None),
               'ts2d_volume_surface_distances')
    return out_i, out_f, out_sum, out_rank, out_weight


def _read_tiled_inf(engines, desc, n_images, engine_flags: bool):
    """The inf flags a tiled call left behind (upstream's inf check, done on the device).  With descriptors, ``last_tiled_inf_per_image``
    of the first engine is their per-image flags; ``last_tiled_inf`` of every engine is its own flag in the library (the flat entry and
    the ensemble: that fold's own) or, without ``engine_flags``, the OR over its images."""
    if desc is not None:
        engines[0].last_tiled_inf_per_image = [bool(desc[i].inf_flag) for i in range(n_images)]
    for e in engines:
        e.last_tiled_inf = bool(e.lib.ts2d_engine_tiled_inf_flag(e._h)) if engine_flags else any(e.last_tiled_inf_per_image)


def unpack_mask(packed: np.ndarray, W: int) -> np.ndarray:
    """[.., W/32] uint32 -> [.., W] uint8 {0,1}."""
    p = np.asarray(packed).view(np.uint32)
    bits = (p[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(p.shape[:-1] + (W,)).astype(np.uint8)
