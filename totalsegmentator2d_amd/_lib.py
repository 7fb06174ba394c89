"""Loader for ``libts2d_engine.so`` (the C-ABI of include/ts2d_engine.h).

north_star asks for "a thin C-ABI cffi layer"; ``cffi`` is used in ABI mode when it is importable and ``ctypes``
otherwise (cffi is absent from this image).  There is deliberately NO CPU fallback: if the HIP library is missing
or cannot be loaded the import of the product path fails loudly.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libts2d_engine.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'ts2d_engine.h')
ABI_VERSION = 9
MAX_STAGES = 16
PRECISION_F32_EXACT = 0
PRECISION_F32_SPLIT_F16X3 = 1
PRECISION_F16 = 2

class ArchDesc(ctypes.Structure):
    """``ts2d_arch_desc``."""
    _fields_ = [('input_channels', ctypes.c_int32), ('num_classes', ctypes.c_int32), ('n_stages', ctypes.c_int32),
                ('features', ctypes.c_int32 * MAX_STAGES), ('n_conv_enc', ctypes.c_int32 * MAX_STAGES),
                ('n_conv_dec', ctypes.c_int32 * MAX_STAGES), ('norm_eps', ctypes.c_float), ('leaky_slope', ctypes.c_float),
                ('strides', (ctypes.c_int32 * 2) * MAX_STAGES)]


class ResidualDesc(ctypes.Structure):
    """``ts2d_residual_desc``: what a ResidualEncoderUNet adds to ``ts2d_arch_desc``."""
    _fields_ = [('n_blocks', ctypes.c_int32 * MAX_STAGES), ('reserved', ctypes.c_int32 * 16)]


class TiledImage(ctypes.Structure):
    """``ts2d_tiled_image``: one image of ``ts2d_engine_predict_tiled_batch``."""
    _fields_ = [('image', ctypes.c_void_p), ('Hp', ctypes.c_int32), ('Wp', ctypes.c_int32), ('n_tiles', ctypes.c_int32),
                ('tile_y', ctypes.c_void_p), ('tile_x', ctypes.c_void_p), ('logits_f16', ctypes.c_void_p), ('seg_u8', ctypes.c_void_p),
                ('inf_flag', ctypes.c_int32)]


class TiledExport(ctypes.Structure):
    """``ts2d_tiled_export``: the resample-back of one image of ``ts2d_engine_predict_tiled_export``."""
    _fields_ = [('src_y', ctypes.c_int32), ('src_x', ctypes.c_int32), ('src_h', ctypes.c_int32), ('src_w', ctypes.c_int32),
                ('out_h', ctypes.c_int32), ('out_w', ctypes.c_int32), ('seg_u8', ctypes.c_void_p), ('logits_f32', ctypes.c_void_p)]


class TiledLabelmap(ctypes.Structure):
    """``ts2d_tiled_labelmap``: resample-back and argmax of one image of ``ts2d_ensemble_predict_tiled_labelmap``."""
    _fields_ = [('src_y', ctypes.c_int32), ('src_x', ctypes.c_int32), ('src_h', ctypes.c_int32), ('src_w', ctypes.c_int32),
                ('out_h', ctypes.c_int32), ('out_w', ctypes.c_int32), ('label_u8', ctypes.c_void_p)]


class TiledProbabilities(ctypes.Structure):
    """``ts2d_tiled_probabilities``: resample-back, non-linearity, fill and decision of one image of ``ts2d_ensemble_predict_tiled_probabilities``."""
    _fields_ = [('src_y', ctypes.c_int32), ('src_x', ctypes.c_int32), ('src_h', ctypes.c_int32), ('src_w', ctypes.c_int32),
                ('out_h', ctypes.c_int32), ('out_w', ctypes.c_int32), ('full_h', ctypes.c_int32), ('full_w', ctypes.c_int32),
                ('box_y', ctypes.c_int32), ('box_x', ctypes.c_int32), ('prob_f32', ctypes.c_void_p), ('decided_u8', ctypes.c_void_p)]


class TiledProbabilitiesRun(ctypes.Structure):
    """``ts2d_tiled_probabilities_run``: the outputs of ``n_slices`` consecutive images of ``ts2d_ensemble_predict_tiled_probabilities_stack`` - slices of
    one volume with one geometry - as a pointer and a head stride into the caller's [K, Z0, full_h, full_w]."""
    _fields_ = [('src_y', ctypes.c_int32), ('src_x', ctypes.c_int32), ('src_h', ctypes.c_int32), ('src_w', ctypes.c_int32),
                ('out_h', ctypes.c_int32), ('out_w', ctypes.c_int32), ('full_h', ctypes.c_int32), ('full_w', ctypes.c_int32),
                ('box_y', ctypes.c_int32), ('box_x', ctypes.c_int32), ('first_image', ctypes.c_int32), ('n_slices', ctypes.c_int32),
                ('prob_f32', ctypes.c_void_p), ('prob_head_stride', ctypes.c_int64), ('decided_u8', ctypes.c_void_p),
                ('decided_head_stride', ctypes.c_int64)]


PROB_MULTILABEL, PROB_LABELMAP, PROB_REGIONS = 0, 1, 2      # TS2D_PROB_*


class CcStep(ctypes.Structure):
    """``ts2d_cc_step``: one step of ``ts2d_keep_largest_components`` - the membership table of its labels and its background byte."""
    _fields_ = [('member', ctypes.c_uint8 * 256), ('background', ctypes.c_uint8)]


CC_GIVE_UP = 1                                              # TS2D_CC_GIVE_UP
PROJECT_MODES = {'max': 0, 'min': 1, 'mean': 2, 'median': 3, 'std': 4, 'first': 5, 'slice': 6}      # TS2D_PROJECT_*
PROJECT_MAX_MODES, PROJECT_RAY_CAP = 16, 8192               # TS2D_PROJECT_MAX_MODES, TS2D_PROJECT_RAY_CAP
PROJECT_NONFINITE, PROJECT_RAY_TOO_LONG = 1, 2              # TS2D_PROJECT_NONFINITE, TS2D_PROJECT_RAY_TOO_LONG
XR_NONFINITE = 1                                            # TS2D_XR_NONFINITE
VISUAL_NONFINITE = 1                                        # TS2D_VISUAL_NONFINITE
STATS_PLANES, STATS_LABELMAP, STATS_NONFINITE = 0, 1, 1     # TS2D_STATS_PLANES, TS2D_STATS_LABELMAP, TS2D_STATS_NONFINITE
STATS_INTS, STATS_F64S, STATS_MAX_CHANNELS = 10, 6, 64      # TS2D_STATS_INTS, TS2D_STATS_F64S, TS2D_STATS_MAX_CHANNELS
STATS_MAX_PERCENTILES = 8                                   # TS2D_STATS_MAX_PERCENTILES
LABELS_RANGE, EVAL_MAX_TOLERANCES, EVAL_MAX_EXTENT = 1, 8, 32767      # TS2D_LABELS_RANGE, TS2D_EVAL_MAX_TOLERANCES, TS2D_EVAL_MAX_EXTENT
EVAL_MAX_PERCENTILES = 8                                    # TS2D_EVAL_MAX_PERCENTILES
COMP_FULL, COMP_FACES, COMP_GIVE_UP, COMP_LIST_FULL, COMP_COUNTERS = 0, 1, 1, 2, 5      # TS2D_COMP_*
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE, MORPH_COUNTERS = 0, 1, 2, 3, 4     # TS2D_MORPH_*

# shorthands of the table below: int, void *, size_t, long long, unsigned long long, char *; pointers to a void * and to the three descriptors
_I, _P, _Z, _LL, _ULL, _S = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_char_p
_PP, _TI, _TE, _TL = ctypes.POINTER(_P), ctypes.POINTER(TiledImage), ctypes.POINTER(TiledExport), ctypes.POINTER(TiledLabelmap)
_TP, _TPR = ctypes.POINTER(TiledProbabilities), ctypes.POINTER(TiledProbabilitiesRun)
_PROJECT = [_I, _P, _Z, _I, _I, _I, _I, _LL, _LL, _LL, _LL, _P, _P]
_D = ctypes.c_double
_XR_GEOMETRY = [_D, _D, _D, _D, _D, _I, _I, _D, _D, _I, _I]      # spacing_x, _y, _z, sdd, sod, view_pa, parallel, du, dv, nu, nv

# every symbol include/ts2d_engine.h declares: name -> (restype, argtypes)
SIGNATURES = {
    'ts2d_abi_version': (_I, []),                 # first: load() checks it before it looks up the rest
    'ts2d_last_error': (_S, []),
    'ts2d_engine_create': (_I, [ctypes.POINTER(ArchDesc), _P, _Z, _I, _PP]),
    'ts2d_engine_create_residual': (_I, [ctypes.POINTER(ArchDesc), ctypes.POINTER(ResidualDesc), _P, _Z, _I, _PP]),
    'ts2d_engine_load_weights': (_I, [_P, _P, _Z]),
    'ts2d_engine_weight_buffer': (_I, [_P, _PP, ctypes.POINTER(_Z)]),
    'ts2d_engine_weights_ready': (_I, [_P]),
    'ts2d_engine_forward': (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _P]),
    'ts2d_engine_check': (_I, [_P]),
    'ts2d_engine_predict_tiled': (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P]),
    'ts2d_engine_predict_tiled_batch': (_I, [_P, _TI, _I, _I, _I, _I, _P]),
    'ts2d_engine_predict_tiled_export': (_I, [_P, _TI, _TE, _I, _I, _I, _I, _P, _I]),
    'ts2d_ensemble_predict_tiled_export': (_I, [_PP, _I, _TI, _TE, _I, _I, _I, _I, _P, _I]),
    'ts2d_ensemble_predict_tiled_labelmap': (_I, [_PP, _I, _TI, _TL, _I, _I, _I, _I, _P, _I]),
    'ts2d_labelmap_from_logits': (_I, [_I, _P, _I, _I, _I, ctypes.POINTER(ctypes.c_int32 * 4), _I, _I, _P]),
    'ts2d_ensemble_predict_tiled_regions': (_I, [_PP, _I, _TI, _TL, _I, _I, _I, _I, _P, _I, _P, _I]),
    'ts2d_regions_from_logits': (_I, [_I, _P, _I, _I, _I, ctypes.POINTER(ctypes.c_int32 * 4), _I, _I, _P, _P]),
    'ts2d_ensemble_predict_tiled_probabilities': (_I, [_PP, _I, _TI, _TP, _I, _I, _I, _I, _P, _I, _I, _P, _I]),
    'ts2d_ensemble_predict_tiled_probabilities_stack': (_I, [_PP, _I, _TI, _I, _TPR, _I, _I, _I, _I, _P, _I, _I, _P, _I]),
    'ts2d_probabilities_from_logits': (_I, [_I, _P, _I, _I, _I, ctypes.POINTER(ctypes.c_int32 * 4), _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    'ts2d_project_coronal': (_I, _PROJECT),
    'ts2d_project_coronal_zscore': (_I, _PROJECT + [_P, _P, _P]),
    'ts2d_project_coronal_modes': (_I, _PROJECT[:-2] + [_P, _P, _I, _P, _P, _P, _P, _P]),
    'ts2d_project_xr': (_I, _PROJECT[:-2] + _XR_GEOMETRY + [_D, _D, _I, _D, _P, _P, _P]),
    'ts2d_project_labels_xr': (_I, _PROJECT[:-2] + _XR_GEOMETRY + [_I, _P, _P]),
    'ts2d_resample_cubic': (_I, [_I, _P, _I, _I, _I, _I, _I, _P, _P]),
    'ts2d_planes_create': (_I, [_I, _P, _I, _I, _I, _PP]),
    'ts2d_planes_crop_zscore': (_I, [_P, ctypes.POINTER(ctypes.c_int32 * 4), _P, ctypes.POINTER(_I)]),
    'ts2d_planes_crop_normalize': (_I, [_P, _P, _P, _P, ctypes.POINTER(ctypes.c_int32 * 4), _P, ctypes.POINTER(_I)]),
    'ts2d_planes_create_stack': (_I, [_I, _P, _I, _I, _I, _I, _PP]),
    'ts2d_planes_crop_normalize_stack': (_I, [_P, _P, _P, _P, ctypes.POINTER(ctypes.c_int32 * 6), _P, ctypes.POINTER(_I)]),
    'ts2d_planes_crop_normalize_stack_masked': (_I, [_P, _P, _P, _P, ctypes.POINTER(ctypes.c_int32 * 6), _P, ctypes.POINTER(_I)]),
    'ts2d_planes_resample_cubic': (_I, [_P, _I, _I]),
    'ts2d_planes_extent': (_I, [_P, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    'ts2d_planes_download': (_I, [_P, _P]),
    'ts2d_planes_destroy': (_I, [_P]),
    'ts2d_keep_largest_components': (_I, [_I, _P, _I, _I, _I, _P, _I, _P, ctypes.POINTER(_I)]),
    'ts2d_visual_labels': (_I, [_I, _P, _I, _I, _I, _D, _D, _P, _I, _I, _I, _P]),
    'ts2d_visual_grey': (_I, [_I, _P, _I, _I, _I, _D, _D, _I, _D, _D, _I, _I, _I, _I, _P, _P, ctypes.POINTER(_I)]),
    'ts2d_label_statistics': (_I, [_I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _Z, _P, _P, ctypes.POINTER(_I)]),
    'ts2d_label_percentiles': (_I, [_I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _P, _I, _Z, _P, _P, _P, ctypes.POINTER(_I)]),
    'ts2d_label_components': (_I, [_I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _Z, _P, _P, _P, ctypes.c_int64, _P, ctypes.POINTER(_I)]),
    'ts2d_project_labels_coronal': (_I, _PROJECT[:-2] + [_I, _P, _P]),
    'ts2d_label_overlap': (_I, [_I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P]),
    'ts2d_surface_distances': (_I, [_I, _P, _I, _P, _I, _P, _I, _I, _I, _D, _D, _P, _I, _Z, _P, _P]),
    'ts2d_surface_distance_profile': (_I, [_I, _P, _I, _P, _I, _P, _I, _I, _I, _D, _D, _P, _I, _P, _I, _I, _Z, _P, _P, _P, _P, _P]),
    'ts2d_volume_surface_distances': (_I, [_I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _D, _D, _D, _P, _I, _P, _I, _I, _Z, _P, _P, _P, _P, _P]),
    'ts2d_label_confusion': (_I, [_I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P]),
    'ts2d_label_morphology': (_I, [_I, _P, _I, _P, _I, _I, _I, _D, _D, _I, _D, _P, ctypes.c_uint64, _P, _P]),
    'ts2d_synth_slices': (_I, [_I, _ULL, _ULL, _ULL, _P, _P]),
    'ts2d_engine_reserve': (_I, [_P, _I, _I, _I]),
    'ts2d_engine_workspace_bytes': (_I, [_P, _I, _I, _I, ctypes.POINTER(_Z)]),
    'ts2d_engine_set_workspace': (_I, [_P, _P, _Z]),
    'ts2d_engine_set_precision': (_I, [_P, _I]),
    'ts2d_engine_set_option': (_I, [_P, _S, _I]),
    'ts2d_engine_set_tile_dtype': (_I, [_P, _I]),
    'ts2d_engine_set_keep_activations': (_I, [_P, _I]),
    'ts2d_engine_set_profiling': (_I, [_P, _I]),
    'ts2d_engine_num_ops': (_I, [_P]),
    'ts2d_engine_op_name': (_S, [_P, _I]),
    'ts2d_engine_op_kernel': (_S, [_P, _I]),
    'ts2d_engine_op_ksplit': (_I, [_P, _I]),
    'ts2d_engine_op_times': (_I, [_P, _P, _I]),
    'ts2d_engine_debug_tensor': (_I, [_P, _S, _P, _Z, ctypes.POINTER(ctypes.c_int32 * 4)]),
    'ts2d_engine_tiled_inf_flag': (_I, [_P]),
    'ts2d_engine_device_bytes': (_Z, [_P]),
    'ts2d_engine_destroy': (_I, [_P]),
}
SYMBOLS = tuple(SIGNATURES)
# added under ABI 9 (the cubic resample; the device-resident planes of preprocess.DevicePlanes, ts2d_planes_crop_normalize after the others, the two *_stack entries, then ts2d_planes_crop_normalize_stack_masked last):
# a library built before them lacks the symbols, still loads, and the callers keep the host route; the probabilities entries likewise (the one for stacks came after the other two: each is looked up on its own)
# ... and the residual-encoder entry: without it a ResidualEncoderUNet cannot be created (Engine says so), a plain net is unaffected
# ... and the largest-component postprocessing: without it postprocess.apply_postprocessing keeps the host route
# ... and the projection modes: without the entry TS2D keeps the host route for a channel name beyond max / mean
# ... and the two entries of the PNG visuals: without them visual.create_visual returns the statement's bytes from the host
# ... and the per-label statistics: without the entry statistics.label_statistics keeps the host route (its statement)
# ... and the percentiles under a label: without the entry statistics.label_statistics takes them from its statement
# ... and the three entries of the evaluation: without them evaluate.evaluate and Result.evaluate keep the host route (the statements)
# ... and the distance profile: without the entry evaluate.evaluate takes percentiles and average distances from its statement
# ... and the boundary distances of volumes: without the entry evaluate.evaluate(volume_distances=True) keeps its statement
# ... and the components of every label at once: without the entry components.label_components and clean_components keep the host route (their statement)
# ... and the confusion matrix: without the entry evaluate.confusion keeps the host route (its statement)
# ... and the label morphology: without the entry morphology.label_morphology keeps the host route (its statement)
# ... and the two entries of the synthetic radiograph: without them xray.synthetic_xr and xray.project_labels_xr keep the host route (their statements)
OPTIONAL = frozenset(n for n in SIGNATURES if n == 'ts2d_resample_cubic' or n.startswith('ts2d_planes_') or 'probabilities' in n
                     or n.startswith('ts2d_visual_')
                     or n in ('ts2d_engine_create_residual', 'ts2d_keep_largest_components', 'ts2d_project_coronal_modes', 'ts2d_label_statistics', 'ts2d_label_percentiles',
                              'ts2d_project_labels_coronal', 'ts2d_label_overlap', 'ts2d_surface_distances', 'ts2d_surface_distance_profile',
                              'ts2d_volume_surface_distances', 'ts2d_label_components', 'ts2d_label_confusion', 'ts2d_project_xr', 'ts2d_project_labels_xr', 'ts2d_label_morphology'))


class EngineLibraryError(RuntimeError):
    pass


_lib = None


def build(verbose: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    import subprocess
    subprocess.check_call(['make', '-C', os.path.join(_HERE, 'csrc')] + ([] if verbose else ['-s']))
    return LIB_PATH


def load():
    """dlopen the engine and declare its signatures.  Raises EngineLibraryError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineLibraryError(
            f"{LIB_PATH} is missing: the MI355X HIP engine has not been built (run `python -c 'import "
            f"__graft_entry__ as g; g.build()'` or `make -C totalsegmentator2d_amd/csrc`). There is no CPU fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as ex:
        raise EngineLibraryError(f"failed to load {LIB_PATH}: {ex}") from ex
    for name, (restype, argtypes) in SIGNATURES.items():
        if name in OPTIONAL and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
        if name == 'ts2d_abi_version' and fn() != ABI_VERSION:      # the table's first entry: another ABI is refused before its symbols are looked up
            raise EngineLibraryError(f"ABI mismatch: library {fn()}, binding {ABI_VERSION}")
    _lib = lib
    return lib


def load_cffi():
    """Same library through cffi (ABI mode) when cffi is installed; returns (ffi, lib) or None."""
    try:
        import cffi
    except ImportError:
        return None
    import re
    ffi = cffi.FFI()
    src = open(HEADER_PATH).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = '\n'.join(l for l in src.splitlines() if not l.strip().startswith('#') and 'extern "C"' not in l
                    and l.strip() not in ('}',))
    src = src.replace('TS2D_MAX_STAGES', str(MAX_STAGES))
    ffi.cdef(src)
    return ffi, ffi.dlopen(LIB_PATH)


def last_error() -> str:
    return load().ts2d_last_error().decode('utf-8', 'replace')


def check(rc: int, what: str):
    """status code -> RuntimeError (reference error convention: Python exceptions,
    ``ts2d/core/inference/prediction_worker.py:211-212``)."""
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")
