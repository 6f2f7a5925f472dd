"""ctypes binding of libdmstereo.so (C ABI: include/dmstereo.h).

``import torch`` happens before the library is loaded so that its ``libamdhip64.so.7``
dependency resolves to the HIP runtime torch already loaded (one runtime per process:
torch's device pointers and streams are then valid in the library).

There is no fallback: if the library is missing or cannot be loaded, every entry point
raises ``DmUnavailable`` (build it with ``python -m deepmatching_stereo_matching_amd.build_ext``).
"""

import ctypes
import os
import re

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DM_LIB_PATH') or os.path.join(HERE, 'libdmstereo.so')
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'dmstereo.h')
HEADER_SGM = os.path.join(os.path.dirname(HERE), 'include', 'dmstereo_sgm.h')   # dm_sgm_refine: a header of its own
HEADER_LSM = os.path.join(os.path.dirname(HERE), 'include', 'dmstereo_lsm.h')   # dm_lsm_affine likewise

DM_OK, DM_ERR_ARG, DM_ERR_SHAPE, DM_ERR_UNSUPPORTED, DM_ERR_HIP = 0, -1, -2, -3, -4
DM_VOLUME_F16, DM_VOLUME_MINMAX_KNOWN = 1, 2   # dm_corr_volume_ex flags
DM_POW_F32, DM_POW_Q4, DM_POW_K, DM_POW_FULL = 0, 1, 2, 3   # dm_pow14_variant forms
DM_TM_CCOEFF, DM_TM_CCOEFF_NORMED = 4, 5
METHODS = {'cv2.TM_CCOEFF_NORMED': DM_TM_CCOEFF_NORMED, 'cv2.TM_CCOEFF': DM_TM_CCOEFF}
CAL_MODES = {'elevation': 0, 'elevation2': 1, 'distance': 2}
DM_GS_FWD4, DM_GS_BWD4, DM_GS_BILAT = 0, 1, 2
DM_MERGE_LAST, DM_MERGE_CENTER, DM_MERGE_FEATHER, DM_MERGE_MEDIAN = 0, 1, 2, 3   # dm_stitch_merge rules
MERGE_RULES = {'last': DM_MERGE_LAST, 'center': DM_MERGE_CENTER, 'feather': DM_MERGE_FEATHER,
               'median': DM_MERGE_MEDIAN}
DM_MERGE_MAX_CAND = 64   # tiles over one pixel that dm_stitch_merge takes
DM_BILAT_FILL, DM_BILAT_GUIDE_U8 = 1, 2   # dm_bilateral_filter flags
DM_MEDIAN_FILL = 1   # dm_median_filter flag
DM_PHOTO_REJECT = 1   # dm_photo_score flag
DM_REFINE_SUBPIX = 1   # dm_photo_refine flag
DM_SGM_SUBPIX = 1   # dm_sgm_refine flag


class DmUnavailable(ImportError):
    pass


class DmError(RuntimeError):
    pass


class DmTiles(ctypes.Structure):
    _fields_ = [('d_img1', ctypes.c_void_p), ('d_img2', ctypes.c_void_p),
                ('pitch1', ctypes.c_int32), ('pitch2', ctypes.c_int32),
                ('d_origins', ctypes.c_void_p), ('T', ctypes.c_int32),
                ('h0', ctypes.c_int32), ('w0', ctypes.c_int32),
                ('ws', ctypes.c_int32), ('method', ctypes.c_int32)]


_P = ctypes.c_void_p
_I = ctypes.c_int32
_TP = ctypes.POINTER(DmTiles)
SIGNATURES = {
    'dm_abi_version': ([], ctypes.c_int),
    'dm_last_error': ([], ctypes.c_char_p),
    'dm_build_config': ([], ctypes.c_char_p),
    'dm_stats_bytes': ([_TP], ctypes.c_size_t),
    'dm_corr_stats': ([_TP, _P, _P], ctypes.c_int),
    'dm_corr_level1': ([_TP, _P, _P, _P], ctypes.c_int),
    'dm_corr_level12': ([_TP, _P, _P, _P, _P], ctypes.c_int),
    'dm_corr_volume': ([_TP, _P, _P, _P], ctypes.c_int),
    'dm_corr_volume_f16': ([_TP, _P, _P, _P], ctypes.c_int),
    'dm_corr_volume_ex': ([_TP, _P, _I, _P, _P], ctypes.c_int),
    'dm_rectify_f16': ([_P, ctypes.c_size_t, _P, _P], ctypes.c_int),
    'dm_rectify': ([_P, ctypes.c_size_t, _P, _P], ctypes.c_int),
    'dm_rectify64': ([_P, ctypes.c_size_t, _P, _P], ctypes.c_int),
    'dm_pow14_variant': ([_I, _P, ctypes.c_size_t, _P, _P], ctypes.c_int),
    'dm_debug_num_tile_f16': ([_P, _P, _I, _P, _P], ctypes.c_int),
    'dm_level_num_f16': ([_TP], ctypes.c_int),
    'dm_aggregate': ([_P, _I, _I, _I, _I, _P, _P], ctypes.c_int),
    'dm_match': ([_TP, _P, ctypes.POINTER(ctypes.c_void_p), _I, _I, _I, _I, _I, _I, _I, _I,
                  _P, _P, _P], ctypes.c_int),
    'dm_subpix_map': ([_P, _I, _I, _I, _I, _I, _P, _P], ctypes.c_int),
    'dm_subpix_map_tiles': ([_TP, _P, _I, _I, _P, _P], ctypes.c_int),
    'dm_sub_pix_cal': ([_P, _P, _I, _I, _I, ctypes.c_double, _P, _P], ctypes.c_int),
    'dm_cal_map': ([_P, _I, _I, _I, _I, _P, _P], ctypes.c_int),
    'dm_gs_schedule': ([_I, _I, _I, _I, _I, _I, _P, _P, ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    'dm_image_threshold': ([_P, ctypes.c_size_t, ctypes.c_double, ctypes.c_double, _P, _P], ctypes.c_int),
    'dm_optimize_loop': ([_P, _P, _I, _I, _I, _I, _I, _I, _I, ctypes.c_double, _P, _P, _I, _P, _P, _I,
                          _P, _P, _P], ctypes.c_int),
    'dm_make_weight': ([_P, _I, _I, _I, _I, _I, ctypes.c_double, ctypes.c_double, _P, _P, _P], ctypes.c_int),
    'dm_opt_loop_bilateral': ([_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P],
                              ctypes.c_int),
    'dm_stitch': ([_P, _I, _I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), _I, _P, _P, _P],
                  ctypes.c_int),
    'dm_seq_sum': ([_P, ctypes.c_int64, _P, _P], ctypes.c_int),
    'dm_fb_check': ([_P, _P, _I, _I, _I, ctypes.c_double, _P, _P, _P], ctypes.c_int),
    'dm_stitch_fb': ([_P, _P, _I, _I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), _I, ctypes.c_double,
                      _P, _P, _P, _P], ctypes.c_int),
    'dm_stitch_merge': ([_P, _P, _I, _I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), _I, ctypes.c_double,
                         _I, _I, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    'dm_fill_bytes': ([_I, _I, _I], ctypes.c_size_t),
    'dm_fill_holes': ([_P, _I, _I, _I, _I, _P, _P, _P, _P], ctypes.c_int),
    'dm_speckle_bytes': ([_I, _I, _I], ctypes.c_size_t),
    'dm_filter_speckles': ([_P, _I, _I, _I, _I, ctypes.c_double, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    'dm_bilateral_bytes': ([_I, _I, _I], ctypes.c_size_t),
    'dm_bilateral_filter': ([_P, _P, _I, _I, _I, _I, _I, ctypes.c_double, ctypes.c_double, _I, _I, _P, _P, _P, _P],
                            ctypes.c_int),
    'dm_median_bytes': ([_I, _I, _I], ctypes.c_size_t),
    'dm_median_filter': ([_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P], ctypes.c_int),
    'dm_photo_bytes': ([_I, _I, _I], ctypes.c_size_t),
    'dm_photo_score': ([_P, ctypes.c_int64, _P, ctypes.c_int64, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I,
                        ctypes.c_double, _P, _I, _P, _P, _P, _P, _P], ctypes.c_int),
    'dm_photo_refine_bytes': ([_I, _I, _I, _I, _I, _I], ctypes.c_size_t),
    'dm_photo_refine': ([_P, ctypes.c_int64, _P, ctypes.c_int64, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I,
                         ctypes.c_double, _I, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    'dm_lsm_refine_bytes': ([_I, _I, _I, _I, _I, _I], ctypes.c_size_t),
    'dm_lsm_refine': ([_P, ctypes.c_int64, _P, ctypes.c_int64, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I,
                       ctypes.c_double, _I, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    'dm_sgm_bytes': ([_I, _I, _I, _I], ctypes.c_size_t),
    'dm_sgm_refine': ([_P, ctypes.c_int64, _P, ctypes.c_int64, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I,
                       _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    'dm_lsm_affine_bytes': ([_I, _I, _I, _I, _I, _I], ctypes.c_size_t),
    'dm_lsm_affine': ([_P, ctypes.c_int64, _P, ctypes.c_int64, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I,
                       ctypes.c_double, ctypes.c_double, _I, _P, _P, _P, _P, _P, _P, _P, _P], ctypes.c_int),
    'dm_downsample2': ([_P, ctypes.c_int64, _I, _I, _P, ctypes.c_int64, _P], ctypes.c_int),
    'dm_tile_prior': ([_P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P], ctypes.c_int),
    'dm_pack_plan': ([_I, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                      ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    'dm_pack_tiles': ([_P, ctypes.c_int64, _P, ctypes.c_int64, _I, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P],
                      ctypes.c_int),
    'dm_shift_matches': ([_P, _P, _I, _I, _I, _P], ctypes.c_int),
}

_lib = None


def header_symbols(header=HEADER):
    """Function names declared in include/dmstereo.h (or in ``header``)."""
    txt = open(header).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(dm_[a-z0-9_]+)\s*\(', txt)))


def load(path=LIB_PATH):
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise DmUnavailable('HIP library %s is not built; run '
                            '`python -m deepmatching_stereo_matching_amd.build_ext`' % path)
    try:
        L = ctypes.CDLL(path)
    except OSError as e:
        raise DmUnavailable('cannot load %s: %s' % (path, e)) from e
    for name, (args, res) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def last_error():
    msg = load().dm_last_error()
    return msg.decode() if msg else ''


def check(rc, what=''):
    if rc == DM_OK:
        return
    msg = '%s: %s' % (what, last_error()) if what else last_error()
    if rc == DM_ERR_SHAPE:
        if 'list index out of range' in msg:
            raise IndexError(msg)
        raise ValueError(msg)
    if rc == DM_ERR_ARG:
        raise ValueError(msg)
    if rc == DM_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise DmError(msg)


def stream_handle(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
