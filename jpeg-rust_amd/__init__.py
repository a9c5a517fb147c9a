"""jpeg-rust_amd -- MI355X-native baseline-JPEG decode path behind martinhath/jpeg-rust's surface.

This module is only the ctypes binding over the C ABI in ``include/mjx.h`` (``libmjx.so``: host JFIF parse in C++,
HIP kernels for gfx950) plus a thin mirror of the reference's Rust interface so tests read like the reference:

    reference (src/jpeg/mod.rs, src/jpeg/decoder.rs)          here
    ---------------------------------------------------------------------------------------------
    JPEGImage::parse(bytes) -> width()/height()/image_data()   JPEGImage.parse(bytes)
    JPEGDecoder::new(data).frame_header().scan_header()        JPEGDecoder(data).frame_header()...
        .dimensions(); huffman_*_tables(); quantization_table()
        .decode() -> (Vec<(u8,u8,u8)>, usize)                  .decode() -> (ndarray[H,W,3] u8, bytes_read)
    HuffmanTable::from_size_data_tables(sizes, data)           HuffmanTable.from_size_data_tables(sizes, data)

There is no CPU fallback: every decode goes through the HIP kernels and raises ``MjxError`` (MJX_ERR_DEVICE) when no
GPU is present.  The directory name contains a hyphen (it is the name the project contract fixes), so import it with
``__graft_entry__.load_package()`` or ``importlib``.
"""
import ctypes
import sys
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_PKG)

# ---- status codes (include/mjx.h) ---------------------------------------------------------------
OK, ERR_TRUNCATED, ERR_UNSUPPORTED_MARKER, ERR_DRI_UNSUPPORTED, ERR_BAD_HUFFMAN, ERR_REF_PANIC, ERR_DEVICE, \
    ERR_UNSUPPORTED_FORMAT, ERR_NO_SCAN, ERR_INVALID_ARG, ERR_NOMEM, ERR_MISSING_TABLE = range(12)
LAYOUT_STANDARD, LAYOUT_REF_COMPAT = 0, 1
PIXELS_REFERENCE, PIXELS_LIBJPEG = 0, 1
IDCT_FLOAT, IDCT_ISLOW = 0, 1
UPSAMPLE_REPLICATE = 0x80        # mjx.h: MJX_UPSAMPLE_REPLICATE, or-ed into rh of upsample_color_host / upsample_luma_host
COLOR_POSITIONAL, COLOR_FILE = 0, 1
MODEL_GREY, MODEL_YCBCR, MODEL_RGB, MODEL_CMYK, MODEL_YCCK = range(5)
MODEL_NAMES = ["grey", "ycbcr", "rgb", "cmyk", "ycck"]
ABI_VERSION = 2                  # mjx.h: MJX_ABI_VERSION, the layout the structures below mirror (mjx_version() prints the library's)
STAGE_ENTROPY, STAGE_PIXELS, STAGE_ALL = 1, 2, 3
KERNEL_NAMES = ["gather", "huff_sync", "huff_fix", "huff_scan", "huff_write", "dc_scan", "idct_color", "upload", "huff_emit", "huff_prefix", "resize"]
SUBSAMPLING = {"444": 0, "422": 1, "420": 2, "gray": 3, "440": 4, "411": 5, "410": 6}


class MjxError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = int(code)
        msg = lib().mjx_strerror(self.code).decode() if _lib is not None else str(code)
        super().__init__("mjx error %d (%s)%s" % (self.code, msg, (": " + what) if what else ""))


class Rect(ctypes.Structure):
    """mjx_rect: a rectangle in the coordinates of the picture a call would otherwise produce; w == h == 0: the whole picture."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("x", "y", "w", "h")]


class Opts(ctypes.Structure):
    _fields_ = [("strict_ref", ctypes.c_uint8), ("layout", ctypes.c_uint8), ("keep_coefs", ctypes.c_uint8),
                ("device_destuff", ctypes.c_uint8), ("chunk_images", ctypes.c_uint32), ("pixels", ctypes.c_uint8),
                ("scale_denom", ctypes.c_uint8), ("rois", ctypes.POINTER(Rect)), ("n_rois", ctypes.c_uint32)]


def _opts_color(self):
    return ctypes.c_uint8.from_address(ctypes.addressof(self) + Opts.COLOR_OFFSET).value


def _opts_set_color(self, v):
    ctypes.c_uint8.from_address(ctypes.addressof(self) + Opts.COLOR_OFFSET).value = int(v)


Opts.COLOR_OFFSET = 10                  # MJX_OPTS_COLOR_OFFSET: the colour option lives in a padding byte behind scale_denom
Opts.color = property(_opts_color, _opts_set_color)


def _opts_progressive(self):
    return ctypes.c_uint8.from_address(ctypes.addressof(self) + Opts.PROGRESSIVE_OFFSET).value


def _opts_set_progressive(self, v):
    ctypes.c_uint8.from_address(ctypes.addressof(self) + Opts.PROGRESSIVE_OFFSET).value = int(v)


Opts.PROGRESSIVE_OFFSET = 11            # MJX_OPTS_PROGRESSIVE_OFFSET: the next padding byte
Opts.progressive = property(_opts_progressive, _opts_set_progressive)


def _opts_idct(self):
    return ctypes.c_uint8.from_address(ctypes.addressof(self) + Opts.IDCT_OFFSET).value


def _opts_set_idct(self, v):
    ctypes.c_uint8.from_address(ctypes.addressof(self) + Opts.IDCT_OFFSET).value = int(v)


Opts.IDCT_OFFSET = 12                   # MJX_OPTS_IDCT_OFFSET: the next padding byte
Opts.idct = property(_opts_idct, _opts_set_idct)


def _opts_exact_scale(self):
    return ctypes.c_uint8.from_address(ctypes.addressof(self) + Opts.EXACT_SCALE_OFFSET).value


def _opts_set_exact_scale(self, v):
    ctypes.c_uint8.from_address(ctypes.addressof(self) + Opts.EXACT_SCALE_OFFSET).value = int(v)


Opts.EXACT_SCALE_OFFSET = 13            # MJX_OPTS_EXACT_SCALE_OFFSET: the next padding byte
Opts.exact_scale = property(_opts_exact_scale, _opts_set_exact_scale)


class Dst(ctypes.Structure):
    """mjx_dst: caller-owned device memory for one picture; pitches in elements."""
    _fields_ = [("dev", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("row_pitch", ctypes.c_uint64), ("plane_pitch", ctypes.c_uint64)]


class OutputDesc(ctypes.Structure):
    """mjx_output: what the pictures of a call leave as (see Output)."""
    _fields_ = [("dtype", ctypes.c_uint8), ("planar", ctypes.c_uint8), ("bgr", ctypes.c_uint8),
                ("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3),
                ("dst", ctypes.POINTER(Dst)), ("n_dst", ctypes.c_uint32)]
    CHANNELS_OFFSET = 3                 # MJX_OUTPUT_CHANNELS_OFFSET: the channel count lives in the byte behind bgr

    @property
    def channels(self):
        return ctypes.c_uint8.from_address(ctypes.addressof(self) + self.CHANNELS_OFFSET).value

    @channels.setter
    def channels(self, v):
        ctypes.c_uint8.from_address(ctypes.addressof(self) + self.CHANNELS_OFFSET).value = int(v)

    PAD_OFFSET = 28                     # MJX_OUTPUT_PAD_OFFSET: the pad colour lives in the three bytes in front of dst

    @property
    def pad(self):
        return tuple((ctypes.c_uint8 * 3).from_address(ctypes.addressof(self) + self.PAD_OFFSET))

    @pad.setter
    def pad(self, v):
        b = (ctypes.c_uint8 * 3).from_address(ctypes.addressof(self) + self.PAD_OFFSET)
        for c in range(3):
            b[c] = int(v[c])


class PlaneLayout(ctypes.Structure):
    """mjx_plane_layout: the planes of one picture; pitches in elements, width / height in samples of the component."""
    _fields_ = [("dev", ctypes.c_void_p * 3), ("row_pitch", ctypes.c_uint64 * 3), ("width", ctypes.c_uint32 * 3), ("height", ctypes.c_uint32 * 3)]


class PlanesDesc(ctypes.Structure):
    """mjx_planes: the pictures of a call leave as their component planes (see Planes)."""
    _fields_ = [("dtype", ctypes.c_uint8), ("interleave_chroma", ctypes.c_uint8),
                ("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3),
                ("dst", ctypes.POINTER(PlaneLayout)), ("n_dst", ctypes.c_uint32)]


class ResizeDesc(ctypes.Structure):
    """mjx_resize: the one target size of a call's pictures (see Resize)."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("antialias", ctypes.c_uint8), ("auto_scale", ctypes.c_uint8)]
    FILTER_OFFSET = 10                  # MJX_RESIZE_FILTER_OFFSET: the filter kind lives in the byte behind auto_scale

    @property
    def filter(self):
        return ctypes.c_uint8.from_address(ctypes.addressof(self) + self.FILTER_OFFSET).value

    @filter.setter
    def filter(self, v):
        ctypes.c_uint8.from_address(ctypes.addressof(self) + self.FILTER_OFFSET).value = int(v)

    FIT_OFFSET = 11                     # MJX_RESIZE_FIT_OFFSET: the fit mode lives in the struct's last byte

    @property
    def fit(self):
        return ctypes.c_uint8.from_address(ctypes.addressof(self) + self.FIT_OFFSET).value

    @fit.setter
    def fit(self, v):
        ctypes.c_uint8.from_address(ctypes.addressof(self) + self.FIT_OFFSET).value = int(v)


class OrientDesc(ctypes.Structure):
    """mjx_orient: where a picture's orientation code comes from (see Orient)."""
    _fields_ = [("from_exif", ctypes.c_uint8), ("extra", ctypes.POINTER(ctypes.c_uint8)), ("n_extra", ctypes.c_uint32)]


DTYPE_U8, DTYPE_F16, DTYPE_F32 = 0, 1, 2
FILTER_TRIANGLE, FILTER_BICUBIC, FILTER_NEAREST = 0, 1, 2
FILTERS = {"bilinear": FILTER_TRIANGLE, "bicubic": FILTER_BICUBIC, "nearest": FILTER_NEAREST}


def _filter_code(filter):
    """A filter's name (or its MJX_FILTER_* code) -> the code."""
    if isinstance(filter, str):
        if filter not in FILTERS:
            raise MjxError(ERR_INVALID_ARG, "filter %r (one of %s)" % (filter, ", ".join(sorted(FILTERS))))
        return FILTERS[filter]
    return int(filter)


FIT_STRETCH, FIT_COVER, FIT_CONTAIN = 0, 1, 2
FITS = {"stretch": FIT_STRETCH, "cover": FIT_COVER, "contain": FIT_CONTAIN}


def _fit_code(fit):
    """A fit mode's name (or its MJX_FIT_* code) -> the code."""
    if isinstance(fit, str):
        if fit not in FITS:
            raise MjxError(ERR_INVALID_ARG, "fit %r (one of %s)" % (fit, ", ".join(sorted(FITS))))
        return FITS[fit]
    return int(fit)


def _pad_bytes(pad):
    """A pad colour -- one value or three, 0 .. 255 -- -> three ints."""
    v = [pad] * 3 if np.isscalar(pad) else list(pad)
    if len(v) == 1:
        v = v * 3
    if len(v) != 3 or any(int(x) != x or not 0 <= int(x) <= 255 for x in v):
        raise MjxError(ERR_INVALID_ARG, "pad=%r (one value or three, 0 .. 255)" % (pad,))
    return tuple(int(x) for x in v)
_NP_DTYPES = {DTYPE_U8: np.uint8, DTYPE_F16: np.float16, DTYPE_F32: np.float32}


class Comp(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint8) for n in ("id", "h", "v", "tq", "td", "ta")]


class HuffTab(ctypes.Structure):
    _fields_ = [("bits", ctypes.c_uint8 * 16), ("vals", ctypes.c_uint8 * 256)]


class ScanPart(ctypes.Structure):
    _fields_ = [("scan", ctypes.POINTER(ctypes.c_uint8)), ("scan_len", ctypes.c_size_t), ("ncomp", ctypes.c_uint8),
                ("comp", ctypes.c_uint8 * 3), ("restart_interval", ctypes.c_uint16), ("n_restart", ctypes.c_uint32),
                ("restart_offsets", ctypes.POINTER(ctypes.c_uint32)), ("dc", HuffTab * 3), ("ac", HuffTab * 3)]


class ScanProg(ctypes.Structure):
    """mjx_scan_prog: Ss, Se, Ah, Al of one scan of a progressive file."""
    _fields_ = [(n, ctypes.c_uint8) for n in ("ss", "se", "ah", "al")]


class ScanDesc(ctypes.Structure):
    _fields_ = [("scan", ctypes.POINTER(ctypes.c_uint8)), ("scan_len", ctypes.c_size_t),
                ("width", ctypes.c_uint16), ("height", ctypes.c_uint16), ("ncomp", ctypes.c_uint8),
                ("comp", Comp * 3), ("qt", (ctypes.c_uint16 * 64) * 4), ("qt_present", ctypes.c_uint8),
                ("dc", HuffTab * 4), ("ac", HuffTab * 4), ("dc_present", ctypes.c_uint8),
                ("ac_present", ctypes.c_uint8), ("scan_is_stuffed", ctypes.c_uint8), ("restart_interval", ctypes.c_uint16),
                ("n_restart", ctypes.c_uint32), ("restart_offsets", ctypes.POINTER(ctypes.c_uint32)),
                ("n_parts", ctypes.c_uint8), ("parts", ctypes.POINTER(ScanPart)), ("owner_", ctypes.c_void_p),
                ("comp_fourth", Comp), ("model", ctypes.c_uint8), ("prog", ctypes.POINTER(ScanProg))]


class ColorInfo(ctypes.Structure):
    """mjx_color_info: what mjx_color_model found in a file."""
    _fields_ = [("model", ctypes.c_uint8), ("ncomp", ctypes.c_uint8), ("jfif", ctypes.c_uint8), ("adobe", ctypes.c_uint8),
                ("adobe_transform", ctypes.c_uint8), ("ids", ctypes.c_uint8 * 4)]


class Image(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("rgb", ctypes.POINTER(ctypes.c_uint8))]


# every symbol include/mjx.h declares: (restype, argtypes)
_P = ctypes.POINTER
_vp, _sz, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SYMBOLS = {
    "mjx_parse": (_int, [ctypes.c_char_p, _sz, _P(Opts), _P(ScanDesc)]),
    "mjx_free_scan": (None, [_P(ScanDesc)]),
    "mjx_validate": (_int, [_P(ScanDesc), _P(Opts)]),
    "mjx_plan_tiles": (_int, [_P(ScanDesc), _P(Opts), _P(ctypes.c_uint64), _P(ctypes.c_uint64), _P(ctypes.c_uint32)]),
    "mjx_decode": (_int, [ctypes.c_char_p, _sz, _P(Opts), _P(Image)]),
    "mjx_decode_batch_out": (_int, [_vp, _P(ctypes.c_char_p), _P(_sz), _sz, _P(Opts), ctypes.c_uint, _P(OutputDesc), _P(_int), _P(_vp)]),
    "mjx_batch_create_out": (_int, [_vp, _P(ScanDesc), _sz, _P(Opts), _P(OutputDesc), _P(_vp), _P(_int)]),
    "mjx_output_layout": (_int, [_P(ScanDesc), _P(Opts), _P(OutputDesc), _sz, _P(Dst), _P(_sz)]),
    "mjx_batch_output_info": (_int, [_vp, _sz, _P(Dst)] + [_P(ctypes.c_uint8)] * 3),
    "mjx_batch_output_channels": (_int, [_vp, _sz, _P(ctypes.c_uint8)]),
    "mjx_batch_copy_output": (_int, [_vp, _sz, _vp, _sz]),
    "mjx_batch_create_planes": (_int, [_vp, _P(ScanDesc), _sz, _P(Opts), _P(PlanesDesc), _P(_vp), _P(_int)]),
    "mjx_decode_batch_planes": (_int, [_vp, _P(ctypes.c_char_p), _P(_sz), _sz, _P(Opts), ctypes.c_uint, _P(PlanesDesc), _P(_int), _P(_vp)]),
    "mjx_planes_layout": (_int, [_P(ScanDesc), _P(Opts), _P(PlanesDesc), _sz, _P(PlaneLayout), _P(ctypes.c_uint32), _P(_sz)]),
    "mjx_batch_plane_info": (_int, [_vp, _sz, _P(ctypes.c_uint32), _P(PlaneLayout), _P(ctypes.c_uint8), _P(ctypes.c_uint8)]),
    "mjx_batch_copy_planes": (_int, [_vp, _sz, _vp, _sz]),
    "mjx_batch_create_planes_orient": (_int, [_vp, _P(ScanDesc), _sz, _P(Opts), _P(PlanesDesc), _P(ResizeDesc), _P(OrientDesc), _P(_vp), _P(_int)]),
    "mjx_decode_batch_planes_orient": (_int, [_vp, _P(ctypes.c_char_p), _P(_sz), _sz, _P(Opts), ctypes.c_uint, _P(PlanesDesc), _P(ResizeDesc), _P(OrientDesc),
                                              _P(_int), _P(_vp)]),
    "mjx_planes_orient_layout": (_int, [_P(ScanDesc), _P(Opts), _P(PlanesDesc), _P(ResizeDesc), ctypes.c_uint8, _sz, _P(PlaneLayout), _P(ctypes.c_uint8), _P(Rect)]),
    "mjx_batch_create_resize": (_int, [_vp, _P(ScanDesc), _sz, _P(Opts), _P(OutputDesc), _P(ResizeDesc), _P(_vp), _P(_int)]),
    "mjx_decode_batch_resize": (_int, [_vp, _P(ctypes.c_char_p), _P(_sz), _sz, _P(Opts), ctypes.c_uint, _P(OutputDesc), _P(ResizeDesc), _P(_int), _P(_vp)]),
    "mjx_resize_plan": (_int, [_P(ScanDesc), _P(Opts), _P(ResizeDesc), _sz, _P(ctypes.c_uint8), _P(Rect), _P(ctypes.c_uint32), _P(ctypes.c_uint32)]),
    "mjx_resize_weights": (_int, [ctypes.c_uint32, ctypes.c_uint32, _int, ctypes.c_uint32, _P(ctypes.c_uint32), _P(ctypes.c_float), _sz, _P(_sz)]),
    "mjx_resize_filter_weights": (_int, [ctypes.c_uint32, ctypes.c_uint32, _int, _int, ctypes.c_uint32, _P(ctypes.c_uint32), _P(ctypes.c_float), _sz, _P(_sz)]),
    "mjx_upsample_color_host": (_int, [_P(_P(ctypes.c_uint8)), _P(ctypes.c_uint32), _P(ctypes.c_uint32), _P(ctypes.c_uint8), _P(ctypes.c_uint8), ctypes.c_uint32,
                                       _P(Rect), _P(ctypes.c_uint8)]),
    "mjx_upsample_luma_host": (_int, [_P(ctypes.c_uint8), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint8, _P(Rect), _P(ctypes.c_uint8)]),
    "mjx_idct_islow_host": (_int, [_P(ctypes.c_int16), _P(ctypes.c_uint16), _P(ctypes.c_uint8)]),
    "mjx_plan_reduced": (_int, [_P(ScanDesc), _P(Opts), _P(ctypes.c_uint32)] + [_P(ctypes.c_uint32)] * 7),
    "mjx_idct_reduced_host": (_int, [_P(ctypes.c_int16), _P(ctypes.c_uint16), ctypes.c_uint32, _P(ctypes.c_uint8)]),
    "mjx_exif_orientation": (_int, [ctypes.c_char_p, _sz, _P(ctypes.c_uint8)]),
    "mjx_orient_compose": (ctypes.c_uint8, [ctypes.c_uint8, ctypes.c_uint8]),
    "mjx_color_model": (_int, [ctypes.c_char_p, _sz, _P(ColorInfo)]),
    "mjx_ink_mul": (ctypes.c_uint8, [ctypes.c_uint8, ctypes.c_uint8]),
    "mjx_batch_image_color": (_int, [_vp, _sz, _P(ctypes.c_uint8)]),
    "mjx_batch_create_orient": (_int, [_vp, _P(ScanDesc), _sz, _P(Opts), _P(OutputDesc), _P(ResizeDesc), _P(OrientDesc), _P(_vp), _P(_int)]),
    "mjx_decode_batch_orient": (_int, [_vp, _P(ctypes.c_char_p), _P(_sz), _sz, _P(Opts), ctypes.c_uint, _P(OutputDesc), _P(ResizeDesc), _P(OrientDesc), _P(_int), _P(_vp)]),
    "mjx_orient_plan": (_int, [_P(ScanDesc), _P(Opts), _P(ResizeDesc), ctypes.c_uint8, _sz, _P(ctypes.c_uint32), _P(ctypes.c_uint32), _P(Rect), _P(ctypes.c_uint8)]),
    "mjx_batch_image_orientation": (_int, [_vp, _sz, _P(ctypes.c_uint8)]),
    "mjx_batch_image_scale": (_int, [_vp, _sz, _P(ctypes.c_uint8)]),
    "mjx_batch_resize_rect": (_int, [_vp, _sz, _P(Rect)]),
    "mjx_batch_fit_rect": (_int, [_vp, _sz, _P(Rect)]),
    "mjx_resize_fit_plan": (_int, [_P(ScanDesc), _P(Opts), _P(OutputDesc), _P(ResizeDesc), ctypes.c_uint8, _sz, _P(Rect), _P(Rect), _P(ctypes.c_uint8)]),
    "mjx_decode_batch": (_int, [_vp, _P(ctypes.c_char_p), _P(_sz), _sz, _P(Opts), ctypes.c_uint, _P(_P(ctypes.c_uint8)), _P(_int), _P(_vp)]),
    "mjx_free_image": (None, [_P(Image)]),
    "mjx_ctx_create": (_int, [_int, _P(_vp)]),
    "mjx_ctx_destroy": (None, [_vp]),
    "mjx_ctx_set_profiling": (_int, [_vp, _int]),
    "mjx_ctx_set_throughput_plan": (_int, [_vp, _int]),
    "mjx_ctx_numa_node": (_int, [_vp]),
    "mjx_host_processors": (ctypes.c_uint, []),
    "mjx_batch_create": (_int, [_vp, _P(ScanDesc), _sz, _P(Opts), _P(_vp), _P(_int)]),
    "mjx_batch_free": (None, [_vp]),
    "mjx_batch_tile": (_int, [_vp, _vp, _sz, _P(_vp)]),
    "mjx_batch_decode": (_int, [_vp, ctypes.c_uint]),
    "mjx_batch_wait": (_int, [_vp]),
    "mjx_batch_size": (_sz, [_vp]),
    "mjx_batch_status": (_int, [_vp, _sz]),
    "mjx_batch_image_info": (_int, [_vp, _sz] + [_P(ctypes.c_uint32)] * 4),
    "mjx_batch_image_roi": (_int, [_vp, _sz] + [_P(ctypes.c_uint32)] * 4),
    "mjx_batch_rgb_device": (_int, [_vp, _sz, _P(_vp), _P(_sz)]),
    "mjx_batch_copy_rgb": (_int, [_vp, _sz, _vp]),
    "mjx_batch_copy_coefs": (_int, [_vp, _sz, _vp, _sz, _P(_sz)]),
    "mjx_batch_compare_rgb": (_int, [_vp, _P(_sz), _vp, _P(_sz), _sz, _P(ctypes.c_uint32), _P(ctypes.c_uint64)]),
    "mjx_batch_bytes": (_int, [_vp] + [_P(ctypes.c_uint64)] * 4),
    "mjx_batch_geometry": (_int, [_vp] + [_P(ctypes.c_uint64)] * 3),
    "mjx_batch_unconverged_runs": (_int, [_vp, _P(ctypes.c_uint64)]),
    "mjx_batch_kernel_ms": (_int, [_vp, _P(ctypes.c_double), _P(ctypes.c_uint64), _int]),
    "mjx_decode_scans": (_int, [_vp, _P(ScanDesc), _sz, _P(Opts), _P(_P(ctypes.c_uint8)), _P(_int), _P(_vp)]),
    "mjx_pool_create": (_int, [_P(_int), _sz, _P(_vp)]),
    "mjx_pool_destroy": (None, [_vp]),
    "mjx_pool_devices": (_sz, [_vp]),
    "mjx_pool_device": (_int, [_vp, _sz]),
    "mjx_pool_set_deal": (_int, [_vp, _int]),
    "mjx_pool_decode_batch": (_int, [_vp, _P(ctypes.c_char_p), _P(_sz), _sz, _P(Opts), ctypes.c_uint, _P(_int), _P(_P(ctypes.c_uint8)), _P(_int), _P(_vp)]),
    "mjx_pool_result_locate": (_int, [_vp, _sz, _P(_sz), _P(_vp), _P(_sz)]),
    "mjx_pool_result_host": (_int, [_vp, _sz, _P(ctypes.c_uint), _P(_int)]),
    "mjx_pool_result_slot_ms": (_int, [_vp, _sz, _P(ctypes.c_double)]),
    "mjx_pool_result_free": (None, [_vp]),
    "mjx_strerror": (ctypes.c_char_p, [_int]),
    "mjx_version": (ctypes.c_char_p, []),
}

_lib = None


def lib_path():
    """In-tree library; MJX_LIB overrides it (A/B comparisons of two builds on the same GPU box)."""
    return os.environ.get("MJX_LIB") or os.path.join(_PKG, "libmjx.so")


def lib():
    """Loads libmjx.so (built in-tree by build.py).  Fails loudly if it is missing: there is no fallback path."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise ImportError("libmjx.so is not built: run `python jpeg-rust_amd/build.py` (hipcc --offload-arch=gfx950)")
        l = ctypes.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


def _check(rc, what=""):
    if rc != OK:
        raise MjxError(rc, what)


DESTUFF_AUTO, DESTUFF_DEVICE, DESTUFF_HOST = 0, 1, 2


def _rects(rois):
    """None, one (x, y, w, h) or a list of them (None in the list: the whole picture) -> a ctypes array of Rect, or None."""
    if rois is None:
        return None
    if len(rois) == 4 and all(isinstance(v, (int, np.integer)) for v in rois):
        rois = [rois]
    arr = (Rect * max(len(rois), 1))()
    for i, r in enumerate(rois):
        x, y, w, h = (0, 0, 0, 0) if r is None else r
        if min(x, y, w, h) < 0 or max(x, y, w, h) > 0xffffffff:
            raise MjxError(ERR_INVALID_ARG, "roi=%s" % (r,))
        arr[i] = Rect(int(x), int(y), int(w), int(h))
    arr._n = len(rois)
    return arr


def _pixels(pixels):
    """None / "reference" / PIXELS_REFERENCE, or "libjpeg" / PIXELS_LIBJPEG (mjx.h: mjx_opts.pixels); "libjpeg-exact": "libjpeg", and
    _idct picks the integer inverse DCT with it."""
    names = {None: PIXELS_REFERENCE, "reference": PIXELS_REFERENCE, "libjpeg": PIXELS_LIBJPEG, "libjpeg-exact": PIXELS_LIBJPEG}
    if pixels is None or isinstance(pixels, str):
        if pixels not in names:
            raise MjxError(ERR_INVALID_ARG, "pixels=%r" % (pixels,))
        return names[pixels]
    if not 0 <= int(pixels) <= 255:
        raise MjxError(ERR_INVALID_ARG, "pixels=%r" % (pixels,))
    return int(pixels)


def _idct(idct, pixels=None):
    """None / "float" / IDCT_FLOAT, or "islow" / "islow-scaled" / IDCT_ISLOW (mjx.h: MJX_OPTS_IDCT); None with pixels="libjpeg-exact" is
    "islow".  ("islow-scaled": "islow", and _opts sets MJX_OPTS_EXACT_SCALE with it.)"""
    names = {None: IDCT_ISLOW if pixels == "libjpeg-exact" else IDCT_FLOAT, "float": IDCT_FLOAT, "islow": IDCT_ISLOW, "islow-scaled": IDCT_ISLOW}
    if idct is None or isinstance(idct, str):
        if idct not in names:
            raise MjxError(ERR_INVALID_ARG, "idct=%r" % (idct,))
        return names[idct]
    if not 0 <= int(idct) <= 255:
        raise MjxError(ERR_INVALID_ARG, "idct=%r" % (idct,))
    return int(idct)


def _color(color):
    """None / "positional" / COLOR_POSITIONAL, or "file" / COLOR_FILE (mjx.h: mjx_opts.color)."""
    names = {None: COLOR_POSITIONAL, "positional": COLOR_POSITIONAL, "file": COLOR_FILE}
    if color is None or isinstance(color, str):
        if color not in names:
            raise MjxError(ERR_INVALID_ARG, "color=%r" % (color,))
        return names[color]
    if not 0 <= int(color) <= 255:
        raise MjxError(ERR_INVALID_ARG, "color=%r" % (color,))
    return int(color)


def _opts(strict_ref=False, layout=LAYOUT_STANDARD, keep_coefs=False, chunk_images=0, device_destuff=False, scale=1, rois=None, pixels=None, color=None, progressive=False, idct=None):
    """device_destuff: True = on the GPU, False = on the host, None = the library's choice (mjx.h: MJX_DESTUFF_*).
    scale: 1, 2, 4 or 8 -- the picture decoded at 1/scale in the DCT domain (mjx.h: mjx_opts.scale_denom).
    rois: see _rects (mjx.h: mjx_opts.rois, n_rois); the Opts returned keeps the array alive.
    pixels: see _pixels -- "libjpeg": rounded samples, fancy chroma upsampling and libjpeg's integer colour tables.
    idct: see _idct -- "islow": libjpeg's integer slow inverse DCT, with pixels="libjpeg" only: the picture is byte for byte libjpeg's
    (mjx.h: MJX_OPTS_IDCT); pixels="libjpeg-exact" is shorthand for pixels="libjpeg", idct="islow".  With pixels="libjpeg-exact" (and the
    integer transform), or with idct="islow-scaled" beside pixels="libjpeg", scale=2, 4 or 8 is libjpeg's own reduced decode (mjx.h:
    MJX_OPTS_EXACT_SCALE: its reduced integer transforms, a size per component), again byte for byte; pixels="libjpeg", idct="islow"
    with a scale stays refused, as it was.
    color: see _color -- "file": the colour model comes from the file (RGB, CMYK and YCCK files decode to R,G,B).
    progressive: True -- progressive files (SOF2) are accepted (mjx.h: MJX_OPTS_PROGRESSIVE); an integer is passed through as it is."""
    dd = DESTUFF_AUTO if device_destuff is None else (DESTUFF_DEVICE if device_destuff else DESTUFF_HOST)
    scale = int(scale)
    if not 0 <= scale <= 255:
        raise MjxError(ERR_INVALID_ARG, "scale=%d" % scale)
    o = Opts(int(bool(strict_ref)), int(layout), int(bool(keep_coefs)), dd, int(chunk_images), _pixels(pixels), scale)
    o.color = _color(color)
    o.idct = _idct(idct, pixels)
    o.exact_scale = int(o.idct == IDCT_ISLOW and (idct == "islow-scaled" or pixels == "libjpeg-exact"))      # (idct given as "islow" or IDCT_ISLOW alike)
    o.progressive = int(progressive) if not isinstance(progressive, bool) and 0 <= int(progressive) <= 255 else int(bool(progressive))
    arr = _rects(rois)
    if arr is not None:
        o._rects = arr                      # (the library borrows the array for the duration of the call)
        o.rois = ctypes.cast(arr, _P(Rect))
        o.n_rois = arr._n
    return o


class Output:
    """What the pictures of a call leave as (mjx.h: mjx_output): dtype "uint8" / "float16" / "float32" (or DTYPE_*), planar
    (3 x H x W) or interleaved (H x W x 3), channels R,G,B or B,G,R.  A float element is fmaf(float(u8), scale[c], bias[c]) with c
    the OUTPUT channel; mean / std (of values in [0, 1], per output channel: (v / 255 - mean) / std) become scale = 1 / (255 std)
    and bias = -mean / std, computed in float64 and rounded once to float32.
    dst: None -- the library owns the output, dense -- or one (device pointer, width, height, row_pitch, plane_pitch) per input,
    pitches in elements.
    channels: 3, or 1 for luminance -- H x W elements, one per pixel (H x W x 1 and 1 x H x W are the same memory; planar only says
    which shape Batch.output gives; bgr has no meaning); mean / std / scale / bias are then one value (a scalar or one element).
    pad: the colour of the border of Resize(fit="contain"), one value or three of 0 .. 255 by OUTPUT channel (bgr does not reorder
    them; luminance uses the first).  A padded element is what a decoded pixel of that value would become: the byte, or
    fmaf(float(byte), scale[c], bias[c]).  0 is black -- Pad(fill=0) before Normalize; the mean colour's bytes give about 0 after
    normalisation.  Ignored by every other fit mode."""

    def __init__(self, dtype="uint8", planar=False, bgr=False, mean=None, std=None, scale=None, bias=None, dst=None, channels=3, pad=0):
        names = {"uint8": DTYPE_U8, "u8": DTYPE_U8, "float16": DTYPE_F16, "f16": DTYPE_F16, "float32": DTYPE_F32, "f32": DTYPE_F32}
        self.dtype = names[dtype] if isinstance(dtype, str) else int(dtype)
        self.planar, self.bgr = bool(planar), bool(bgr)
        self.channels = int(channels)
        if not 0 <= self.channels <= 255:
            raise MjxError(ERR_INVALID_ARG, "channels=%r" % (channels,))
        self.pad = _pad_bytes(pad)
        if (mean is not None or std is not None) and (scale is not None or bias is not None):
            raise MjxError(ERR_INVALID_ARG, "mean / std or scale / bias, not both")
        def three(v, d):
            if v is None:
                return [float(d)] * 3
            if np.isscalar(v):
                return [float(v)] * 3
            v = [float(x) for x in v]
            return v * 3 if self.channels == 1 and len(v) == 1 else v
        if mean is not None or std is not None:
            m, sd = np.array(three(mean, 0.0), np.float64), np.array(three(std, 1.0), np.float64)
            sc, bi = 1.0 / (255.0 * sd), -m / sd
        else:
            sc, bi = np.array(three(scale, 1.0), np.float64), np.array(three(bias, 0.0), np.float64)
        if len(sc) != 3 or len(bi) != 3:
            raise MjxError(ERR_INVALID_ARG, "one value per channel")
        self.scale, self.bias = sc.astype(np.float32), bi.astype(np.float32)
        self.dst = None if dst is None else [tuple(int(v) for v in d) for d in dst]

    def desc(self):
        """-> the ctypes mjx_output (it keeps its dst array alive)."""
        d = OutputDesc(self.dtype, int(self.planar), int(self.bgr))
        d.channels = self.channels
        d.pad = self.pad
        for c in range(3):
            d.scale[c], d.bias[c] = float(self.scale[c]), float(self.bias[c])
        if self.dst is not None:
            arr = (Dst * max(len(self.dst), 1))()
            for i, v in enumerate(self.dst):
                arr[i] = Dst(v[0] or None, v[1], v[2], v[3], v[4])
            d._arr = arr
            d.dst = ctypes.cast(arr, _P(Dst))
            d.n_dst = len(self.dst)
        return d

    def numpy_dtype(self):
        return _NP_DTYPES[self.dtype]


class Planes:
    """YCbCr output (mjx.h: mjx_planes): the pictures of a call leave as their component planes -- Y, Cb, Cr at their own sampling,
    no upsampling and no colour conversion; a uint8 4:2:0 picture is an I420 frame, with interleave=True NV12.  dtype "uint8" /
    "float16" / "float32" (or DTYPE_*); a float element is fmaf(float(u8), scale[c], bias[c]) with c the COMPONENT; mean / std (of
    values in [0, 1], per component) become scale = 1 / (255 std) and bias = -mean / std as in Output.
    dst: None -- the library owns the planes, dense and back to back -- or per input a list of (device pointer, row_pitch) per plane
    with the planes' (width, height) per component: ([(ptr, pitch), ...], [(w, h), ...]); pitches in elements."""

    def __init__(self, dtype="uint8", interleave=False, mean=None, std=None, scale=None, bias=None, dst=None):
        names = {"uint8": DTYPE_U8, "u8": DTYPE_U8, "float16": DTYPE_F16, "f16": DTYPE_F16, "float32": DTYPE_F32, "f32": DTYPE_F32}
        self.dtype = names[dtype] if isinstance(dtype, str) else int(dtype)
        self.interleave = bool(interleave)
        if (mean is not None or std is not None) and (scale is not None or bias is not None):
            raise MjxError(ERR_INVALID_ARG, "mean / std or scale / bias, not both")
        three = lambda v, d: [float(d)] * 3 if v is None else ([float(v)] * 3 if np.isscalar(v) else [float(x) for x in v])
        if mean is not None or std is not None:
            m, sd = np.array(three(mean, 0.0), np.float64), np.array(three(std, 1.0), np.float64)
            sc, bi = 1.0 / (255.0 * sd), -m / sd
        else:
            sc, bi = np.array(three(scale, 1.0), np.float64), np.array(three(bias, 0.0), np.float64)
        if len(sc) != 3 or len(bi) != 3:
            raise MjxError(ERR_INVALID_ARG, "one value per component")
        self.scale, self.bias = sc.astype(np.float32), bi.astype(np.float32)
        self.dst = dst

    def desc(self):
        """-> the ctypes mjx_planes (it keeps its dst array alive)."""
        d = PlanesDesc(self.dtype, int(self.interleave))
        for c in range(3):
            d.scale[c], d.bias[c] = float(self.scale[c]), float(self.bias[c])
        if self.dst is not None:
            arr = (PlaneLayout * max(len(self.dst), 1))()
            for i, (planes, sizes) in enumerate(self.dst):
                for c, (ptr, pitch) in enumerate(planes):
                    arr[i].dev[c] = int(ptr) or None
                    arr[i].row_pitch[c] = int(pitch)
                for c, (w, h) in enumerate(sizes):
                    arr[i].width[c], arr[i].height[c] = int(w), int(h)
            d._arr = arr
            d.dst = ctypes.cast(arr, _P(PlaneLayout))
            d.n_dst = len(self.dst)
        return d

    def numpy_dtype(self):
        return _NP_DTYPES[self.dtype]


def _planes_ref(planes):
    d = planes.desc() if isinstance(planes, Planes) else planes
    return d, ctypes.byref(d)


class Resize:
    """Resize on the device (mjx.h: mjx_resize): every picture of the call leaves at width x height, resampled from its decoded
    rectangle with the filter of torch.nn.functional.interpolate(mode=filter, align_corners=False, antialias=antialias) --
    filter "bilinear" (the triangle), "bicubic" (torch's two rules: a = -0.5, widening with the ratio, with antialias, which is also
    Pillow's BICUBIC; a = -0.75 and four taps without, which does not widen when shrinking) or "nearest" (torch's nearest-exact,
    Pillow's NEAREST; antialias is ignored).  auto_scale: the library picks the DCT-domain scale (1, 1/2, 1/4, 1/8) per picture so that the filter
    never has to shrink by more than it must; rois are then in FULL-SIZE coordinates and scale must be 1.  Without it the call's
    scale and rois apply as in any call.
    fit: "stretch" -- the rectangle is stretched to the target --, "cover" -- centre-crop: the largest centred part of the rectangle
    with the target's aspect fills the target, byte for byte the stretch call on that part -- or "contain" -- letterbox: the rectangle
    is resized to fit inside the target, centred, and the rest is Output's pad colour (mjx.h has the rule in integers).
    Mapping a source coordinate to the output: with p = ParsedScan.fit_plan(resize, ...), a point (px, py) of the oriented picture, in
    the coordinates p["asked"] is given in, lies at inner.x + (px - asked.x) * inner.w / asked.w, inner.y + (py - asked.y) * inner.h /
    asked.h of the target; Batch.fit_rect(i) gives the inner rectangle of a picture of a batch."""

    def __init__(self, width, height, antialias=True, auto_scale=True, filter="bilinear", fit="stretch"):
        self.width, self.height = int(width), int(height)
        self.antialias, self.auto_scale = bool(antialias), bool(auto_scale)
        self.filter = filter
        _filter_code(filter)
        self.fit = fit
        _fit_code(fit)
        if not (0 <= self.width <= 0xffffffff and 0 <= self.height <= 0xffffffff):
            raise MjxError(ERR_INVALID_ARG, "resize to %d x %d" % (self.width, self.height))

    def desc(self):
        d = ResizeDesc(self.width, self.height, int(self.antialias), int(self.auto_scale))
        d.filter = _filter_code(self.filter)
        d.fit = _fit_code(self.fit)
        return d

    def sized(self, width, height):
        """This description at another target size: everything else, the filter and the fit mode included, is kept."""
        return Resize(width, height, self.antialias, self.auto_scale, self.filter, self.fit)


def _rs_ref(resize):
    if resize is None:
        return None, None
    d = resize.desc() if isinstance(resize, Resize) else resize
    return d, ctypes.byref(d)


class Orient:
    """Orientation on the device (mjx.h: mjx_orient): picture i leaves turned by its EXIF orientation tag (exif=True; read from the
    file's bytes) followed by extra[i] -- None, one code 1..8 for every picture, or a list with one per picture (2 is the horizontal
    flip).  Rectangles are then in the coordinates of the picture that leaves."""

    def __init__(self, exif=True, extra=None):
        self.exif = bool(exif)
        self.extra = extra

    def codes(self, n):
        if self.extra is None:
            return None
        return [int(self.extra)] * n if isinstance(self.extra, (int, np.integer)) else [int(c) for c in self.extra]

    def desc(self, n, exif=None):
        """-> (what must stay alive, the mjx_orient); exif=False: the tags have been folded into `extra` already."""
        codes = self.codes(n)
        arr = (ctypes.c_uint8 * max(len(codes), 1))(*codes) if codes is not None else None
        d = OrientDesc(int(self.exif if exif is None else exif), ctypes.cast(arr, _P(ctypes.c_uint8)) if arr is not None else None,
                       len(codes) if codes is not None else 0)
        return (arr, d), d


def exif_orientation(data):
    """mjx_exif_orientation (host only): the EXIF orientation code 1..8 of a file; 1 when it has no readable tag."""
    c = ctypes.c_uint8()
    _check(lib().mjx_exif_orientation(bytes(data), len(data), ctypes.byref(c)), "mjx_exif_orientation")
    return c.value


def orient_compose(first, then):
    """mjx_orient_compose: the one code that does what `first` followed by `then` does."""
    c = int(lib().mjx_orient_compose(int(first), int(then)))
    if not c:
        raise MjxError(ERR_INVALID_ARG, "orient_compose(%r, %r)" % (first, then))
    return c


def resize_weights(n_in, n_out, antialias, X, filter="bilinear"):
    """mjx_resize_weights / mjx_resize_filter_weights (host only; the routine the resize kernel runs) -> (first input index, float32
    weights of the window); filter as Resize's."""
    first, cnt = ctypes.c_uint32(), _sz()
    f = _filter_code(filter)
    if f != FILTER_TRIANGLE:
        args = (int(n_in), int(n_out), f, int(bool(antialias)), int(X), ctypes.byref(first))
        _check(lib().mjx_resize_filter_weights(*args, None, 0, ctypes.byref(cnt)), "mjx_resize_filter_weights")
        w = np.zeros(max(cnt.value, 1), np.float32)
        _check(lib().mjx_resize_filter_weights(*args, w.ctypes.data_as(_P(ctypes.c_float)), cnt.value, ctypes.byref(cnt)), "mjx_resize_filter_weights")
        return first.value, w[:cnt.value]
    _check(lib().mjx_resize_weights(int(n_in), int(n_out), int(bool(antialias)), int(X), ctypes.byref(first), None, 0, ctypes.byref(cnt)), "mjx_resize_weights")
    w = np.zeros(max(cnt.value, 1), np.float32)
    _check(lib().mjx_resize_weights(int(n_in), int(n_out), int(bool(antialias)), int(X), ctypes.byref(first),
                                    w.ctypes.data_as(_P(ctypes.c_float)), cnt.value, ctypes.byref(cnt)), "mjx_resize_weights")
    return first.value, w[:cnt.value]


def upsample_color_host(planes, rh, rv, rect):
    """mjx_upsample_color_host (host only; the routines k_upsample_color runs): one or three uint8 planes [ch, cw], their upsampling
    ratios rh[c], rv[c] (1, 2 or 4) and a rectangle (x, y, w, h) of the upsampled picture -> ndarray [h, w, 3] uint8, the "libjpeg"
    pixels of that rectangle."""
    n = len(planes)
    pl = [np.ascontiguousarray(q, np.uint8) for q in planes]
    ptrs = (_P(ctypes.c_uint8) * n)(*[q.ctypes.data_as(_P(ctypes.c_uint8)) for q in pl])
    cw = (ctypes.c_uint32 * n)(*[q.shape[1] for q in pl])
    ch = (ctypes.c_uint32 * n)(*[q.shape[0] for q in pl])
    a_rh = (ctypes.c_uint8 * n)(*[int(v) for v in rh])
    a_rv = (ctypes.c_uint8 * n)(*[int(v) for v in rv])
    x, y, w, h = (int(v) for v in rect)
    r = Rect(x, y, w, h)
    out = np.zeros((max(h, 1), max(w, 1), 3), np.uint8)
    _check(lib().mjx_upsample_color_host(ptrs, cw, ch, a_rh, a_rv, n, ctypes.byref(r), out.ctypes.data_as(_P(ctypes.c_uint8))), "mjx_upsample_color_host")
    return out[:h, :w]


def upsample_luma_host(plane, rh, rv, rect):
    """mjx_upsample_luma_host (host only; the routine k_upsample_luma runs): one uint8 plane [ch, cw], its upsampling ratios (1, 2 or 4)
    and a rectangle (x, y, w, h) of the upsampled plane -> ndarray [h, w] uint8, the "libjpeg" luminance of that rectangle."""
    pl = np.ascontiguousarray(plane, np.uint8)
    x, y, w, h = (int(v) for v in rect)
    r = Rect(x, y, w, h)
    out = np.zeros((max(h, 1), max(w, 1)), np.uint8)
    _check(lib().mjx_upsample_luma_host(pl.ctypes.data_as(_P(ctypes.c_uint8)), pl.shape[1], pl.shape[0], int(rh), int(rv), ctypes.byref(r),
                                        out.ctypes.data_as(_P(ctypes.c_uint8))), "mjx_upsample_luma_host")
    return out[:h, :w]


def idct_reduced_host(coef, q, n):
    """mjx_idct_reduced_host (host only; the lane routines of the integer inverse DCT at a reduced scale): one block's 64 coefficients
    (int16) and raw DQT entries (uint16), [8, 8] in natural order, and the transform's size n (8, 4, 2 or 1) -> ndarray [n, n] uint8."""
    c = np.ascontiguousarray(coef, dtype=np.int16).reshape(64)
    t = np.ascontiguousarray(q, dtype=np.uint16).reshape(64)
    out = np.empty((int(n), int(n)), np.uint8)
    _check(lib().mjx_idct_reduced_host(c.ctypes.data_as(_P(ctypes.c_int16)), t.ctypes.data_as(_P(ctypes.c_uint16)), int(n),
                                       out.ctypes.data_as(_P(ctypes.c_uint8))), "mjx_idct_reduced_host")
    return out


def idct_islow_host(coef, q):
    """mjx_idct_islow_host (host only; the lane routine stage B's integer sink runs): one block's 64 coefficients (int16) and its 64
    raw DQT entries (uint16), both [8, 8] in natural order -> ndarray [8, 8] uint8, the samples of idct="islow"."""
    c = np.ascontiguousarray(coef, np.int16).reshape(64)
    t = np.ascontiguousarray(q, np.uint16).reshape(64)
    out = np.zeros(64, np.uint8)
    _check(lib().mjx_idct_islow_host(c.ctypes.data_as(_P(ctypes.c_int16)), t.ctypes.data_as(_P(ctypes.c_uint16)),
                                     out.ctypes.data_as(_P(ctypes.c_uint8))), "mjx_idct_islow_host")
    return out.reshape(8, 8)


def _out_ref(output):
    if output is None:
        return None, None
    d = output.desc() if isinstance(output, Output) else output
    return d, ctypes.byref(d)


# ---- host parse ------------------------------------------------------------------------------------
class ParsedScan:
    """Owns one mjx_scan_desc filled by mjx_parse (reference: the state JPEGImage::parse hands to JPEGDecoder)."""

    def __init__(self, data, strict_ref=False, device_destuff=False, color=None, progressive=False):
        """color: "file" -- four-component files parse, and desc.model says what the components are (see Batch)."""
        self.desc = ScanDesc()
        self._owned = False
        o = _opts(strict_ref=strict_ref, device_destuff=device_destuff, color=color, progressive=progressive)
        _check(lib().mjx_parse(bytes(data), len(data), ctypes.byref(o), ctypes.byref(self.desc)), "mjx_parse")
        self._owned = True

    def scan_bytes(self):
        return ctypes.string_at(self.desc.scan, self.desc.scan_len)

    def validate(self, layout=LAYOUT_STANDARD, strict_ref=False, scale=1, roi=None, pixels=None, color=None, progressive=False, idct=None):
        """Status mjx_batch_create would give this image (host only).  roi: (x, y, w, h) in the scaled picture's coordinates."""
        o = _opts(layout=layout, strict_ref=strict_ref, scale=scale, rois=roi, pixels=pixels, idct=idct, color=color, progressive=progressive)
        return int(lib().mjx_validate(ctypes.byref(self.desc), ctypes.byref(o)))

    def plan_tiles(self, roi=None, scale=1, pixels=None, color=None, progressive=False, idct=None):
        """mjx_plan_tiles (host only) -> dict(tiles_read, tiles_total, tile_mcus): the stage-B tiles a decode with this rectangle
        fetches and transforms, of the picture's tiles, and the MCUs a tile holds."""
        o = _opts(scale=scale, rois=roi, pixels=pixels, idct=idct, color=color, progressive=progressive)
        rd, tot, t = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        _check(lib().mjx_plan_tiles(ctypes.byref(self.desc), ctypes.byref(o), ctypes.byref(rd), ctypes.byref(tot), ctypes.byref(t)), "mjx_plan_tiles")
        return dict(tiles_read=rd.value, tiles_total=tot.value, tile_mcus=t.value)

    def plan_reduced(self, scale=1, pixels="libjpeg-exact", idct=None, color=None, progressive=False):
        """mjx_plan_reduced (host only) -> [dict(size, plane_w, plane_h, rh, rv, stride, replicated)] per component: the planner's geometry
        of the exact pixels' planes at this scale -- the transform size libjpeg picks, the plane's samples, its upsampling ratios."""
        o = _opts(scale=scale, pixels=pixels, idct=idct, color=color, progressive=progressive)
        n = ctypes.c_uint32()
        arr = [(ctypes.c_uint32 * 3)() for _ in range(7)]
        _check(lib().mjx_plan_reduced(ctypes.byref(self.desc), ctypes.byref(o), ctypes.byref(n), *arr), "mjx_plan_reduced")
        keys = ("size", "plane_w", "plane_h", "rh", "rv", "stride", "replicated")
        return [{k: int(a[c]) for k, a in zip(keys, arr)} for c in range(n.value)]

    def output_layout(self, output=None, i=0, roi=None, scale=1, layout=LAYOUT_STANDARD, color=None, progressive=False):
        """mjx_output_layout (host only) -> dict(width, height, row_pitch, plane_pitch, bytes, dev): what a decode of this picture
        as input i of a call with this Output would write; pitches in elements, bytes from the first element to the last."""
        o = _opts(layout=layout, scale=scale, rois=roi, color=color, progressive=progressive)
        keep, ref = _out_ref(output)
        lay, nb = Dst(), _sz()
        _check(lib().mjx_output_layout(ctypes.byref(self.desc), ctypes.byref(o), ref, int(i), ctypes.byref(lay), ctypes.byref(nb)), "mjx_output_layout")
        return dict(width=lay.width, height=lay.height, row_pitch=lay.row_pitch, plane_pitch=lay.plane_pitch, bytes=nb.value, dev=lay.dev or 0)

    def planes_layout(self, planes, i=0, roi=None, scale=1, layout=LAYOUT_STANDARD, pixels=None, strict_ref=False, color=None, progressive=False,
                      resize=None, code=None, idct=None):
        """mjx_planes_layout (host only) -> dict(nplanes, width, height, row_pitch, dev -- a list of three each --, bytes): the planes a
        decode of this picture as input i of a call with this Planes would write; pitches in elements, sizes in samples.
        resize (a Resize) and / or code (the resolved orientation, 1 .. 8): mjx_planes_orient_layout -- the planes that LEAVE such a
        call (roi in the turned picture's coordinates, full size with auto_scale), and on top of the keys above `scale`, the scale the
        picture is decoded at, and `rect` = (x, y, w, h), the rectangle of the stored picture its intermediate covers."""
        o = _opts(layout=layout, scale=scale, rois=roi, pixels=pixels, idct=idct, strict_ref=strict_ref, color=color, progressive=progressive)
        keep, ref = _planes_ref(planes)
        if resize is not None or code is not None:
            keep_rs, rs_ref = _rs_ref(resize)
            lay, s, r = PlaneLayout(), ctypes.c_uint8(), Rect()
            _check(lib().mjx_planes_orient_layout(ctypes.byref(self.desc), ctypes.byref(o), ref, rs_ref, 1 if code is None else int(code), int(i),
                                                  ctypes.byref(lay), ctypes.byref(s), ctypes.byref(r)), "mjx_planes_orient_layout")
            d = keep
            ncomp = int(self.desc.ncomp)
            il = bool(d.interleave_chroma) and ncomp == 3
            nplanes = 1 if ncomp == 1 else 2 if il else 3
            esz = (1, 2, 4)[d.dtype]
            total = sum(((lay.height[c] - 1) * lay.row_pitch[c] + lay.width[c] * (2 if il and c == 1 else 1)) * esz for c in range(nplanes))
            return dict(nplanes=nplanes, width=list(lay.width), height=list(lay.height), row_pitch=list(lay.row_pitch),
                        dev=[v or 0 for v in lay.dev], bytes=total, scale=s.value, rect=(r.x, r.y, r.w, r.h))
        lay, np_, nb = PlaneLayout(), ctypes.c_uint32(), _sz()
        _check(lib().mjx_planes_layout(ctypes.byref(self.desc), ctypes.byref(o), ref, int(i), ctypes.byref(lay), ctypes.byref(np_), ctypes.byref(nb)), "mjx_planes_layout")
        return dict(nplanes=np_.value, width=list(lay.width), height=list(lay.height), row_pitch=list(lay.row_pitch),
                    dev=[v or 0 for v in lay.dev], bytes=nb.value)

    def resize_plan(self, resize, roi=None, scale=1, i=0, layout=LAYOUT_STANDARD, pixels=None, idct=None):
        """mjx_resize_plan (host only) -> dict(scale, rect=(x, y, w, h) at that scale, taps_x, taps_y): what a resized decode of this
        picture with this Resize takes; roi in full-size coordinates with auto_scale, else in the scaled picture's."""
        o = _opts(layout=layout, scale=scale, rois=roi, pixels=pixels, idct=idct)
        keep, ref = _rs_ref(resize)
        s, r, tx, ty = ctypes.c_uint8(), Rect(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().mjx_resize_plan(ctypes.byref(self.desc), ctypes.byref(o), ref, int(i), ctypes.byref(s), ctypes.byref(r), ctypes.byref(tx), ctypes.byref(ty)), "mjx_resize_plan")
        return dict(scale=s.value, rect=(r.x, r.y, r.w, r.h), taps_x=tx.value, taps_y=ty.value)

    def fit_plan(self, resize, output=None, code=1, roi=None, scale=1, i=0, layout=LAYOUT_STANDARD):
        """mjx_resize_fit_plan (host only) -> dict(inner=(x, y, w, h), asked=(x, y, w, h), scale): the inner rectangle of the target this
        picture fills under this Resize's fit mode (the whole target unless the mode is "contain"), the rectangle asked for -- roi or the
        whole picture, for "cover" its centred part -- in the coordinates of the oriented picture (full size with auto_scale, else at the
        call's scale), and the scale the picture is decoded at.  A source point (px, py) in asked's coordinates lies at
        inner.x + (px - asked.x) * inner.w / asked.w, inner.y + (py - asked.y) * inner.h / asked.h of the output."""
        o = _opts(layout=layout, scale=scale, rois=roi)
        keep, ref = _rs_ref(resize)
        keep_o, oref = _out_ref(output)
        inner, asked, s = Rect(), Rect(), ctypes.c_uint8()
        _check(lib().mjx_resize_fit_plan(ctypes.byref(self.desc), ctypes.byref(o), oref, ref, int(code), int(i), ctypes.byref(inner),
                                         ctypes.byref(asked), ctypes.byref(s)), "mjx_resize_fit_plan")
        return dict(inner=(inner.x, inner.y, inner.w, inner.h), asked=(asked.x, asked.y, asked.w, asked.h), scale=s.value)

    def orient_plan(self, code, resize=None, roi=None, scale=1, i=0, layout=LAYOUT_STANDARD):
        """mjx_orient_plan (host only) -> dict(width, height, stored_rect=(x, y, w, h), scale): the picture that leaves when this one is
        decoded with orientation code `code` (roi in the oriented picture's coordinates), and what is decoded for it."""
        o = _opts(layout=layout, scale=scale, rois=roi)
        keep, ref = _rs_ref(resize)
        w, h, r, s = ctypes.c_uint32(), ctypes.c_uint32(), Rect(), ctypes.c_uint8()
        _check(lib().mjx_orient_plan(ctypes.byref(self.desc), ctypes.byref(o), ref, int(code), int(i), ctypes.byref(w), ctypes.byref(h),
                                     ctypes.byref(r), ctypes.byref(s)), "mjx_orient_plan")
        return dict(width=w.value, height=h.value, stored_rect=(r.x, r.y, r.w, r.h), scale=s.value)

    def close(self):
        if self._owned:
            lib().mjx_free_scan(ctypes.byref(self.desc))
            self._owned = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- device context / batch ----------------------------------------------------------------------------
class Context:
    def __init__(self, device=0, profiling=False, throughput_plan=False):
        """throughput_plan: batches are always cut into 512-byte subsequences (for a small base that Batch.tile replicates)."""
        self.h = _vp()
        self.device = int(device)
        _check(lib().mjx_ctx_create(int(device), ctypes.byref(self.h)), "mjx_ctx_create(device=%d)" % device)
        if profiling:
            self.set_profiling(True)
        if throughput_plan:
            _check(lib().mjx_ctx_set_throughput_plan(self.h, 1))

    def set_profiling(self, on):
        _check(lib().mjx_ctx_set_profiling(self.h, int(bool(on))))

    def close(self):
        if self.h:
            lib().mjx_ctx_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        # not during interpreter shutdown: the HIP runtime may already be gone (its teardown aborts the process when a
        # device handle is released after it); the driver reclaims everything at exit anyway
        if sys is None or sys.is_finalizing():          # (at interpreter shutdown module globals may be gone already)
            return
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """Device-resident batch: inputs uploaded at construction, ``decode()`` only enqueues kernels."""

    def __init__(self, ctx, scans=None, strict_ref=False, layout=LAYOUT_STANDARD, keep_coefs=False, chunk_images=0,
                 _handle=None, scale=1, rois=None, output=None, resize=None, orient=None, datas=None, pixels=None, planes=None, color=None, progressive=False, idct=None):
        """scale: 1, 2, 4 or 8 -- every picture decoded at 1/scale (info(), rgb(), rgb_device() and bytes() then speak of the
        scaled picture; tile() keeps the scale).
        rois: one (x, y, w, h) for every picture, or a list with one per picture (None or (0, 0, 0, 0): the whole picture), in the
        coordinates of the scaled picture -- info(), rgb(), rgb_device(), bytes() and compare_rgb() then speak of the cropped
        picture, roi(i) says where it lies; tile() keeps the rectangles.
        output: an Output -- the pictures leave in that format (output(i), output_info(i); rgb() and compare_rgb() do not serve
        such a batch), in the batch's memory or, Output(dst=...), in device memory of the caller's: idle when decode() is called,
        complete when wait() returns.
        resize: a Resize -- every picture leaves at its width x height, through `output` (None: interleaved uint8); info(),
        output_info() and output() speak of the target picture, scale(i) and rect(i) of what was decoded for it.
        orient: an Orient -- every picture leaves turned (orientation(i): by which code), rois are in the coordinates of the turned
        picture, info(), output_info() and output() speak of it, roi(i) and rect(i) of the stored picture.  Parsed scans hold no
        EXIF segment: with Orient(exif=True) pass the files' bytes as `datas`, and the tags are read from them here.
        pixels: "libjpeg" (PIXELS_LIBJPEG) -- the pictures libjpeg-based decoders give: rounded samples, fancy chroma upsampling,
        integer colour tables (STANDARD layout at full size only); everything above composes with it; tile() keeps it.
        planes: a Planes -- the pictures leave as their component planes (planes(i), plane_info(i)); scale, rois and pixels apply,
        output does not go with it; tile() keeps it.  With resize and / or orient (mjx_batch_create_planes_orient) every plane is
        turned and resampled to its own share of the target: planes(i) and plane_info(i) give the planes that leave, info(i) the
        picture that leaves, scale(i), roi(i) and rect(i) what was decoded for it, orientation(i) the code; fit="contain" is refused.
        color: "file" (COLOR_FILE) -- what a file's components are comes from the file (JFIF / Adobe segments, component ids:
        mjx.h, mjx_opts.color): RGB, CMYK and YCCK files decode to R,G,B (color_model(i) says which a picture was); the scans must
        have been parsed with color="file" too.  Luminance output, planes and pixels="libjpeg" refuse such pictures
        (ERR_UNSUPPORTED_FORMAT); YCbCr and grey pictures are unchanged.  Default: three components are Y, Cb, Cr by position."""
        self.ctx = ctx
        self.h = _vp()
        if _handle is not None:
            self.h = _handle
            return
        n = len(scans)
        arr = (ScanDesc * max(n, 1))()
        for i, s in enumerate(scans):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(s.desc if isinstance(s, ParsedScan) else s),
                           ctypes.sizeof(ScanDesc))
        st = (_int * max(n, 1))()
        o = _opts(strict_ref, layout, keep_coefs, chunk_images, scale=scale, rois=rois, pixels=pixels, idct=idct, color=color, progressive=progressive)
        keep, ref = _out_ref(output)
        if planes is not None and (resize is not None or orient is not None):
            if output is not None:
                raise MjxError(ERR_INVALID_ARG, "planes go without output")
            keep_pl, pl_ref = _planes_ref(planes)
            keep_rs, rs_ref = _rs_ref(resize)
            od_ref = None
            if orient is not None:
                if orient.exif:
                    if datas is None or len(datas) != n:
                        raise MjxError(ERR_INVALID_ARG, "Orient(exif=True) needs the files' bytes: datas")
                    extra = orient.codes(n) or [1] * n
                    if len(extra) != n:
                        raise MjxError(ERR_INVALID_ARG, "Orient(extra=...): %d codes for %d pictures" % (len(extra), n))
                    orient = Orient(False, [orient_compose(exif_orientation(d), e) if 1 <= e <= 8 else e for d, e in zip(datas, extra)])
                keep_or, od = orient.desc(n, exif=False)
                od_ref = ctypes.byref(od)
            _check(lib().mjx_batch_create_planes_orient(ctx.h, arr, n, ctypes.byref(o), pl_ref, rs_ref, od_ref, ctypes.byref(self.h), st),
                   "mjx_batch_create_planes_orient")
        elif planes is not None:
            if output is not None:
                raise MjxError(ERR_INVALID_ARG, "planes go without output")
            keep_pl, pl_ref = _planes_ref(planes)
            _check(lib().mjx_batch_create_planes(ctx.h, arr, n, ctypes.byref(o), pl_ref, ctypes.byref(self.h), st), "mjx_batch_create_planes")
        elif orient is not None:
            if orient.exif:
                if datas is None or len(datas) != n:
                    raise MjxError(ERR_INVALID_ARG, "Orient(exif=True) needs the files' bytes: datas")
                extra = orient.codes(n) or [1] * n
                if len(extra) != n:
                    raise MjxError(ERR_INVALID_ARG, "Orient(extra=...): %d codes for %d pictures" % (len(extra), n))
                orient = Orient(False, [orient_compose(exif_orientation(d), e) if 1 <= e <= 8 else e for d, e in zip(datas, extra)])
            keep_rs, rs_ref = _rs_ref(resize)
            keep_or, od = orient.desc(n, exif=False)
            _check(lib().mjx_batch_create_orient(ctx.h, arr, n, ctypes.byref(o), ref, rs_ref, ctypes.byref(od), ctypes.byref(self.h), st), "mjx_batch_create_orient")
        elif resize is not None:
            keep_rs, rs_ref = _rs_ref(resize)
            _check(lib().mjx_batch_create_resize(ctx.h, arr, n, ctypes.byref(o), ref, rs_ref, ctypes.byref(self.h), st), "mjx_batch_create_resize")
        else:
            _check(lib().mjx_batch_create_out(ctx.h, arr, n, ctypes.byref(o), ref, ctypes.byref(self.h), st), "mjx_batch_create_out")
        self.create_status = list(st)[:n]

    def tile(self, times):
        h = _vp()
        _check(lib().mjx_batch_tile(self.ctx.h, self.h, int(times), ctypes.byref(h)), "mjx_batch_tile")
        return Batch(self.ctx, _handle=h)

    def decode(self, stages=STAGE_ALL):
        _check(lib().mjx_batch_decode(self.h, int(stages)), "mjx_batch_decode")

    def wait(self):
        _check(lib().mjx_batch_wait(self.h), "mjx_batch_wait")

    def __len__(self):
        return int(lib().mjx_batch_size(self.h))

    def status(self, i):
        return int(lib().mjx_batch_status(self.h, i))

    def info(self, i):
        v = [ctypes.c_uint32() for _ in range(4)]
        lib().mjx_batch_image_info(self.h, i, *[ctypes.byref(x) for x in v])
        return dict(width=v[0].value, height=v[1].value, bpm=v[2].value, mcus=v[3].value)

    def roi(self, i):
        """Where picture i lies in the uncropped picture: dict(x, y, w, h, full_width, full_height)."""
        v = [ctypes.c_uint32() for _ in range(4)]
        lib().mjx_batch_image_roi(self.h, i, *[ctypes.byref(x) for x in v])
        inf = self.info(i)
        return dict(x=v[0].value, y=v[1].value, w=inf["width"], h=inf["height"], full_width=v[2].value, full_height=v[3].value)

    def scale(self, i):
        """The DCT-domain scale picture i was decoded at: the call's, or the one Resize(auto_scale=True) picked."""
        v = ctypes.c_uint8()
        lib().mjx_batch_image_scale(self.h, i, ctypes.byref(v))
        return v.value

    def color_model(self, i):
        """The colour model of picture i: MODEL_GREY, MODEL_YCBCR, MODEL_RGB, MODEL_CMYK or MODEL_YCCK (MODEL_NAMES)."""
        v = ctypes.c_uint8(0)
        lib().mjx_batch_image_color(self.h, i, ctypes.byref(v))
        return v.value

    def orientation(self, i):
        """The orientation code picture i left with: the file's tag followed by its extra code (1: as stored)."""
        v = ctypes.c_uint8(1)
        lib().mjx_batch_image_orientation(self.h, i, ctypes.byref(v))
        return v.value

    def rect(self, i):
        """(x, y, w, h) of what was decoded for picture i, in the coordinates of the picture at scale(i) (roi(i): its size)."""
        r = Rect()
        lib().mjx_batch_resize_rect(self.h, i, ctypes.byref(r))
        return (r.x, r.y, r.w, r.h)

    def fit_rect(self, i):
        """mjx_batch_fit_rect -> (x, y, w, h): the inner rectangle of picture i's target, the part the picture fills -- the whole target
        for Resize(fit="stretch") and "cover", the letterboxed part for "contain"; zeros for a batch without a resize.  With
        ParsedScan.fit_plan's `asked` a source point maps to inner.x + (px - asked.x) * inner.w / asked.w, likewise in y."""
        r = Rect()
        lib().mjx_batch_fit_rect(self.h, i, ctypes.byref(r))
        return (r.x, r.y, r.w, r.h)

    def rgb(self, i):
        inf = self.info(i)
        out = np.empty((inf["height"], inf["width"], 3), np.uint8)
        _check(lib().mjx_batch_copy_rgb(self.h, i, out.ctypes.data_as(_vp)), "mjx_batch_copy_rgb")
        return out

    def output_info(self, i):
        """mjx_batch_output_info and mjx_batch_output_channels -> dict(dev, width, height, row_pitch, plane_pitch, dtype, planar, bgr,
        channels); pitches in elements."""
        lay = Dst()
        v = [ctypes.c_uint8() for _ in range(4)]
        _check(lib().mjx_batch_output_info(self.h, i, ctypes.byref(lay), *[ctypes.byref(x) for x in v[:3]]), "mjx_batch_output_info")
        _check(lib().mjx_batch_output_channels(self.h, i, ctypes.byref(v[3])), "mjx_batch_output_channels")
        return dict(dev=lay.dev or 0, width=lay.width, height=lay.height, row_pitch=lay.row_pitch, plane_pitch=lay.plane_pitch,
                    dtype=v[0].value, planar=bool(v[1].value), bgr=bool(v[2].value), channels=v[3].value)

    def output(self, i):
        """Picture i's library-owned output as an ndarray of its dtype: [3, H, W] (planar) or [H, W, 3]; a luminance picture [1, H, W] or
        [H, W, 1] as the call's Output said (the memory is the same)."""
        inf = self.output_info(i)
        if inf["channels"] == 1:
            shape = (1, inf["height"], inf["width"]) if inf["planar"] else (inf["height"], inf["width"], 1)
        else:
            shape = (3, inf["height"], inf["width"]) if inf["planar"] else (inf["height"], inf["width"], 3)
        out = np.empty(shape, _NP_DTYPES[inf["dtype"]])
        _check(lib().mjx_batch_copy_output(self.h, i, out.ctypes.data_as(_vp), out.nbytes), "mjx_batch_copy_output")
        return out

    def plane_info(self, i):
        """mjx_batch_plane_info -> dict(nplanes, dev, row_pitch, width, height -- lists of three --, dtype, interleave)."""
        lay, np_, dt, il = PlaneLayout(), ctypes.c_uint32(), ctypes.c_uint8(), ctypes.c_uint8()
        _check(lib().mjx_batch_plane_info(self.h, i, ctypes.byref(np_), ctypes.byref(lay), ctypes.byref(dt), ctypes.byref(il)), "mjx_batch_plane_info")
        return dict(nplanes=np_.value, dev=[v or 0 for v in lay.dev], row_pitch=list(lay.row_pitch), width=list(lay.width), height=list(lay.height),
                    dtype=dt.value, interleave=bool(il.value))

    def planes(self, i):
        """Picture i's library-owned planes as a tuple of ndarrays of the planes' dtype: (Y,), (Y, Cb, Cr), each [h_c, w_c], or with
        interleaved chroma (Y, CbCr) with CbCr [h, w, 2]."""
        inf = self.plane_info(i)
        dt = np.dtype(_NP_DTYPES[inf["dtype"]])
        shapes = [(inf["height"][c], inf["width"][c]) for c in range(inf["nplanes"])]
        if inf["interleave"]:
            shapes[1] = shapes[1] + (2,)
        counts = [int(np.prod(sh)) for sh in shapes]
        buf = np.empty(sum(counts), dt)
        _check(lib().mjx_batch_copy_planes(self.h, i, buf.ctypes.data_as(_vp), buf.nbytes), "mjx_batch_copy_planes")
        out, at = [], 0
        for sh, cnt in zip(shapes, counts):
            out.append(buf[at:at + cnt].reshape(sh))
            at += cnt
        return tuple(out)

    def rgb_device(self, i):
        p, n = _vp(), _sz()
        _check(lib().mjx_batch_rgb_device(self.h, i, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def coefs(self, i):
        """T0 stream of image i: int16 [blocks, 64], MCU-interleaved decode order, zig-zag, DC predicted."""
        inf = self.info(i)
        nb = inf["bpm"] * inf["mcus"]
        out = np.empty((nb, 64), np.int16)
        got = _sz()
        _check(lib().mjx_batch_copy_coefs(self.h, i, out.ctypes.data_as(_vp), nb, ctypes.byref(got)), "copy_coefs")
        return out

    def compare_rgb(self, mine, other, theirs):
        """On-device comparison of picture mine[k] with picture theirs[k] of batch `other` (may be self):
        -> (max |difference| per pair as uint32 array, 0xffffffff = sizes differ / a picture failed; differing bytes per pair)."""
        n = len(mine)
        assert n == len(theirs)
        ia = (_sz * max(n, 1))(*[int(x) for x in mine])
        ib = (_sz * max(n, 1))(*[int(x) for x in theirs])
        mx = np.zeros(max(n, 1), np.uint32)
        cnt = np.zeros(max(n, 1), np.uint64)
        _check(lib().mjx_batch_compare_rgb(self.h, ia, other.h, ib, n, mx.ctypes.data_as(_P(ctypes.c_uint32)),
                                           cnt.ctypes.data_as(_P(ctypes.c_uint64))), "mjx_batch_compare_rgb")
        return mx[:n], cnt[:n]

    def bytes(self):
        v = [ctypes.c_uint64() for _ in range(4)]
        _check(lib().mjx_batch_bytes(self.h, *[ctypes.byref(x) for x in v]))
        return dict(scan=v[0].value, rgb=v[1].value, coef=v[2].value, pixels=v[3].value)

    def geometry(self):
        v = [ctypes.c_uint64() for _ in range(3)]
        _check(lib().mjx_batch_geometry(self.h, *[ctypes.byref(x) for x in v]))
        return dict(subsequences=v[0].value, blocks=v[1].value, chunks=v[2].value)

    def unconverged_runs(self):
        """Chunk runs since creation whose synchronisation had not converged in time (their pictures were skipped in that run; wait()
        repairs the last decode only): a throughput loop that enqueues several decodes before one wait checks this stays put."""
        v = ctypes.c_uint64()
        _check(lib().mjx_batch_unconverged_runs(self.h, ctypes.byref(v)))
        return v.value

    def kernel_ms(self, reset=False):
        ms = (ctypes.c_double * len(KERNEL_NAMES))()
        cnt = (ctypes.c_uint64 * len(KERNEL_NAMES))()
        _check(lib().mjx_batch_kernel_ms(self.h, ms, cnt, int(reset)))
        return {k: (ms[i], int(cnt[i])) for i, k in enumerate(KERNEL_NAMES)}

    def close(self):
        if self.h:
            lib().mjx_batch_free(self.h)
            self.h = _vp()

    def __del__(self):
        # not during interpreter shutdown: the HIP runtime may already be gone (its teardown aborts the process when a
        # device handle is released after it); the driver reclaims everything at exit anyway
        if sys is None or sys.is_finalizing():          # (at interpreter shutdown module globals may be gone already)
            return
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ---- mirror of the reference's interface ------------------------------------------------------------------
class HuffmanTable:
    """HuffmanTable::from_size_data_tables (src/jpeg/huffman.rs:37): keeps the DHT slices; codes are built in C++."""

    def __init__(self, size_data, data_table):
        self.size_data = bytes(size_data)
        self.data_table = bytes(data_table)
        if len(self.size_data) != 16:
            raise ValueError("size_data must hold 16 counts")

    @staticmethod
    def from_size_data_tables(size_data, data_table):
        return HuffmanTable(size_data, data_table)


class FrameComponentHeader:  # src/jpeg/mod.rs:104-113
    def __init__(self, component_id, horizontal_sampling_factor, vertical_sampling_factor, quantization_selector):
        self.component_id = component_id
        self.horizontal_sampling_factor = horizontal_sampling_factor
        self.vertical_sampling_factor = vertical_sampling_factor
        self.quantization_selector = quantization_selector


class FrameHeader:  # src/jpeg/mod.rs:90-101
    def __init__(self, sample_precision, num_lines, samples_per_line, frame_components):
        self.sample_precision = sample_precision
        self.num_lines = num_lines
        self.samples_per_line = samples_per_line
        self.image_components = len(frame_components)
        self.frame_components = list(frame_components)


class ScanComponentHeader:  # src/jpeg/mod.rs:132-139
    def __init__(self, component_id, dc_table_selector, ac_table_selector):
        self.component_id = component_id
        self.dc_table_selector = dc_table_selector
        self.ac_table_selector = ac_table_selector


class ScanHeader:  # src/jpeg/mod.rs:116-129
    def __init__(self, scan_components):
        self.num_components = len(scan_components)
        self.scan_components = list(scan_components)


class JPEGDecoder:
    """Builder with the reference's method names (src/jpeg/decoder.rs:55-162); decode() runs on the GPU."""

    def __init__(self, data):
        self.data = bytes(data)
        self._frame = None
        self._scan = None
        self._dims = (0, 0)
        self._ac, self._dc, self._qt = {}, {}, {}
        self.layout = LAYOUT_STANDARD

    def dimensions(self, dims):
        self._dims = (int(dims[0]), int(dims[1]))
        return self

    def frame_header(self, frame_header):
        self._frame = frame_header
        return self

    def scan_header(self, scan_header):
        self._scan = scan_header
        return self

    def huffman_ac_tables(self, ident, table):
        self._ac[int(ident)] = table

    def huffman_dc_tables(self, ident, table):
        self._dc[int(ident)] = table

    def quantization_table(self, ident, table):
        self._qt[int(ident)] = [int(v) for v in table]

    def _desc(self):
        d = ScanDesc()
        self._buf = (ctypes.c_uint8 * (len(self.data) + 32)).from_buffer_copy(self.data + b"\xaa" * 32)
        d.scan = ctypes.cast(self._buf, ctypes.POINTER(ctypes.c_uint8))
        d.scan_len = len(self.data)
        d.width, d.height = self._dims
        if self._frame is None or self._scan is None:
            raise MjxError(ERR_REF_PANIC, "frame_header/scan_header missing (reference: unwrap on None)")
        d.ncomp = self._scan.num_components
        if d.ncomp not in (1, 3):
            raise MjxError(ERR_UNSUPPORTED_FORMAT)
        for i, sc in enumerate(self._scan.scan_components):      # scan order, decoder.rs:141-150
            fc = [f for f in self._frame.frame_components if f.component_id == sc.component_id]
            if not fc:
                raise MjxError(ERR_REF_PANIC, "scan component not in frame")
            d.comp[i] = Comp(sc.component_id, fc[0].horizontal_sampling_factor, fc[0].vertical_sampling_factor,
                             fc[0].quantization_selector, sc.dc_table_selector, sc.ac_table_selector)
        for k, t in self._qt.items():
            for j in range(64):
                d.qt[k][j] = t[j]
            d.qt_present |= 1 << k
        for store, present, tabs in ((d.dc, "dc_present", self._dc), (d.ac, "ac_present", self._ac)):
            for k, t in tabs.items():
                for j in range(16):
                    store[k].bits[j] = t.size_data[j]
                for j, v in enumerate(t.data_table[:256]):
                    store[k].vals[j] = v
                setattr(d, present, getattr(d, present) | (1 << k))
        return d

    def decode(self, ctx=None):
        """-> (rgb ndarray [H, W, 3] uint8, bytes_read).  bytes_read is bookkeeping the reference's caller ignores
        (src/jpeg/mod.rs:415-417); it is reported as the scan length."""
        ctx = ctx or default_context()
        b = Batch(ctx, [self._desc()], layout=self.layout)
        try:
            if b.create_status[0] != OK:
                raise MjxError(b.create_status[0])
            b.decode()
            b.wait()
            if b.status(0) != OK:
                raise MjxError(b.status(0))
            return b.rgb(0), len(self.data)
        finally:
            b.close()


class JPEGImage:
    """JPEGImage::parse (src/jpeg/mod.rs:202) -> width() :467, height() :471, image_data() :475."""

    def __init__(self, width, height, rgb):
        self._w, self._h, self._rgb = width, height, rgb

    @staticmethod
    def parse(data, strict_ref=False, layout=LAYOUT_STANDARD, ctx=None, scale=1, roi=None, pixels=None, color=None, progressive=False, idct=None):
        """scale: 1, 2, 4 or 8 -- the picture at 1/scale (width() and height() are the scaled picture's).
        roi: (x, y, w, h) of the scaled picture -- only that rectangle is produced (width() and height() are its).
        pixels: "libjpeg", color: "file" -- see Batch."""
        ctx = ctx or default_context()
        scan = ParsedScan(data, strict_ref=strict_ref, color=color, progressive=progressive)
        try:
            b = Batch(ctx, [scan], strict_ref=strict_ref, layout=layout, scale=scale, rois=roi, pixels=pixels, idct=idct, color=color, progressive=progressive)
            try:
                if b.create_status[0] != OK:
                    raise MjxError(b.create_status[0])
                b.decode()
                b.wait()
                if b.status(0) != OK:
                    raise MjxError(b.status(0))
                rgb = b.rgb(0)
                return JPEGImage(rgb.shape[1], rgb.shape[0], rgb)
            finally:
                b.close()
        finally:
            scan.close()

    def width(self):
        return self._w

    def height(self):
        return self._h

    def image_data(self):
        """ndarray [H, W, 3] uint8 (the reference returns Option<&Vec<(u8,u8,u8)>> of length W*H, row-major)."""
        return self._rgb


def decode_batch(ctx, datas, strict_ref=False, layout=LAYOUT_STANDARD, threads=0, device_destuff=None, keep_coefs=False, scale=1, rois=None,
                 output=None, chunk_images=0, resize=None, orient=None, pixels=None, planes=None, color=None, progressive=False, idct=None):
    """mjx_decode_batch: parse (host threads) + GPU decode of a list of files -> (Batch, [status per file]).  scale, rois, pixels, color: see Batch.
    device_destuff: the host copies the entropy-coded bytes as they are; de-stuffing, restart markers and the scan's length
    are found on the GPU.  output: an Output (mjx_decode_batch_out) -- see Batch.  resize: a Resize (mjx_decode_batch_resize).  orient: an Orient
    (mjx_decode_batch_orient): the files' EXIF orientation and / or a code per file on top.  planes: a Planes (mjx_decode_batch_planes) --
    the pictures leave as their component planes; output does not go with it, resize and orient do (mjx_decode_batch_planes_orient)."""
    n = len(datas)
    arr = (ctypes.c_char_p * max(n, 1))(*[bytes(d) for d in datas])
    lens = (_sz * max(n, 1))(*[len(d) for d in datas])
    st = (_int * max(n, 1))()
    ptrs = (_P(ctypes.c_uint8) * max(n, 1))()
    h = _vp()
    o = _opts(strict_ref, layout, keep_coefs=keep_coefs, chunk_images=chunk_images, device_destuff=device_destuff, scale=scale, rois=rois, pixels=pixels, idct=idct, color=color, progressive=progressive)
    if planes is not None:
        if output is not None:
            raise MjxError(ERR_INVALID_ARG, "planes go without output")
        keep_pl, pl_ref = _planes_ref(planes)
        if resize is not None or orient is not None:
            keep_rs, rs_ref = _rs_ref(resize)
            keep_or, od = orient.desc(n) if orient is not None else (None, None)
            _check(lib().mjx_decode_batch_planes_orient(ctx.h, arr, lens, n, ctypes.byref(o), int(threads), pl_ref, rs_ref,
                                                        ctypes.byref(od) if od is not None else None, st, ctypes.byref(h)), "mjx_decode_batch_planes_orient")
            return Batch(ctx, _handle=h), list(st)[:n]
        _check(lib().mjx_decode_batch_planes(ctx.h, arr, lens, n, ctypes.byref(o), int(threads), pl_ref, st, ctypes.byref(h)), "mjx_decode_batch_planes")
        return Batch(ctx, _handle=h), list(st)[:n]
    if orient is not None:
        keep, ref = _out_ref(output)
        keep_rs, rs_ref = _rs_ref(resize)
        keep_or, od = orient.desc(n)
        _check(lib().mjx_decode_batch_orient(ctx.h, arr, lens, n, ctypes.byref(o), int(threads), ref, rs_ref, ctypes.byref(od), st, ctypes.byref(h)), "mjx_decode_batch_orient")
        return Batch(ctx, _handle=h), list(st)[:n]
    if resize is not None:
        keep, ref = _out_ref(output)
        keep_rs, rs_ref = _rs_ref(resize)
        _check(lib().mjx_decode_batch_resize(ctx.h, arr, lens, n, ctypes.byref(o), int(threads), ref, rs_ref, st, ctypes.byref(h)), "mjx_decode_batch_resize")
        return Batch(ctx, _handle=h), list(st)[:n]
    if output is not None:
        keep, ref = _out_ref(output)
        _check(lib().mjx_decode_batch_out(ctx.h, arr, lens, n, ctypes.byref(o), int(threads), ref, st, ctypes.byref(h)), "mjx_decode_batch_out")
        return Batch(ctx, _handle=h), list(st)[:n]
    _check(lib().mjx_decode_batch(ctx.h, arr, lens, n, ctypes.byref(o), int(threads), ptrs, st, ctypes.byref(h)), "mjx_decode_batch")
    return Batch(ctx, _handle=h), list(st)[:n]


def decode_into(ctx, datas, out, scale=1, rois=None, mean=None, std=None, bgr=False, threads=0, device_destuff=None, planar=None, resize=None,
                orient=None, pixels=None, color=None, progressive=False, pad=0, idct=None):
    """Decodes the files straight into a torch tensor on the context's device: N x 3 x H x W (planar) or N x H x W x 3, of uint8,
    float16 or float32; picture i -- at 1/scale, its rectangle rois[i] -- must be H x W.  Float tensors take (v / 255 - mean) / std
    per OUTPUT channel (see Output); bgr: channel 0 is blue.  The pointers and pitches come from data_ptr() and stride(): the
    innermost dimension must be dense (planar: stride 1 along W; interleaved: stride 1 along the channels and 3 along W), rows
    and planes may be padded, and the pictures must not overlap (the batch stride covers a picture's span).
    planar: True / False says which form the tensor is.  None takes it from the shape: N x 3 x H x W when the second dimension is
    3, N x H x W x 3 when only the last is; a shape that reads both ways (N x 3 x H x 3) needs the keyword.
    Luminance (Output(channels=1)): N x 1 x H x W or N x H x W x 1 -- taken from the shape when neither of the two dimensions is 3;
    N x 1 x H x 1 needs the keyword -- with padded rows; mean / std are then scalars or have one element.
    torch's current stream is synchronised before the call (the library writes on streams of its
    own) and the batch is complete when this returns.  -> the per-picture statuses.
    pad: the border colour of resize=Resize(fit="contain") (Output's pad: one value or three of 0 .. 255, by OUTPUT channel).
    resize: True, or a Resize (its antialias, auto_scale, filter and fit mode; a size, if it names one, must be the tensor's) -- the pictures, of any
    size, are resampled on the device to the tensor's H x W (see Resize); None: every picture must be H x W as it is.
    orient: an Orient -- the pictures are turned on the device (see Orient); H x W and rois speak of the turned pictures.
    pixels: "libjpeg", color: "file" -- see Batch."""
    import torch
    n = len(datas)
    if not isinstance(out, torch.Tensor) or out.dim() != 4 or out.shape[0] != n:
        raise MjxError(ERR_INVALID_ARG, "out: a tensor of %d pictures" % n)
    names = {torch.uint8: DTYPE_U8, torch.float16: DTYPE_F16, torch.float32: DTYPE_F32}
    if out.dtype not in names:
        raise MjxError(ERR_INVALID_ARG, "out.dtype %s" % out.dtype)
    if out.device.type != "cuda" or out.device.index != ctx.device:
        raise MjxError(ERR_INVALID_ARG, "out lies on %s, not on the context's device %d" % (out.device, ctx.device))
    sn, s1, s2, s3 = out.stride()
    channels = 3
    if planar is None:
        if out.shape[1] == 3 and out.shape[3] == 3:
            raise MjxError(ERR_INVALID_ARG, "out: %s reads as 3 x H x W and as H x W x 3: say planar=True or planar=False" % (tuple(out.shape),))
        if out.shape[1] == 3 or out.shape[3] == 3:
            planar = out.shape[1] == 3
        elif out.shape[1] == 1 and out.shape[3] == 1:
            raise MjxError(ERR_INVALID_ARG, "out: %s reads as 1 x H x W and as H x W x 1: say planar=True or planar=False" % (tuple(out.shape),))
        else:
            planar = out.shape[1] == 1
    if planar and out.shape[1] == 1:                 # luminance, 1 x H x W: one element per pixel, rows may be padded
        channels = 1
        h, w = int(out.shape[2]), int(out.shape[3])
        ok = s3 == 1 and s2 >= w
        row_pitch, plane_pitch = s2, 0
        span = (h - 1) * s2 + w
    elif not planar and out.shape[3] == 1:           # luminance, H x W x 1: the same memory
        channels = 1
        h, w = int(out.shape[1]), int(out.shape[2])
        ok = s2 == 1 and s1 >= w
        row_pitch, plane_pitch = s1, 0
        span = (h - 1) * s1 + w
    elif planar and out.shape[1] == 3:
        h, w = int(out.shape[2]), int(out.shape[3])
        ok = s3 == 1 and s2 >= w and s1 >= h * s2
        row_pitch, plane_pitch = s2, s1
        span = 2 * s1 + (h - 1) * s2 + w
    elif not planar and out.shape[3] == 3:
        h, w = int(out.shape[1]), int(out.shape[2])
        ok = s3 == 1 and s2 == 3 and s1 >= 3 * w
        row_pitch, plane_pitch = s1, 0
        span = (h - 1) * s1 + 3 * w
    else:
        raise MjxError(ERR_INVALID_ARG, "out: N x 3 x H x W or N x H x W x 3 (luminance: N x 1 x H x W or N x H x W x 1)")
    if not ok or (n > 1 and sn < span):
        raise MjxError(ERR_INVALID_ARG, "out.stride() %s: neither 3 x H x W nor H x W x 3 with a dense innermost dimension, or the pictures overlap" % (tuple(out.stride()),))
    esz = out.element_size()
    dst = [(out.data_ptr() + i * sn * esz, w, h, row_pitch, plane_pitch) for i in range(n)]
    fmt = Output(names[out.dtype], planar=bool(planar), bgr=bgr, mean=mean, std=std, dst=dst, channels=channels, pad=pad)
    torch.cuda.current_stream(out.device).synchronize()
    if resize is not None and resize is not False:
        rs = Resize(w, h) if resize is True else resize.sized(w, h)
        if resize is not True and (resize.width or resize.height) and (resize.width, resize.height) != (w, h):
            raise MjxError(ERR_INVALID_ARG, "resize to %d x %d into a tensor of %d x %d" % (resize.width, resize.height, w, h))
    else:
        rs = None
    batch, status = decode_batch(ctx, datas, threads=threads, device_destuff=device_destuff, scale=scale, rois=rois, output=fmt, resize=rs, orient=orient, pixels=pixels, idct=idct, color=color, progressive=progressive)
    batch.close()
    return status


def decode_planes_into(ctx, datas, y, cb=None, cr=None, cbcr=None, scale=1, rois=None, mean=None, std=None, threads=0, device_destuff=None, pixels=None,
                       resize=None, orient=None, idct=None):
    """Decodes the files' component planes straight into torch tensors on the context's device: decode_planes_into(ctx, datas, y, cb,
    cr) with y N x Hy x Wy, cb and cr N x Hc x Wc, or decode_planes_into(ctx, datas, y, cbcr=t) with t N x Hc x Wc x 2 (NV12's second
    plane); one-component files take y alone.  All pictures of the call have one size and layout; tensors are of one dtype (uint8,
    float16, float32); the innermost dimension is dense, rows may be padded and the pictures of a tensor must not overlap.  Float
    tensors take (v / 255 - mean) / std per COMPONENT.  torch's current stream is synchronised before the call and the planes are
    complete when this returns.  -> the per-picture statuses.
    resize: True, or a Resize (its antialias, auto_scale, filter and fit mode; a size, if it names one, must be y's) -- the target is
    y's H x W and the files may differ in size; they still share one sampling layout, since the tensors have one chroma size: a
    picture of another layout gets ERR_INVALID_ARG and its slot is untouched.  orient: an Orient -- the planes are turned on the
    device; the tensors' sizes and rois speak of the turned pictures."""
    import torch
    n = len(datas)
    if cbcr is not None and (cb is not None or cr is not None):
        raise MjxError(ERR_INVALID_ARG, "cb and cr, or cbcr")
    tensors = [y] + ([cbcr] if cbcr is not None else [t for t in (cb, cr) if t is not None])
    if (cb is None) != (cr is None):
        raise MjxError(ERR_INVALID_ARG, "cb and cr go together")
    names = {torch.uint8: DTYPE_U8, torch.float16: DTYPE_F16, torch.float32: DTYPE_F32}
    per_plane, sizes = [], []
    for k, t in enumerate(tensors):
        pair = cbcr is not None and k == 1
        if not isinstance(t, torch.Tensor) or t.dim() != (4 if pair else 3) or t.shape[0] != n or (pair and t.shape[3] != 2):
            raise MjxError(ERR_INVALID_ARG, "plane %d: a tensor of %d planes" % (k, n))
        if t.dtype not in names or t.dtype != y.dtype:
            raise MjxError(ERR_INVALID_ARG, "plane %d: dtype %s" % (k, t.dtype))
        if t.device.type != "cuda" or t.device.index != ctx.device:
            raise MjxError(ERR_INVALID_ARG, "plane %d lies on %s, not on the context's device %d" % (k, t.device, ctx.device))
        st = t.stride()
        h, w = int(t.shape[1]), int(t.shape[2])
        row = 2 * w if pair else w
        ok = (st[3] == 1 and st[2] == 2) if pair else st[2] == 1
        if not ok or st[1] < row or (n > 1 and st[0] < (h - 1) * st[1] + row):
            raise MjxError(ERR_INVALID_ARG, "plane %d: stride %s -- the innermost dimension is dense, rows at least a row apart, pictures apart" % (k, tuple(st)))
        per_plane.append((t.data_ptr(), st[0] * t.element_size(), st[1]))
        sizes.append((w, h))
    if cbcr is not None:
        sizes.append(sizes[1])
    dst = [([(ptr + i * step, pitch) for ptr, step, pitch in per_plane], sizes) for i in range(n)]
    fmt = Planes(names[y.dtype], interleave=cbcr is not None, mean=mean, std=std, dst=dst)
    torch.cuda.current_stream(y.device).synchronize()
    rs = None
    if resize is not None and resize is not False:
        w, h = sizes[0]
        rs = Resize(w, h) if resize is True else resize.sized(w, h)
        if resize is not True and (resize.width or resize.height) and (resize.width, resize.height) != (w, h):
            raise MjxError(ERR_INVALID_ARG, "resize to %d x %d into a tensor of %d x %d" % (resize.width, resize.height, w, h))
    batch, status = decode_batch(ctx, datas, threads=threads, device_destuff=device_destuff, scale=scale, rois=rois, pixels=pixels, idct=idct, planes=fmt,
                                 resize=rs, orient=orient)
    batch.close()
    return status


class Pool:
    """mjx_pool: one context, host thread and work queue per device slot; the files of a call are dealt to the slots by
    compressed bytes (largest first; i mod N for equal files) or round robin (set_deal).  threads_per_device = 0: the slots
    share the host's processors (max(2, P / 2N) parse threads each)."""

    def __init__(self, devices):
        self.h = _vp()
        arr = (_int * len(devices))(*[int(d) for d in devices])
        _check(lib().mjx_pool_create(arr, len(devices), ctypes.byref(self.h)), "mjx_pool_create(%s)" % list(devices))

    def __len__(self):
        return int(lib().mjx_pool_devices(self.h))

    def device(self, slot):
        return int(lib().mjx_pool_device(self.h, slot))

    def set_deal(self, round_robin):
        _check(lib().mjx_pool_set_deal(self.h, 1 if round_robin else 0), "mjx_pool_set_deal")

    def decode_batch(self, datas, strict_ref=False, layout=LAYOUT_STANDARD, threads_per_device=0, device_destuff=None, scale=1, rois=None, pixels=None, color=None, progressive=False, idct=None):
        """-> PoolResult; .slot_of[i], .status[i], .rgb(i), .rc (the call's return code: a failed slot fails its own files only).
        scale, rois, pixels, color: see Batch (a file's rectangle follows it to its slot)."""
        n = len(datas)
        arr = (ctypes.c_char_p * max(n, 1))(*[bytes(d) for d in datas])
        lens = (_sz * max(n, 1))(*[len(d) for d in datas])
        st = (_int * max(n, 1))()
        slots = (_int * max(n, 1))()
        ptrs = (_P(ctypes.c_uint8) * max(n, 1))()
        h = _vp()
        o = _opts(strict_ref, layout, device_destuff=device_destuff, scale=scale, rois=rois, pixels=pixels, idct=idct, color=color, progressive=progressive)
        rc = lib().mjx_pool_decode_batch(self.h, arr, lens, n, ctypes.byref(o), int(threads_per_device), slots, ptrs, st, ctypes.byref(h))
        if not h:
            _check(rc, "mjx_pool_decode_batch")
        res = PoolResult(h, list(slots)[:n], list(st)[:n], [ctypes.cast(p, _vp).value for p in ptrs][:n])
        res.rc = int(rc)
        return res

    def close(self):
        if self.h:
            lib().mjx_pool_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        if sys is None or sys.is_finalizing():          # (at interpreter shutdown module globals may be gone already)
            return
        try:
            self.close()
        except Exception:
            pass


class PoolResult:
    def __init__(self, h, slot_of, status, ptrs):
        self.h, self.slot_of, self.status, self.ptrs = h, slot_of, status, ptrs

    def locate(self, i):
        slot, idx, b = _sz(), _sz(), _vp()
        _check(lib().mjx_pool_result_locate(self.h, i, ctypes.byref(slot), ctypes.byref(b), ctypes.byref(idx)))
        return slot.value, b, idx.value

    def host(self, slot):
        """-> (parse threads the slot's call ran with, NUMA node its host thread is bound to or -1)"""
        t, node = ctypes.c_uint(), _int()
        _check(lib().mjx_pool_result_host(self.h, slot, ctypes.byref(t), ctypes.byref(node)), "mjx_pool_result_host")
        return int(t.value), int(node.value)

    def slot_ms(self, slot):
        """-> wall clock (ms) of the slot's own mjx_decode_batch in this call (0.0: the slot had no file)"""
        ms = ctypes.c_double()
        _check(lib().mjx_pool_result_slot_ms(self.h, slot, ctypes.byref(ms)), "mjx_pool_result_slot_ms")
        return float(ms.value)

    def compare_rgb(self, mine, theirs):
        """On-device comparison of picture mine[k] with picture theirs[k] of this result (they may lie in different slots'
        batches on one device) -> (max |difference| per pair, differing bytes per pair), see Batch.compare_rgb."""
        n = len(mine)
        mx = np.zeros(max(n, 1), np.uint32)
        cnt = np.zeros(max(n, 1), np.uint64)
        groups = {}
        for k in range(n):
            _, ba, ia = self.locate(mine[k])
            _, bb, ib = self.locate(theirs[k])
            groups.setdefault((ba.value, bb.value), []).append((k, ia, ib))
        for (ha, hb), items in groups.items():
            m = len(items)
            ia = (_sz * m)(*[x[1] for x in items])
            ib = (_sz * m)(*[x[2] for x in items])
            gm = np.zeros(m, np.uint32)
            gc = np.zeros(m, np.uint64)
            _check(lib().mjx_batch_compare_rgb(_vp(ha), ia, _vp(hb), ib, m, gm.ctypes.data_as(_P(ctypes.c_uint32)),
                                               gc.ctypes.data_as(_P(ctypes.c_uint64))), "mjx_batch_compare_rgb")
            for j, x in enumerate(items):
                mx[x[0]], cnt[x[0]] = gm[j], gc[j]
        return mx[:n], cnt[:n]

    def rgb(self, i):
        _, b, idx = self.locate(i)
        v = [ctypes.c_uint32() for _ in range(4)]
        lib().mjx_batch_image_info(b, idx, *[ctypes.byref(x) for x in v])
        out = np.empty((v[1].value, v[0].value, 3), np.uint8)
        _check(lib().mjx_batch_copy_rgb(b, idx, out.ctypes.data_as(_vp)), "mjx_batch_copy_rgb")
        return out

    def close(self):
        if self.h:
            lib().mjx_pool_result_free(self.h)
            self.h = _vp()

    def __del__(self):
        if sys is None or sys.is_finalizing():          # (at interpreter shutdown module globals may be gone already)
            return
        try:
            self.close()
        except Exception:
            pass


def plan_tiles(data, roi=None, scale=1, pixels=None, color=None, progressive=False, idct=None):
    """Host only: the stage-B tiles a decode of this file with this rectangle and scale reads -> see ParsedScan.plan_tiles."""
    scan = ParsedScan(data, color=color, progressive=progressive)
    try:
        return scan.plan_tiles(roi=roi, scale=scale, pixels=pixels, idct=idct, color=color, progressive=progressive)
    finally:
        scan.close()


def resize_plan(data, resize, roi=None, scale=1, pixels=None, idct=None):
    """Host only: the scale, rectangle and tap counts of a resized decode of this file -> see ParsedScan.resize_plan."""
    scan = ParsedScan(data)
    try:
        return scan.resize_plan(resize, roi=roi, scale=scale, pixels=pixels, idct=idct)
    finally:
        scan.close()


def orient_plan(data, code, resize=None, roi=None, scale=1):
    """Host only: the picture that leaves when this file is decoded with orientation code `code` -> see ParsedScan.orient_plan."""
    scan = ParsedScan(data)
    try:
        return scan.orient_plan(code, resize=resize, roi=roi, scale=scale)
    finally:
        scan.close()


def planes_layout(data, planes, i=0, roi=None, scale=1, pixels=None, resize=None, code=None, idct=None):
    """Host only: the planes a decode of this file as input i with this Planes would write -> see ParsedScan.planes_layout (resize, code:
    the planes that leave a call with a resize and / or an orientation)."""
    scan = ParsedScan(data)
    try:
        return scan.planes_layout(planes, i=i, roi=roi, scale=scale, pixels=pixels, idct=idct, resize=resize, code=code)
    finally:
        scan.close()


def output_layout(data, output=None, i=0, roi=None, scale=1):
    """Host only: what a decode of this file as input i with this Output would write -> see ParsedScan.output_layout."""
    scan = ParsedScan(data)
    try:
        return scan.output_layout(output, i=i, roi=roi, scale=scale)
    finally:
        scan.close()


def color_model(data):
    """mjx_color_model (host only) -> dict(model -- MODEL_*, name, ncomp, jfif, adobe, adobe_transform, ids): what the components of
    the file are when a call takes the file's word for it (color="file")."""
    ci = ColorInfo()
    _check(lib().mjx_color_model(bytes(data), len(data), ctypes.byref(ci)), "mjx_color_model")
    return dict(model=ci.model, name=MODEL_NAMES[ci.model], ncomp=ci.ncomp, jfif=bool(ci.jfif), adobe=bool(ci.adobe),
                adobe_transform=ci.adobe_transform, ids=list(ci.ids)[:ci.ncomp])


def ink_mul(a, k):
    """mjx_ink_mul: (a k + 127) // 255, the routine the kernels multiply a sample by K with (CMYK, YCCK)."""
    return int(lib().mjx_ink_mul(int(a), int(k)))


def decode(data, strict_ref=False, layout=LAYOUT_STANDARD, scale=1, roi=None, pixels=None, color=None, progressive=False, idct=None):
    """One-shot C entry point mjx_decode (parse + GPU decode + copy back) -> ndarray [H, W, 3] uint8.  scale: see Batch.
    roi: (x, y, w, h) of the scaled picture -- the array is that rectangle, [h, w, 3]."""
    img = Image()
    o = _opts(strict_ref, layout, scale=scale, rois=roi, pixels=pixels, idct=idct, color=color, progressive=progressive)
    _check(lib().mjx_decode(bytes(data), len(data), ctypes.byref(o), ctypes.byref(img)), "mjx_decode")
    try:
        return np.ctypeslib.as_array(img.rgb, (img.height, img.width, 3)).copy()
    finally:
        lib().mjx_free_image(ctypes.byref(img))


# ---- synthetic inputs ----------------------------------------------------------------
_synth = None


def synth_lib():
    global _synth
    if _synth is None:
        path = os.path.join(_PKG, "synth", "libmjx_synth.so")
        if not os.path.exists(path):
            raise ImportError("libmjx_synth.so is not built: run `python jpeg-rust_amd/build.py`")
        s = ctypes.CDLL(path)
        s.mjxs_synth_jpeg.restype = _sz
        s.mjxs_synth_jpeg.argtypes = [_int] * 4 + [ctypes.c_uint64, ctypes.c_float, ctypes.c_char_p, _sz]
        s.mjxs_synth_jpeg_ex.restype = _sz
        s.mjxs_synth_jpeg_ex.argtypes = [_int] * 5 + [ctypes.c_uint64, ctypes.c_float, ctypes.c_char_p, _sz]
        s.mjxs_encode_ex.restype = _sz
        s.mjxs_encode_ex.argtypes = [_vp, _int, _int, _int, _int, _int, ctypes.c_char_p, _sz]
        s.mjxs_encode.restype = _sz
        s.mjxs_encode.argtypes = [_vp, _int, _int, _int, _int, ctypes.c_char_p, _sz]
        s.mjxs_fill_rgb.restype = None
        s.mjxs_fill_rgb.argtypes = [_vp, _int, _int, ctypes.c_uint64, ctypes.c_float]
        _synth = s
    return _synth


def synth_jpeg(width, height, subsampling="420", quality=75, seed=0, noise_sigma=6.0, dqt16=False):
    """Deterministic baseline JPEG: plane waves + noise content, Annex-K tables, only markers the reference parses.
    dqt16: 16-bit quantisation tables (Pq = 1, src/jpeg/mod.rs:245-256), values not clamped at 255."""
    cap = width * height * 3 + 65536
    buf = ctypes.create_string_buffer(cap)
    n = synth_lib().mjxs_synth_jpeg_ex(width, height, SUBSAMPLING[subsampling], quality, 1 if dqt16 else 0, seed, noise_sigma, buf, cap)
    if n == 0:
        raise RuntimeError("synthetic encode failed")
    return buf.raw[:n]


def encode_rgb(rgb, subsampling="420", quality=75, dqt16=False):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    cap = w * h * 3 + 65536
    buf = ctypes.create_string_buffer(cap)
    n = synth_lib().mjxs_encode_ex(rgb.ctypes.data_as(_vp), w, h, SUBSAMPLING[subsampling], quality, 1 if dqt16 else 0, buf, cap)
    if n == 0:
        raise RuntimeError("encode failed")
    return buf.raw[:n]


def synth_batch(n_unique, width, height, subsampling="420", quality=75, seed0=0, threads=None):
    threads = threads or min(32, os.cpu_count() or 1)
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(lambda s: synth_jpeg(width, height, subsampling, quality, seed0 + s), range(n_unique)))
