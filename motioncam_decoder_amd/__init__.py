"""motioncam_decoder_amd -- MI355X (gfx950) MCRAW frame-decode path.

Python is plumbing only: this module loads the C-ABI shared library
(``lib/libmcraw_hip.so``, declared in ``include/mcraw_hip.h``) with ctypes and
hands it device pointers (e.g. ``torch.Tensor.data_ptr()``).  The product is
the HIP library and the C++ ``motioncam::Decoder`` facade under ``host/``.

There is no CPU decode path here: if the HIP library is missing or no GPU is
present, every decode call raises.
"""
import collections
import ctypes as C
import functools
import os

__all__ = ["lib_path", "load", "Context", "Pool", "Frame", "EncFrame", "FloatOut", "McrawError", "TYPE_LEGACY", "TYPE_BLOCK",
           "MEM_DEVICE", "MEM_HOST", "KERNELS", "ENC_KERNELS", "ABI_SYMBOLS", "encode_bound7", "cfa_planes",
           "RgbParams", "RgbColor", "RGB_KERNELS", "rgb_color", "Display", "transfer_lut", "DISP_U8", "DISP_U16",
           "DISP_CHW", "DISP_HWC", "Yuv", "YUV_NV12", "YUV_P010", "yuv_matrix", "yuv_planes", "Shade", "gain_map",
           "shading_map", "Stats", "STATS_ACCUMULATE", "FrameStats", "stats_white_balance", "stats_percentile",
           "stats_clipped", "FixPix", "FIXPIX_HOT", "FIXPIX_COLD", "pack_pixels", "Denoise", "noise_lut", "Merge", "Align",
           "AlignCells", "Cells", "cell_grid", "align_window", "fit_crop", "Area", "RGB_AREA", "Resample", "RGB_RESAMPLE",
           "FILTER_LINEAR", "FILTER_CUBIC", "Warp", "RGB_WARP", "quantize_affine", "fit_affine", "stabilize", "RGB_HA",
           "Mesh", "RGB_MESH", "MESH_STEP", "mesh_grid", "affine_mesh", "distortion_mesh", "stabilize_mesh", "mesh_check",
           "Highlights", "HighlightChroma", "HL_CLIP", "HL_REBUILD", "HL_ACCUMULATE", "highlight_gains",
           "Noise", "NoiseStats", "NOISE_ACCUMULATE", "noise_fit", "noise_quantile_gain"]

_PKG = os.path.dirname(os.path.abspath(__file__))

TYPE_LEGACY = 6
TYPE_BLOCK = 7
MEM_DEVICE = 0
MEM_HOST = 1

# status bits (include/mcraw_hip.h)
E_ARGS, E_HEADER, E_TRUNCATED, E_SIDESTREAM, E_CAPACITY, E_DEVICE = 0x1, 0x2, 0x4, 0x8, 0x10, 0x100

KERNELS = {"k7_side": 0, "k7_tiles": 3, "k6_decode": 6}
ENC_KERNELS = {"k7e_payload": 7, "k7e_side": 8}  # the encoder's launches (mcraw_encode_batch)
RGB_KERNELS = {"krgb_mhc": 9, "krgb_bin2": 10}  # the demosaic's launches (mcraw_demosaic_batch)

# every symbol include/mcraw_hip.h declares
ABI_SYMBOLS = [
    "mcraw_ctx_create", "mcraw_ctx_destroy", "mcraw_last_error", "mcraw_decode7", "mcraw_decode6",
    "mcraw_decode_batch", "mcraw_ctx_synchronize", "mcraw_ctx_profile", "mcraw_ctx_kernel_ms",
    "mcraw_host_alloc", "mcraw_host_free", "mcraw_ctx_set_post", "mcraw_decode_batch_async", "mcraw_ticket_wait",
    "mcraw_ctx_profile_every", "mcraw_legacy_launch_order", "mcraw_shard_of", "mcraw_shard_count", "mcraw_pool_create", "mcraw_pool_destroy", "mcraw_pool_last_error",
    "mcraw_pool_size", "mcraw_pool_device", "mcraw_pool_numa_cpus", "mcraw_pool_ctx", "mcraw_pool_set_post",
    "mcraw_pool_host_alloc", "mcraw_pool_decode_batch", "mcraw_pool_decode_batch_async", "mcraw_pool_ticket_wait",
    "mcraw_pool_decode_batch_device", "mcraw_ctx_xcd_runs", "mcraw_pool_synchronize", "mcraw_tile_order",
    "mcraw_ctx_last_serial", "mcraw_ctx_batch_status", "mcraw_ctx_errors", "mcraw_ctx_side_parts", "mcraw_ctx_host_way",
    "mcraw_encode_bound7", "mcraw_encode_batch", "mcraw_encode7", "mcraw_ctx_set_float_out", "mcraw_pool_set_float_out",
    "mcraw_demosaic_batch", "mcraw_demosaic_display_batch", "mcraw_demosaic_yuv_batch", "mcraw_shade_batch",
    "mcraw_stats_batch", "mcraw_stats_record_bytes", "mcraw_fixpix_batch", "mcraw_denoise_batch",
    "mcraw_merge_batch", "mcraw_align_batch", "mcraw_align_work_bytes", "mcraw_demosaic_area_batch", "mcraw_area_work_bytes",
    "mcraw_demosaic_resample_batch", "mcraw_resample_work_bytes", "mcraw_demosaic_warp_batch",
    "mcraw_align_cells_batch", "mcraw_align_cells_work_bytes", "mcraw_merge_cells_batch",
    "mcraw_highlights_measure_batch", "mcraw_highlights_batch",
    "mcraw_mesh_nodes", "mcraw_mesh_check", "mcraw_demosaic_mesh_batch",
    "mcraw_noise_batch", "mcraw_noise_record_bytes", "mcraw_noise_energy_bin",
]

POST_BLACK, POST_PACK12, POST_PACK10, POST_PACK14 = 1, 2, 4, 8
_PACK_FLAG = {16: 0, 12: POST_PACK12, 10: POST_PACK10, 14: POST_PACK14}


class Post(C.Structure):
    """struct mcraw_post (include/mcraw_hip.h)."""
    _fields_ = [("flags", C.c_uint32), ("black", C.c_uint16 * 4)]


class McrawError(RuntimeError):
    pass


# normalised float output (mcraw_ctx_set_float_out)
FLOAT_F32, FLOAT_F16, FLOAT_BF16 = 1, 2, 3
LAYOUT_MOSAIC, LAYOUT_PLANES = 0, 1
FLOAT_CLIP = 1
_FLOAT_CODES = {"f32": FLOAT_F32, "f16": FLOAT_F16, "bf16": FLOAT_BF16,
                "float32": FLOAT_F32, "float16": FLOAT_F16, "bfloat16": FLOAT_BF16}
_LAYOUTS = {"mosaic": LAYOUT_MOSAIC, "planes": LAYOUT_PLANES}
# plane of CFA position p = (row & 1) * 2 + (col & 1) that puts R, G (R row), G (B row), B in planes 0..3
_CFA_PLANES = {"rggb": [0, 1, 2, 3], "bggr": [3, 2, 1, 0], "grbg": [1, 0, 3, 2], "gbrg": [2, 3, 0, 1]}


class FloatOut(C.Structure):
    """struct mcraw_float_out (include/mcraw_hip.h)."""
    _fields_ = [("dtype", C.c_uint32), ("layout", C.c_uint32), ("flags", C.c_uint32), ("black", C.c_uint16 * 4),
                ("white", C.c_float), ("plane", C.c_uint8 * 4)]


def cfa_planes(arrangement):
    """The ``plane`` map of set_float_out / decode_tensor that puts R, G (on the R row), G (on the B row), B in planes
    0..3, from the container's ``sensorArrangment`` ("rggb", "bggr", "grbg" or "gbrg")."""
    key = str(arrangement).strip().lower()
    if key not in _CFA_PLANES:
        raise ValueError("unknown sensorArrangment %r (rggb, bggr, grbg or gbrg)" % (arrangement,))
    return list(_CFA_PLANES[key])


def _float_code(dtype):
    """MCRAW_FLOAT_* of a torch dtype or of "f32" / "f16" / "bf16" (torch is not needed for the strings)."""
    if isinstance(dtype, str):
        code = _FLOAT_CODES.get(dtype.lower())
    else:
        code = _FLOAT_CODES.get(str(dtype).replace("torch.", ""))
    if code is None:
        raise ValueError("float output dtype must be torch.float32 / float16 / bfloat16 or 'f32' / 'f16' / 'bf16', not %r" % (dtype,))
    return code


def float_out(dtype, white, layout="planes", black=(0, 0, 0, 0), clip=False, plane=None):
    """The FloatOut struct of these arguments (plane: None = identity)."""
    if layout not in _LAYOUTS:
        raise ValueError("layout must be 'planes' or 'mosaic', not %r" % (layout,))
    f = FloatOut()
    f.dtype = _float_code(dtype)
    f.layout = _LAYOUTS[layout]
    f.flags = FLOAT_CLIP if clip else 0
    black = list(black)
    if len(black) != 4:
        raise ValueError("black: four levels, by CFA position (row & 1) * 2 + (col & 1)")
    for i in range(4):
        f.black[i] = int(black[i])
    f.white = float(white)
    plane = [0, 1, 2, 3] if plane is None else list(plane)
    if len(plane) != 4:
        raise ValueError("plane: four plane indices, by CFA position")
    for i in range(4):
        f.plane[i] = int(plane[i])
    return f


# demosaic to planar linear RGB (mcraw_demosaic_batch)
RGB_MHC, RGB_BIN2 = 1, 2
RGB_AREA = 3  # mcraw_demosaic_area_batch only
RGB_RESAMPLE = 4  # mcraw_demosaic_resample_batch only
RGB_WARP = 5  # mcraw_demosaic_warp_batch only
RGB_HA = 6  # the edge-directed demosaic (Hamilton-Adams): full resolution, valid where RGB_MHC is
RGB_MESH = 7  # mcraw_demosaic_mesh_batch only
MESH_STEP = 32  # output pixels between the nodes of a mesh, both axes
FILTER_LINEAR, FILTER_CUBIC = 0, 1
_RGB_ALGOS = {"mhc": RGB_MHC, "bin2": RGB_BIN2, "area": RGB_AREA, "resample": RGB_RESAMPLE, "warp": RGB_WARP, "ha": RGB_HA,
              "mesh": RGB_MESH}
_FILTERS = {"linear": FILTER_LINEAR, "cubic": FILTER_CUBIC}
_CFA_CODES = {"rggb": 0, "bggr": 1, "grbg": 2, "gbrg": 3}


class RgbParams(C.Structure):
    """struct mcraw_rgb (include/mcraw_hip.h)."""
    _fields_ = [("algo", C.c_uint32), ("dtype", C.c_uint32), ("flags", C.c_uint32), ("cfa", C.c_uint32),
                ("black", C.c_uint16 * 4), ("white", C.c_float)]


class RgbColor(C.Structure):
    """struct mcraw_rgb_color (include/mcraw_hip.h): white-balance gains and a row-major 3x3 matrix, out = m . v."""
    _fields_ = [("gain", C.c_float * 3), ("m", C.c_float * 9)]


class Area(C.Structure):
    """struct mcraw_area (include/mcraw_hip.h): the crop window in the mosaic and the output size."""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("cw", C.c_uint32), ("ch", C.c_uint32), ("out_w", C.c_uint32),
                ("out_h", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class Resample(C.Structure):
    """struct mcraw_resample (include/mcraw_hip.h): the crop window in the mosaic, the output size and the filter."""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("cw", C.c_uint32), ("ch", C.c_uint32), ("out_w", C.c_uint32),
                ("out_h", C.c_uint32), ("filter", C.c_uint32), ("reserved", C.c_uint32)]


class Warp(C.Structure):
    """struct mcraw_warp (include/mcraw_hip.h): the output size and the filter of mcraw_demosaic_warp_batch."""
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("filter", C.c_uint32), ("reserved", C.c_uint32)]


class Mesh(C.Structure):
    """struct mcraw_mesh (include/mcraw_hip.h): the output size and the filter of mcraw_demosaic_mesh_batch."""
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("filter", C.c_uint32), ("reserved", C.c_uint32)]


# The scaled algos of the demosaic methods (size=, crop=): algo -> (the window struct, the library's work-bytes function, its entry
# point for the three families, the geometry rule as the ValueError states it).
_SCALED = {
    "area": (Area, "mcraw_area_work_bytes", "mcraw_demosaic_area_batch",
             "the crop must be even and not empty, and hold 1 .. 16 quads per output pixel along each axis"),
    "resample": (Resample, "mcraw_resample_work_bytes", "mcraw_demosaic_resample_batch",
                 "the crop must be even and not empty, and the size 1/2 .. 2 of it along each axis"),
}

# What the demosaic methods know in front of their output (Context._demosaic_front).  mos: the mosaics (N, H, W) behind the
# optional stages; single: the caller's was (H, W); n, h, w: their shape; src: _strided's triple (None for no frames); ho, wo: the
# output size; key: the cfa's; area: the (y0, x0, h, w) crop of a scaled algo (None for the others); filt: the MCRAW_FILTER_* code
# of algo "resample", "warp" and "mesh" (None for the others); maps: the int32 (nmaps, 6) host array of algo "warp" (None for the
# others); mesh: the int32 (nmesh, My, Mx, 2) device tensor of algo "mesh" (None for the others).
_Front = collections.namedtuple("_Front", "mos single n h w src ho wo key area filt maps mesh", defaults=(None, None))


def fit_crop(height, width, Ho, Wo, algo="area"):
    """The largest centred crop (y0, x0, h, w) of a height x width mosaic that has the output's aspect ratio Wo : Ho, for
    algo="area": h = 2 Ho t and w = 2 Wo t for the largest t (a real number) that fits, both rounded down to even numbers, the
    origin rounded down to even.  Raises ValueError when the sizes are no positive integers or when the crop breaks the ratio
    rule of mcraw_demosaic_area_batch (Ho <= h / 2 <= 16 Ho, Wo <= w / 2 <= 16 Wo).  fit_crop(3024, 4032, 1080, 1920) is
    (378, 0, 2268, 4032).  algo="resample": the same crop under the rule of mcraw_demosaic_resample_batch (h / 2 <= Ho <= 2 h,
    w / 2 <= Wo <= 2 w): fit_crop(3024, 4032, 2160, 3840, algo="resample") is (378, 0, 2268, 4032)."""
    if algo not in _SCALED:
        raise ValueError("fit_crop: algo must be 'area' or 'resample', not %r" % (algo,))
    for v in (height, width, Ho, Wo):
        if isinstance(v, bool) or v != int(v) or int(v) < 1:
            raise ValueError("fit_crop: sizes must be positive integers, not %r" % (v,))
    height, width, Ho, Wo = int(height), int(width), int(Ho), int(Wo)
    if width * Ho <= height * Wo:  # the width binds
        w = width // 2 * 2
        h = (width * Ho) // Wo // 2 * 2
    else:
        h = height // 2 * 2
        w = (height * Wo) // Ho // 2 * 2
    if algo == "resample":
        if not (2 <= h <= 2 * Ho <= 4 * h and 2 <= w <= 2 * Wo <= 4 * w):
            raise ValueError("fit_crop: a %d x %d crop of a %d x %d mosaic onto %d x %d is outside 1/2 .. 2 samples per pixel"
                             % (h, w, height, width, Ho, Wo))
    elif not (Ho <= h // 2 <= 16 * Ho and Wo <= w // 2 <= 16 * Wo):
        raise ValueError("fit_crop: a %d x %d crop of a %d x %d mosaic onto %d x %d is outside 1 .. 16 quads per pixel"
                         % (h, w, height, width, Ho, Wo))
    return ((height - h) // 4 * 2, (width - w) // 4 * 2, h, w)


_WARP_ONE, _WARP_DEV = 65536, 16384  # the linear part's unit and its largest deviation from the identity (include/mcraw_hip.h)


def quantize_affine(affine):
    """Float maps (2, 3) or (N, 2, 3), rows [[ayy, ayx, ty], [axy, axx, tx]] in samples, as the int32 maps (6,) or (N, 6) that
    mcraw_demosaic_warp_batch takes, {ayy, ayx, ty, axy, axx, tx}: floor(v * 65536 + 0.5) for the linear part,
    floor(v * 256 + 0.5) for the translation (host only, float64).  Raises ValueError for another shape and for values that
    are not finite or leave int32."""
    import numpy as np
    a = np.asarray(affine, dtype=np.float64)
    if a.shape[-2:] != (2, 3) or a.ndim not in (2, 3):
        raise ValueError("quantize_affine: maps must be (2, 3) or (N, 2, 3), not %r" % (a.shape,))
    if not np.isfinite(a).all():
        raise ValueError("quantize_affine: a map entry is not finite")
    q = np.floor(a * np.array([65536.0, 65536.0, 256.0]) + 0.5)
    if q.size and (q.min() < -2 ** 31 or q.max() > 2 ** 31 - 1):
        raise ValueError("quantize_affine: a map entry leaves int32")
    return np.ascontiguousarray(q.astype(np.int32).reshape(a.shape[:-2] + (6,)))


def _affine_maps(fn, affine, n):
    """affine= of the demosaic methods as the contiguous int32 host array (nmaps, 6), nmaps 1 or n.  A tensor on the device is
    brought to the host, which synchronises."""
    import numpy as np
    if hasattr(affine, "detach") and hasattr(affine, "cpu"):  # a torch tensor, wherever it lives
        affine = affine.detach().cpu().numpy()
    a = np.asarray(affine)
    if a.dtype.kind in "iu":
        if a.dtype != np.int32 or a.ndim not in (1, 2) or a.shape[-1] != 6:
            raise ValueError("%s: integer maps must be int32 (6,) or (N, 6), not %s %r" % (fn, a.dtype, a.shape))
        maps = np.ascontiguousarray(a.reshape(-1, 6))
    elif a.dtype.kind == "f":
        try:
            maps = quantize_affine(a).reshape(-1, 6)
        except ValueError as e:
            raise ValueError("%s: affine: %s" % (fn, e)) from None
    else:
        raise ValueError("%s: affine must be int32 (6,) / (N, 6) or float (2, 3) / (N, 2, 3)" % fn)
    if n and maps.shape[0] not in (1, n):
        raise ValueError("%s: affine holds %d maps for %d frames (one for all, or one each)" % (fn, maps.shape[0], n))
    return maps


def fit_affine(pos, height, width, cell=None):
    """The displacement model of a clip, float64 (N, 2, 3): D_t(y, x) = D[t, :, :2] @ (y, x) + D[t, :, 2] ~ pos_t at (y, x), rows
    (y, x) as everywhere.  pos (N, 2), as Context.align returns it: a zero linear part and the translation.  pos (N, Cy, Cx, 2)
    with cell=(cell_h, cell_w), as Context.align_cells returns it for (Cy, Cx) = cell_grid(height, width, cell): the least-
    squares affine over the cell centres (i * cell_h + cell_h / 2, j * cell_w + cell_w / 2); a grid with a single row or column
    of cells leaves that axis's slope 0.  Host only (a tensor is brought to the host); stabilize() turns the model into maps."""
    import numpy as np
    if hasattr(pos, "detach") and hasattr(pos, "cpu"):
        pos = pos.detach().cpu().numpy()
    p = np.asarray(pos, dtype=np.float64)
    if p.ndim == 2 and p.shape[1] == 2 and cell is None:
        D = np.zeros((p.shape[0], 2, 3))
        D[:, :, 2] = p
        return D
    if p.ndim != 4 or p.shape[3] != 2 or cell is None:
        raise ValueError("fit_affine: pos must be (N, 2), or (N, Cy, Cx, 2) with cell=(cell_h, cell_w), not %r" % (p.shape,))
    if tuple(p.shape[1:3]) != cell_grid(height, width, cell):
        raise ValueError("fit_affine: a %r field is not the cell_grid of %d x %d frames with cells %r" % (tuple(p.shape[1:3]), height, width, tuple(cell)))
    n, cy, cx = p.shape[:3]
    yc = np.arange(cy) * float(cell[0]) + cell[0] / 2.0
    xc = np.arange(cx) * float(cell[1]) + cell[1] / 2.0
    Y, X = np.meshgrid(yc, xc, indexing="ij")
    cols = [Y.ravel() - Y.mean() if cy > 1 else None, X.ravel() - X.mean() if cx > 1 else None]
    A = np.stack([c for c in cols if c is not None] + [np.ones(cy * cx)], axis=1)   # centred: well conditioned
    sol = np.linalg.lstsq(A, p.reshape(n, cy * cx, 2).transpose(1, 0, 2).reshape(cy * cx, n * 2), rcond=None)[0].reshape(A.shape[1], n, 2)
    D = np.zeros((n, 2, 3))
    k = 0
    for axis, c in enumerate(cols):
        if c is not None:
            D[:, :, axis] = sol[k]
            k += 1
    D[:, :, 2] = sol[k] - D[:, :, 0] * Y.mean() - D[:, :, 1] * X.mean()
    return D


def stabilize(D, height, width, size, window=0, limit=True):
    """The maps that stabilise a clip, int32 (N, 6) for affine= of the demosaic methods, from its displacement model D (N, 2, 3)
    (fit_affine).  The sign follows mcraw_merge_batch's pos: in[t][q + pos[t] - pos[b]] looks like in[b][q], so
    out_t(q) = in[t][q + D_t(q) - S_t(q)], with S_t the coefficient-wise mean of D over frames t - window .. t + window (clipped
    to the batch): the smooth path that stays in the result.  window=0: S = 0, a lock onto the frame of position 0.  Output
    pixel (i, k) of size = (Ho, Wo) is q = (i + (height - Ho) // 2, k + (width - Wo) // 2): the centred window.  limit=True
    clamps each frame's translation per axis so that the four corners of the output read inside the frame, as the library
    demands, and raises ValueError where no translation can do that (the size is too large for the roll and zoom) or where the
    linear part leaves the library's bounds (|a - identity| <= 1/4); limit=False returns the maps as they are.  Host only."""
    import numpy as np
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 3 or D.shape[1:] != (2, 3):
        raise ValueError("stabilize: D must be (N, 2, 3), not %r" % (D.shape,))
    try:
        ho, wo = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("stabilize: size must be (Ho, Wo)") from None
    height, width, window = int(height), int(width), int(window)
    if not (1 <= ho <= height and 1 <= wo <= width) or window < 0:
        raise ValueError("stabilize: size %r must fit the %d x %d frame, and window be >= 0" % (size, height, width))
    n = D.shape[0]
    S = np.zeros_like(D)
    if window:
        for t in range(n):
            S[t] = D[max(0, t - window):min(n, t + window + 1)].mean(axis=0)
    R = D - S
    off = np.array([(height - ho) // 2, (width - wo) // 2], dtype=np.float64)
    M = R[:, :, :2] + np.eye(2)
    A = np.concatenate([M, (M @ off + R[:, :, 2])[:, :, None]], axis=2)
    maps = quantize_affine(A).reshape(n, 6)
    if not limit:
        return maps
    for t in range(n):
        m = maps[t].astype(np.int64)
        if max(abs(m[0] - _WARP_ONE), abs(m[4] - _WARP_ONE), abs(m[1]), abs(m[3])) > _WARP_DEV:
            raise ValueError("stabilize: the linear part of frame %d leaves the warp's bounds (|a - identity| <= 1/4)" % t)
        for base, side, name in ((0, height, "rows"), (3, width, "columns")):
            c = [(m[base] * i + m[base + 1] * k + 128) >> 8 for i in (0, ho - 1) for k in (0, wo - 1)]
            lo, hi = -min(c), 256 * (side - 1) - max(c)
            if lo > hi:
                raise ValueError("stabilize: frame %d: a %d x %d output cannot stay inside the frame's %s under this roll and zoom"
                                 % (t, ho, wo, name))
            maps[t, base + 2] = min(max(int(m[base + 2]), lo), hi)
    return maps


def mesh_grid(Ho, Wo):
    """(My, Mx): the nodes of the mesh of an Ho x Wo output, ceil(Ho / 32) + 1 and ceil(Wo / 32) + 1 (host only)."""
    for v in (Ho, Wo):
        if isinstance(v, bool) or v != int(v) or not 1 <= int(v) <= 65536:
            raise ValueError("mesh_grid: Ho and Wo must be integers 1 .. 65536, not %r" % (v,))
    return (int(Ho) + MESH_STEP - 1) // MESH_STEP + 1, (int(Wo) + MESH_STEP - 1) // MESH_STEP + 1


def _mesh_size(fn, size):
    try:
        ho, wo = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("%s: size must be (Ho, Wo)" % fn) from None
    if not (1 <= ho <= 65536 and 1 <= wo <= 65536):
        raise ValueError("%s: size must be (Ho, Wo), both 1 .. 65536, not %r" % (fn, size))
    return ho, wo


def _mesh_round(fn, v):
    """floor(v * 256 + 0.5) as int32; ValueError where that is not finite or leaves int32."""
    import numpy as np
    q = np.floor(np.asarray(v, dtype=np.float64) * 256.0 + 0.5)
    if not np.isfinite(q).all() or (q.size and (q.min() < -2 ** 31 or q.max() > 2 ** 31 - 1)):
        raise ValueError("%s: a node is not finite or leaves int32" % fn)
    return np.ascontiguousarray(q.astype(np.int32))


def _mesh_maps(fn, maps):
    """Affine maps as int32 (N, 6): _affine_maps, which also takes integers of another width (a list of Python ints)."""
    import numpy as np
    if hasattr(maps, "detach") and hasattr(maps, "cpu"):
        maps = maps.detach().cpu().numpy()
    a = np.asarray(maps)
    if a.dtype.kind in "iu" and a.dtype != np.int32 and a.size and -2 ** 31 <= a.min() and a.max() < 2 ** 31:
        a = a.astype(np.int32)
    return _affine_maps(fn, a, 0)


def affine_mesh(maps, size):
    """The meshes of affine maps, int32 (N, My, Mx, 2): the position mcraw_demosaic_warp_batch gives output pixel (32 a, 32 b)
    under each map, at every node -- also those behind the last partial tile --, so that algo="mesh" follows algo="warp" to
    within 1/256 sample, and bit for bit where the linear part is the identity.  maps: int32 (6,) or (N, 6) as the library takes
    them, or float (2, 3) / (N, 2, 3) (quantize_affine).  Host only."""
    import numpy as np
    ho, wo = _mesh_size("affine_mesh", size)
    m = _mesh_maps("affine_mesh", maps).astype(np.int64)
    my, mx = mesh_grid(ho, wo)
    i = (MESH_STEP * np.arange(my, dtype=np.int64))[None, :, None]
    k = (MESH_STEP * np.arange(mx, dtype=np.int64))[None, None, :]
    c = [m[:, j][:, None, None] for j in range(6)]
    Y = c[2] + ((c[0] * i + c[1] * k + 128) >> 8)
    X = c[5] + ((c[3] * i + c[4] * k + 128) >> 8)
    out = np.stack([Y, X], axis=-1)
    if out.min() < -2 ** 31 or out.max() > 2 ** 31 - 1:
        raise ValueError("affine_mesh: a node leaves int32")
    return np.ascontiguousarray(out.astype(np.int32))


def _affine_float(fn, affine):
    """Stabilise maps, int32 (6,) / (N, 6) or float (2, 3) / (N, 2, 3), as float64 (N, 2, 3) in samples."""
    import numpy as np
    m = _mesh_maps(fn, affine).astype(np.float64).reshape(-1, 2, 3)
    return m / np.array([65536.0, 65536.0, 256.0])


def distortion_mesh(height, width, size, radial=(1.0, 0.0, 0.0, 0.0), tangential=(0.0, 0.0), center=(0.5, 0.5), affine=None):
    """The mesh of DNG's WarpRectilinear for one plane, int32 (My, Mx, 2), or (N, My, Mx, 2) with affine= (N, 6): output pixel q
    reads the frame at c + f(r) d + tangential terms, with c = center * (width - 1, height - 1) (center is (cx, cy) in 0 .. 1 as
    in DNG), d = (q - c) / m, m the largest distance from c to a corner of the frame, r^2 = dx^2 + dy^2,
    f = k0 + k1 r^2 + k2 r^4 + k3 r^6, and the tangential terms (kt0, kt1) of the DNG specification:
    x: 2 kt0 dx dy + kt1 (r^2 + 2 dx^2), y: kt0 (r^2 + 2 dy^2) + 2 kt1 dx dy; the result is scaled back by m.  q of output pixel
    (i, k): the centred window, (i + (height - Ho) // 2, k + (width - Wo) // 2), or with affine= (stabilise maps of stabilize(),
    (6,) or (N, 6)) the position that map gives -- it is applied first, so one pass undistorts and stabilises.  float64, rounded
    as floor(v * 256 + 0.5).  Host only."""
    import numpy as np
    fn = "distortion_mesh"
    ho, wo = _mesh_size(fn, size)
    height, width = int(height), int(width)
    try:
        k = [float(v) for v in radial]
        kt = [float(v) for v in tangential]
        cx, cy = (float(v) for v in center)
    except (TypeError, ValueError):
        raise ValueError("%s: radial (k0, k1, k2, k3), tangential (kt0, kt1) and center (cx, cy) must be numbers" % fn) from None
    if len(k) != 4 or len(kt) != 2 or height < 1 or width < 1:
        raise ValueError("%s: radial holds four terms, tangential two, and the frame is at least 1 x 1" % fn)
    my, mx = mesh_grid(ho, wo)
    i = (MESH_STEP * np.arange(my, dtype=np.float64))[None, :, None]
    kk = (MESH_STEP * np.arange(mx, dtype=np.float64))[None, None, :]
    batched = False
    if affine is None:
        qy = i + float((height - ho) // 2) + 0.0 * kk
        qx = kk + float((width - wo) // 2) + 0.0 * i
    else:
        A = _affine_float(fn, affine)
        batched = tuple(np.shape(affine)) not in ((6,), (2, 3))  # one map gives one mesh, without N
        qy = A[:, 0, 0][:, None, None] * i + A[:, 0, 1][:, None, None] * kk + A[:, 0, 2][:, None, None]
        qx = A[:, 1, 0][:, None, None] * i + A[:, 1, 1][:, None, None] * kk + A[:, 1, 2][:, None, None]
    py, px = cy * (height - 1), cx * (width - 1)
    m = max(np.hypot(px - x, py - y) for x in (0.0, width - 1.0) for y in (0.0, height - 1.0))
    m = m if m > 0 else 1.0
    dy, dx = (qy - py) / m, (qx - px) / m
    r2 = dx * dx + dy * dy
    f = k[0] + r2 * (k[1] + r2 * (k[2] + r2 * k[3]))
    sy = py + m * (f * dy + kt[0] * (r2 + 2.0 * dy * dy) + 2.0 * kt[1] * dx * dy)
    sx = px + m * (f * dx + 2.0 * kt[0] * dx * dy + kt[1] * (r2 + 2.0 * dx * dx))
    out = _mesh_round(fn, np.stack([sy, sx], axis=-1))
    return out if batched else out[0]


def stabilize_mesh(field, height, width, cell, size, window=0, limit=True):
    """The meshes that stabilise a clip cell by cell, int32 (N, My, Mx, 2), from the field of local positions (N, Cy, Cx, 2) that
    Context.align_cells returns for (Cy, Cx) = cell_grid(height, width, cell): what fit_affine would flatten to six numbers per
    frame.  R_t = field_t minus the per-cell mean over frames t - window .. t + window (clipped to the batch; window=0: R = field,
    a lock onto the frame of position 0, stabilize()'s sign); R_t(q) is bilinear between the cell centres
    (i cell_h + cell_h / 2, j cell_w + cell_w / 2) and continues linearly beyond the outermost ones (constant along an axis with
    one cell).  Node = 256 (q + R_t(q)) at q, the centred window's pixel (32 a + (height - Ho) // 2, 32 b + (width - Wo) // 2),
    rounded as floor(v + 0.5).  limit=True raises ValueError where mesh_check() rejects a tile.  Host only."""
    import numpy as np
    fn = "stabilize_mesh"
    if hasattr(field, "detach") and hasattr(field, "cpu"):
        field = field.detach().cpu().numpy()
    p = np.asarray(field, dtype=np.float64)
    ho, wo = _mesh_size(fn, size)
    height, width, window = int(height), int(width), int(window)
    if p.ndim != 4 or p.shape[3] != 2 or tuple(p.shape[1:3]) != cell_grid(height, width, cell):
        raise ValueError("%s: field must be (N, Cy, Cx, 2), the cell_grid of %d x %d frames with cells %r, not %r"
                         % (fn, height, width, tuple(cell), p.shape))
    if not (ho <= height and wo <= width) or window < 0:
        raise ValueError("%s: size %r must fit the %d x %d frame, and window be >= 0" % (fn, size, height, width))
    n, cy, cx = p.shape[:3]
    R = p.copy()
    if window:
        for t in range(n):
            R[t] = p[t] - p[max(0, t - window):min(n, t + window + 1)].mean(axis=0)
    my, mx = mesh_grid(ho, wo)
    qy = MESH_STEP * np.arange(my, dtype=np.float64) + float((height - ho) // 2)
    qx = MESH_STEP * np.arange(mx, dtype=np.float64) + float((width - wo) // 2)

    def axis(q, cells, step):  # the two cells about q and the weight of the second: linear beyond the outermost centres
        if cells == 1:
            return np.zeros(q.size, dtype=np.int64), np.zeros(q.size, dtype=np.int64), np.zeros(q.size)
        g = (q - step / 2.0) / step
        lo = np.clip(np.floor(g).astype(np.int64), 0, cells - 2)
        return lo, lo + 1, g - lo

    y0, y1, fy = axis(qy, cy, float(cell[0]))
    x0, x1, fx = axis(qx, cx, float(cell[1]))
    fy, fx = fy[None, :, None, None], fx[None, None, :, None]
    top = R[:, y0][:, :, x0] * (1.0 - fx) + R[:, y0][:, :, x1] * fx
    bot = R[:, y1][:, :, x0] * (1.0 - fx) + R[:, y1][:, :, x1] * fx
    Rq = top * (1.0 - fy) + bot * fy                                     # (N, My, Mx, 2)
    q = np.stack(np.meshgrid(qy, qx, indexing="ij"), axis=-1)[None]
    out = _mesh_round(fn, q + Rq)
    if limit:
        try:
            mesh_check(out, height, width, (ho, wo))
        except ValueError as e:
            raise ValueError("%s: %s" % (fn, e)) from None
    return out


def mesh_check(mesh, height, width, size, inside=False):
    """mcraw_mesh_check on a host mesh, int32 (My, Mx, 2) or (N, My, Mx, 2) for size = (Ho, Wo): raises ValueError with the
    library's message naming the first frame and tile whose source window is larger than the kernel holds (the tap clamp would
    act there), or -- inside=True -- whose corner pixel reads outside the height x width frame (the border rule would act).
    Needs neither a GPU nor a context."""
    import numpy as np
    ho, wo = _mesh_size("mesh_check", size)
    a = np.asarray(mesh)
    grid = mesh_grid(ho, wo) + (2,)
    if a.dtype != np.int32 or a.ndim not in (3, 4) or tuple(a.shape[-3:]) != grid or a.size == 0:
        raise ValueError("mesh_check: mesh must be int32 %r or (N, ...), not %s %r" % (grid, a.dtype, a.shape))
    a = np.ascontiguousarray(a.reshape((-1,) + grid))
    lib = load()
    m = Mesh()
    m.out_h, m.out_w, m.filter, m.reserved = ho, wo, FILTER_CUBIC, 0
    if lib.mcraw_mesh_check(C.byref(m), a.ctypes.data_as(C.POINTER(C.c_int32)), int(a.shape[0]), int(width), int(height), 1 if inside else 0) != 0:
        raise ValueError(lib.mcraw_last_error().decode())


# display-ready integer RGB through a transfer-curve LUT (mcraw_demosaic_display_batch)
DISP_U8, DISP_U16 = 1, 2
DISP_CHW, DISP_HWC = 0, 1
_DISP_LAYOUTS = {"chw": DISP_CHW, "hwc": DISP_HWC}


class Display(C.Structure):
    """struct mcraw_display (include/mcraw_hip.h): output dtype, layout and the device LUT of L = 1 << lut_log2 entries."""
    _fields_ = [("dtype", C.c_uint32), ("layout", C.c_uint32), ("lut_log2", C.c_uint32), ("reserved", C.c_uint32),
                ("lut", C.c_void_p)]


# video-ready Y'CbCr 4:2:0 (mcraw_demosaic_yuv_batch)
YUV_NV12, YUV_P010 = 1, 2
_YUV_FORMATS = {"nv12": (YUV_NV12, 8, 12), "p010": (YUV_P010, 10, 16)}  # code, bits, default in_bits
_YUV_KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
_YUV_SH = tuple(range(24, 0, -1))  # candidates for sh, largest first


class Yuv(C.Structure):
    """struct mcraw_yuv (include/mcraw_hip.h): format, the device LUT and the integer matrix behind it."""
    _fields_ = [("format", C.c_uint32), ("lut_log2", C.c_uint32), ("in_bits", C.c_uint32), ("sh", C.c_uint32),
                ("y_off", C.c_int32), ("c_off", C.c_int32), ("cy", C.c_int32 * 3), ("cb", C.c_int32 * 3),
                ("cr", C.c_int32 * 3), ("reserved", C.c_uint32), ("lut", C.c_void_p)]


# lens-shading gain maps on mosaics (mcraw_shade_batch)
class Shade(C.Structure):
    """struct mcraw_shade (include/mcraw_hip.h): the device gain map (nmaps, 4, map_h, map_w) in Q3.12 by CFA position, the
    black levels the gain pivots on and the level the output saturates at."""
    _fields_ = [("map_w", C.c_uint32), ("map_h", C.c_uint32), ("nmaps", C.c_uint32), ("top", C.c_uint32),
                ("black", C.c_uint16 * 4), ("reserved", C.c_uint32 * 2), ("map", C.c_void_p)]


def gain_map(gains, cfa="rggb", order="rggb"):
    """The uint16 Q3.12 gain map of Context.shade / shading= from float gains (4, gh, gw) or (N, 4, gh, gw): entries
    rint(g * 4096), planes in CFA-position order p = (y & 1) * 2 + (x & 1) for the sensor arrangement `cfa`.  order "rggb":
    the planes of `gains` are R, G (red row), G (blue row), B and are permuted as cfa_planes(cfa) says; order "cfa": they are
    in CFA-position order already.  Raises ValueError on a non-finite or negative gain, or one that rounds above 32767
    (gains stay below 8)."""
    import numpy as np
    perm = cfa_planes(cfa)
    if order not in ("rggb", "cfa"):
        raise ValueError("order must be 'rggb' or 'cfa', not %r" % (order,))
    g = np.asarray(gains, dtype=np.float64)
    if g.ndim not in (3, 4) or g.shape[-3] != 4 or g.shape[-1] < 1 or g.shape[-2] < 1:
        raise ValueError("gain_map: gains must be (4, gh, gw) or (N, 4, gh, gw), not %r" % (g.shape,))
    if not np.all(np.isfinite(g)):
        raise ValueError("gain_map: non-finite gain")
    if np.any(g < 0):
        raise ValueError("gain_map: negative gain")
    q = np.rint(g * 4096.0)
    if np.any(q > 32767):
        raise ValueError("gain_map: a gain rounds above 32767 / 4096 (gains must stay below 8)")
    if order == "rggb":
        q = q[..., perm, :, :]
    return np.ascontiguousarray(q.astype(np.uint16))


def shading_map(frame_meta, cfa="rggb"):
    """The gain map (gain_map) of a frame's metadata, or None when it carries none: reads `lensShadingMap` -- four planes in
    Android's LensShadingMap order [R, G_even, G_odd, B], taken as R, G (red row), G (blue row), B, each a flat list of
    lensShadingMapHeight * lensShadingMapWidth gains in row-major order or a list of rows -- with `lensShadingMapWidth` /
    `lensShadingMapHeight`.
    UNVERIFIED: the key names and the layout are written from memory of the recorder's files; the reference reads none of
    these keys and no real clip was at hand.  All of the parsing is in this function: a clip that differs needs a change
    here only (or build the map with gain_map)."""
    import numpy as np
    if frame_meta is None or frame_meta.get("lensShadingMap") is None:
        return None
    planes = frame_meta["lensShadingMap"]
    if len(planes) != 4:
        raise ValueError("lensShadingMap must hold four planes, not %d" % len(planes))
    gw, gh = frame_meta.get("lensShadingMapWidth"), frame_meta.get("lensShadingMapHeight")
    out = []
    for pl in planes:
        a = np.asarray(pl, dtype=np.float64)
        if a.ndim == 1:
            if gw is None or gh is None or int(gw) * int(gh) != a.size:
                raise ValueError("lensShadingMap: a flat plane needs lensShadingMapWidth * lensShadingMapHeight == its length")
            a = a.reshape(int(gh), int(gw))
        elif a.ndim != 2 or (gw is not None and int(gw) != a.shape[1]) or (gh is not None and int(gh) != a.shape[0]):
            raise ValueError("lensShadingMap: a plane must be a flat list or lensShadingMapHeight rows of lensShadingMapWidth gains")
        out.append(a)
    if any(a.shape != out[0].shape for a in out):
        raise ValueError("lensShadingMap: the four planes differ in size")
    return gain_map(np.stack(out), cfa)


# per-frame statistics of mosaics (mcraw_stats_batch)
STATS_ACCUMULATE = 1


class Stats(C.Structure):
    """struct mcraw_stats (include/mcraw_hip.h): bins, shift, the window, the saturation levels by CFA position, flags."""
    _fields_ = [("bins_log2", C.c_uint32), ("shift", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32),
                ("h", C.c_uint32), ("sat", C.c_uint16 * 4), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class FrameStats:
    """What Context.stats returns: `raw`, the (N, record_bytes) uint8 tensor of mcraw_stats_batch's records ((record_bytes,)
    for an (H, W) mosaic), and exact views into it, by CFA position p = (y & 1) * 2 + (x & 1): hist (N, 4, bins) int32;
    cnt, nsat, min, max (N, 4) int32; sum (N, 4) int64 (the unsaturated samples only); bins and shift as given.  The signed
    views are exact because a frame of at most 65536 x 65536 has at most 2^30 samples per position; records that were
    accumulated into (accumulate=True) can pass 2^31, and their int32 views then show negative numbers: reinterpret them as
    unsigned.  The views are device tensors: reading them synchronises like any other tensor."""

    def __init__(self, raw, bins, shift):
        import torch
        self.raw, self.bins, self.shift = raw, int(bins), int(shift)
        nb = 16 * self.bins
        lead = tuple(raw.shape[:-1])
        words = raw[..., :nb + 64].view(torch.int32)
        self.hist = words[..., :4 * self.bins].unflatten(-1, (4, self.bins))
        small = words[..., 4 * self.bins:]
        self.cnt, self.nsat, self.min, self.max = (small[..., 4 * i:4 * i + 4] for i in range(4))
        self.sum = raw[..., nb + 64:nb + 96].view(torch.int64)
        assert tuple(self.sum.shape) == lead + (4,)

    def cpu(self):
        """The fields as numpy arrays on the host (a dict with hist, cnt, nsat, min, max, sum, bins, shift): what the
        stats_* helpers take."""
        d = {k: getattr(self, k).cpu().numpy() for k in ("hist", "cnt", "nsat", "min", "max", "sum")}
        d["bins"], d["shift"] = self.bins, self.shift
        return d


def _stats_arrays(st):
    """(fields as numpy arrays with a leading frame axis, whether that axis was added) of a FrameStats or of a mapping /
    object that holds its arrays on the CPU."""
    import numpy as np
    if isinstance(st, FrameStats):
        st = st.cpu()
    get = st.__getitem__ if isinstance(st, dict) else (lambda k: getattr(st, k))
    d = {k: np.asarray(get(k)).astype(np.int64) for k in ("hist", "cnt", "nsat", "sum")}
    d["shift"] = int(get("shift"))
    single = d["cnt"].ndim == 1
    if single:
        d = {k: (v[None] if k != "shift" else v) for k, v in d.items()}
    return d, single


def stats_white_balance(st, black=(0, 0, 0, 0), cfa="rggb"):
    """Grey-world white-balance gains (N, 3) float64, R, G, B with G = 1, from a FrameStats (or its arrays on the CPU): usable
    as gain= of the demosaic methods.  The mean of a CFA position is sum / (cnt - nsat) - black (the unsaturated samples
    only; black by CFA position, as everywhere); the two green positions are pooled by their counts; gain = mean G / mean
    of the channel.  A channel without an unsaturated sample, or with a mean <= 0, gets gain 1 (and so do both others when
    that channel is G).  A (4,)-shaped record gives (3,)."""
    import numpy as np
    d, single = _stats_arrays(st)
    plane = cfa_planes(cfa)  # plane[p]: 0 R, 1 G (R row), 2 G (B row), 3 B
    black = np.asarray(black, dtype=np.float64).ravel()
    if black.size != 4:
        raise ValueError("black: four levels, by CFA position (row & 1) * 2 + (col & 1)")
    good = (d["cnt"] - d["nsat"]).astype(np.float64)  # (N, 4) by position
    above = d["sum"].astype(np.float64) - good * black[None, :]  # sum of (v - black) over the unsaturated samples
    n = good.shape[0]
    tot, num = np.zeros((n, 3)), np.zeros((n, 3))
    for p in range(4):
        ch = (0, 1, 1, 2)[plane[p]]
        tot[:, ch] += good[:, p]
        num[:, ch] += above[:, p]
    mean = np.where(tot > 0, num / np.maximum(tot, 1.0), 0.0)
    gains = np.ones((n, 3))
    ok = mean > 0
    for ch in (0, 2):
        use = ok[:, ch] & ok[:, 1]
        gains[use, ch] = mean[use, 1] / mean[use, ch]
    return gains[0] if single else gains


def stats_percentile(st, q, pool=True):
    """The level below which the fraction q (0 .. 1) of the samples lies, from the histogram: the smallest bin b whose
    cumulative count reaches ceil(q * total) (bin 0 for q = 0), returned as that bin's upper edge
    min(((b + 1) << shift) - 1, 65535).  q * total is computed exactly (q may be a fractions.Fraction).  Per frame, (N,)
    int64, over the four CFA positions pooled, or (N, 4) per position with pool=False; usable as white=, or to match
    exposures."""
    import numpy as np
    from fractions import Fraction
    if not 0 <= q <= 1:
        raise ValueError("q must be in 0 .. 1")
    d, single = _stats_arrays(st)
    hist = d["hist"].sum(axis=1, keepdims=True) if pool else d["hist"]  # (N, 1 or 4, B)
    cum = np.cumsum(hist, axis=-1)
    total = cum[..., -1]
    fq = Fraction(q)
    need = np.array([-((-fq.numerator * int(t)) // fq.denominator) for t in total.ravel()],
                    dtype=np.int64).reshape(total.shape)  # ceil(q * total) in integers
    b = (cum < need[..., None]).sum(axis=-1)  # the first bin that reaches it; B when none does
    edge = np.minimum(((np.minimum(b, hist.shape[-1] - 1) + 1) << d["shift"]) - 1, 65535)
    if pool:
        edge = edge[:, 0]
    return edge[0] if single else edge


def stats_clipped(st):
    """nsat / cnt per frame and CFA position, (N, 4) float64 (0 where a position has no sample)."""
    import numpy as np
    d, single = _stats_arrays(st)
    r = d["nsat"] / np.maximum(d["cnt"], 1)
    return r[0] if single else r


# the noise measurement of mosaics (mcraw_noise_batch)
NOISE_ACCUMULATE = 1
NOISE_LEVELS, NOISE_BINS = 32, 128
NOISE_RECORD_BYTES = 4 * (4 * NOISE_LEVELS * NOISE_BINS + 8)


class Noise(C.Structure):
    """struct mcraw_noise (include/mcraw_hip.h): the level shift, the window, the rejection levels by CFA position, flags."""
    _fields_ = [("shift", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("sat", C.c_uint16 * 4), ("lo", C.c_uint16 * 4), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class NoiseStats:
    """What Context.noise_stats returns: `raw`, the (N, 65568) uint8 tensor of mcraw_noise_batch's records ((65568,) for an
    (H, W) mosaic), and exact views into it, by CFA position p = (y & 1) * 2 + (x & 1): hist (N, 4, 32, 128) int32, the
    count of accepted 16 x 16 blocks by level bin and energy bin; nblk, nrej (N, 4) int32, the accepted and the rejected
    ones; shift as given.  A frame has at most 2^24 blocks, so the signed views are exact; records that were accumulated
    into can pass 2^31: reinterpret them as unsigned.  The views are device tensors: reading them synchronises."""

    def __init__(self, raw, shift):
        import torch
        self.raw, self.shift = raw, int(shift)
        nh = 16 * NOISE_LEVELS * NOISE_BINS
        self.hist = raw[..., :nh].view(torch.int32).unflatten(-1, (4, NOISE_LEVELS, NOISE_BINS))
        self.nblk = raw[..., nh:nh + 16].view(torch.int32)
        self.nrej = raw[..., nh + 16:nh + 32].view(torch.int32)

    def cpu(self):
        """The fields as numpy arrays on the host (a dict with hist, nblk, nrej, shift): what noise_fit takes."""
        d = {k: getattr(self, k).cpu().numpy() for k in ("hist", "nblk", "nrej")}
        d["shift"] = self.shift
        return d


def _noise_energy(planes):
    """T of 8 x 8 planes (..., 8, 8) of integers: the sum of the 96 squared second differences along rows and columns."""
    import numpy as np
    b = np.asarray(planes).astype(np.int64)
    dh = b[..., :, :-2] - 2 * b[..., :, 1:-1] + b[..., :, 2:]
    dv = b[..., :-2, :] - 2 * b[..., 1:-1, :] + b[..., 2:, :]
    return (dh * dh).sum((-1, -2)) + (dv * dv).sum((-1, -2))


def _noise_energy_bin(T):
    """The energy bin of T (int64 array, 0 <= T < 2^53): 0 below 16, else min(4 * (e - 4) + f + 1, 127)."""
    import numpy as np
    T = np.asarray(T, dtype=np.int64)
    e = np.frexp(np.maximum(T, 16).astype(np.float64))[1].astype(np.int64) - 1  # floor(log2 T): exact below 2^53
    f = (np.maximum(T, 16) >> (e - 2)) & 3
    return np.where(T < 16, 0, np.minimum(4 * (e - 4) + f + 1, NOISE_BINS - 1))


def _noise_edge(vb):
    """The lower edge of energy bin vb >= 1: 2^e * (1 + f / 4)."""
    return float(1 << (4 + (vb - 1) // 4)) * (1.0 + ((vb - 1) % 4) / 4.0)


def _noise_quantile(counts, q):
    """The point below which the fraction q of a 128-bin energy histogram lies, linear in log2 between the edges of the bin
    that holds it.  Bins 0 and 127 have no two edges and never carry the answer: the point is clamped into bins 1 .. 126."""
    import numpy as np
    c = np.asarray(counts, dtype=np.float64)
    cum = np.cumsum(c)
    t = q * cum[-1]
    j = min(max(int(np.searchsorted(cum, t)), 1), NOISE_BINS - 2)
    fr = min(max((t - cum[j - 1]) / max(c[j], 1.0), 0.0), 1.0)
    lo, hi = np.log2(_noise_edge(j)), np.log2(_noise_edge(j + 1))
    return float(2.0 ** (lo + fr * (hi - lo)))


@functools.lru_cache(maxsize=None)
def noise_quantile_gain(quantile):
    """K(quantile): the `quantile` point of T / sigma^2 of pure Gaussian noise, by a seeded simulation through the stage's own
    arithmetic -- 3 x 16384 planes of rounded samples around level 32768 with sigma 16, 64 and 256, their T binned and the
    point read from the histogram as noise_fit reads it -- and the mean of the three.  The mean of T / sigma^2 is 576; the
    lower quantiles lie below it (K(0.15) is about 441, K(0.1) about 410).  Deterministic, cached per quantile."""
    import numpy as np
    rng = np.random.default_rng(0x6E6F6973)
    ks = []
    for sigma in (16.0, 64.0, 256.0):
        planes = np.rint(32768.0 + sigma * rng.standard_normal((16384, 8, 8))).astype(np.int64)
        h = np.bincount(_noise_energy_bin(_noise_energy(planes)), minlength=NOISE_BINS)
        ks.append(_noise_quantile(h, quantile) / sigma ** 2)
    return float(np.mean(ks))


def _noise_line(x, y, w):
    """Least squares of y = a * x + b with weights w under a, b >= 0: the free solution where it is feasible, else the better
    of the two on the boundary."""
    import numpy as np
    sw, sx, sy = w.sum(), (w * x).sum(), (w * y).sum()
    sxx, sxy = (w * x * x).sum(), (w * x * y).sum()
    det = sw * sxx - sx * sx
    if det > 0:
        a, b = (sw * sxy - sx * sy) / det, (sxx * sy - sx * sxy) / det
        if a >= 0 and b >= 0:
            return a, b
    cands = [(0.0, max(sy / sw, 0.0)), (max(sxy / sxx, 0.0) if sxx > 0 else 0.0, 0.0)]
    return min(cands, key=lambda ab: float((w * (ab[0] * x + ab[1] - y) ** 2).sum()))


def noise_fit(st, black, white, quantile=0.15, min_blocks=200, pool=True):
    """The noise profile (S, O) -- variance = S * x + O on values x normalised to [0, 1], per CFA position
    (row & 1) * 2 + (col & 1): what noise_lut takes -- from a NoiseStats (or its arrays on the CPU).  Each (4,) float64 over
    the frames pooled, or (N, 4) per frame with pool=False.  On the CPU in float64, deterministic.
    For every position p and level bin l with at least min_blocks accepted blocks the `quantile` point of the energy
    histogram is read (linear in log2 between the bin's edges; bins 0 and 127 never carry it) and divided by
    noise_quantile_gain(quantile), the same point of T / sigma^2 under pure Gaussian noise: the variance in DN^2 at the bin's
    mid level m = (l << shift) + (1 << shift) / 2.  A textured block or one across an edge can only raise T, so a low
    quantile follows the noise while most of a level's blocks may be textured.  var(m) = a * (m - black[p]) + b is fitted by
    least squares, a, b >= 0, the weight of a bin being its block count over the square of its variance (a quantile of n blocks is
    off by a fraction of itself that goes with 1 / sqrt(n)), and S = a / R, O = b / R^2 with R = white - black[p] invert
    noise_lut's formula.  Raises ValueError when fewer than two level bins of a position qualify."""
    import numpy as np
    if isinstance(st, NoiseStats):
        st = st.cpu()
    get = st.__getitem__ if isinstance(st, dict) else (lambda k: getattr(st, k))
    hist = np.asarray(get("hist")).astype(np.int64) & 0xFFFFFFFF
    shift = int(get("shift"))
    if hist.shape[-3:] != (4, NOISE_LEVELS, NOISE_BINS) or hist.ndim not in (3, 4):
        raise ValueError("noise_fit: hist must be (4, 32, 128) or (N, 4, 32, 128)")
    if not 0 < quantile < 1:
        raise ValueError("noise_fit: quantile must be inside 0 .. 1")
    hist = hist[None] if hist.ndim == 3 else hist
    if pool:
        hist = hist.sum(axis=0, keepdims=True)
    black = np.asarray(black, dtype=np.float64)
    black = np.full(4, float(black)) if black.ndim == 0 else black
    white = float(white)
    if black.shape != (4,) or not (white > black).all():
        raise ValueError("noise_fit: black is one level or four, by CFA position, and white lies above them")
    K = noise_quantile_gain(float(quantile))
    mid = (np.arange(NOISE_LEVELS, dtype=np.float64) * (1 << shift)) + (1 << shift) / 2.0
    S, O = np.zeros((hist.shape[0], 4)), np.zeros((hist.shape[0], 4))
    for f in range(hist.shape[0]):
        for p in range(4):
            cnt = hist[f, p].sum(axis=-1)
            use = np.nonzero(cnt >= max(int(min_blocks), 1))[0]
            if use.size < 2:
                raise ValueError("noise_fit: CFA position %d%s has %d level bins with at least %d accepted blocks, two are "
                                 "needed (blocks by level bin: %s)" % (p, "" if pool else " of frame %d" % f, use.size,
                                                                       min_blocks, cnt.tolist()))
            var = np.array([_noise_quantile(hist[f, p, l], quantile) / K for l in use])
            # A quantile of n blocks is off by a fraction of itself that goes with 1 / sqrt(n), whatever the variance: the weight
            # of a bin is n / var^2, var first as measured, then twice as fitted (a measured one would favour the bins that
            # came out low).
            x, model = mid[use] - black[p], var
            for _ in range(3):
                a, b = _noise_line(x, var, cnt[use] / (model * model))
                model = np.maximum(a * x + b, 0.25 * var)
            R = white - black[p]
            S[f, p], O[f, p] = a / R, b / (R * R)
    return (S[0], O[0]) if pool else (S, O)


# defective pixels of mosaics (mcraw_fixpix_batch)
FIXPIX_HOT, FIXPIX_COLD = 1, 2
FIXPIX_MAX_LIST = 1 << 20


class FixPix(C.Structure):
    """struct mcraw_fixpix (include/mcraw_hip.h): flags, rank, the thresholds and black levels by CFA position, the device
    list of packed pixels and the device records of the counts."""
    _fields_ = [("flags", C.c_uint32), ("rank", C.c_uint32), ("rel_thr", C.c_uint32), ("nlist", C.c_uint32),
                ("black", C.c_uint16 * 4), ("abs_thr", C.c_uint16 * 4), ("list", C.c_void_p), ("counts", C.c_void_p),
                ("reserved", C.c_uint32 * 2)]


def pack_pixels(xy):
    """The static list of Context.fix_pixels / defects= from pixel coordinates: an integer array (K, 2) of (x, y) -> the
    uint32 entries y << 16 | x, ascending and without duplicates (what mcraw_fixpix_batch's search expects).  K = 0 gives an
    empty list.  Raises ValueError on another shape, a non-integer dtype, a coordinate outside 0 .. 65535, or more than
    1 << 20 distinct pixels.  (Android's hotPixelMap is such a list of (x, y); under which key a .mcraw file carries it is
    UNVERIFIED -- the reference reads no such key and no real clip was at hand -- so no helper here guesses it.)"""
    import numpy as np
    a = np.asarray(xy)
    if a.ndim != 2 or a.shape[1] != 2:
        if a.size == 0:
            return np.zeros(0, np.uint32)
        raise ValueError("pack_pixels: pixels must be (K, 2) of (x, y), not %r" % (a.shape,))
    if a.dtype.kind not in "iu":
        raise ValueError("pack_pixels: pixel coordinates must be integers, not %s" % a.dtype)
    if a.size and (int(a.min()) < 0 or int(a.max()) > 65535):
        raise ValueError("pack_pixels: a coordinate outside 0 .. 65535")
    a = a.astype(np.uint32)
    packed = np.unique((a[:, 1] << np.uint32(16)) | a[:, 0])  # ascending, duplicates gone
    if packed.size > FIXPIX_MAX_LIST:
        raise ValueError("pack_pixels: more than %d pixels" % FIXPIX_MAX_LIST)
    return np.ascontiguousarray(packed, dtype=np.uint32)


# clipped highlights of mosaics (mcraw_highlights_batch, mcraw_highlights_measure_batch)
HL_CLIP, HL_REBUILD = 0, 1
HL_ACCUMULATE = 1
_HL_MODES = {"clip": HL_CLIP, "rebuild": HL_REBUILD}
_HL_KEYS = ("sat", "black", "gain", "cfa", "mode", "chroma", "lo", "top")


class Highlights(C.Structure):
    """struct mcraw_highlights (include/mcraw_hip.h): mode, cfa, flags, top, then black, sat, gain (Q4.12) and lo by CFA
    position, the device records and how many there are."""
    _fields_ = [("mode", C.c_uint32), ("cfa", C.c_uint32), ("flags", C.c_uint32), ("top", C.c_uint32),
                ("black", C.c_uint16 * 4), ("sat", C.c_uint16 * 4), ("gain", C.c_uint16 * 4), ("lo", C.c_uint16 * 4),
                ("rec", C.c_void_p), ("nrec", C.c_uint32), ("reserved", C.c_uint32)]


class HighlightChroma:
    """The records of Context.highlight_chroma: `raw`, an int64 tensor (R, 8) of R records of 64 bytes as the library lays them
    out (R: N, or 1 for the whole batch); `sum`, int64 (R, 4), and `cnt`, int32 (R, 4), are views of it by CFA position: the sum
    of v - ref over the pixels that took part and how many there were."""

    def __init__(self, raw):
        import torch
        self.raw = raw
        self.sum = raw[:, :4]
        self.cnt = raw.view(torch.int32)[:, 8:12]

    def cpu(self):
        """(sum int64 (R, 4), cnt uint32 (R, 4)) as numpy arrays; synchronises."""
        import numpy as np
        a = self.raw.cpu().numpy()
        return a[:, :4].copy(), np.ascontiguousarray(a[:, 4:6]).view(np.uint32).copy()


def highlight_gains(gain, cfa="rggb"):
    """The white-balance gains (r, g, b) that the demosaic methods take (rgb_color gives them) as the highlight stage takes
    them: four Q4.12 integers by CFA position p = (y & 1) * 2 + (x & 1) for the sensor arrangement `cfa`, rint(g * 4096), where
    16.0 itself becomes 65535.  Raises ValueError for a gain outside 1/16 .. 16 or not finite."""
    import numpy as np
    planes = cfa_planes(cfa)  # plane[p]: 0 R, 1 G (R row), 2 G (B row), 3 B
    g = np.asarray(gain, dtype=np.float64).reshape(-1)
    if g.size != 3 or not np.isfinite(g).all() or (g < 1.0 / 16.0).any() or (g > 16.0).any():
        raise ValueError("highlight_gains: gain must be three finite values (r, g, b) in 1/16 .. 16, not %r" % (gain,))
    q = np.minimum(np.rint(g * 4096.0), 65535.0).astype(np.int64)
    return [int(q[(0, 1, 1, 2)[planes[p]]]) for p in range(4)]


def _hl_struct(fn, sat, black, gain, cfa, lo, top, mode):
    """struct mcraw_highlights for method `fn` from its arguments (rec, nrec and flags are left 0)."""
    key = str(cfa).strip().lower()
    if key not in _CFA_CODES:
        raise ValueError("unknown cfa %r (rggb, bggr, grbg or gbrg)" % (cfa,))
    if mode not in _HL_MODES:
        raise ValueError("%s: mode must be 'rebuild' or 'clip', not %r" % (fn, mode))
    four = lambda v: [v] * 4 if not hasattr(v, "__len__") else list(v)
    sat, black = four(sat), four(black)
    if len(sat) != 4 or len(black) != 4 or any(v != int(v) or v < 0 or v > 65535 for v in sat + black):
        raise ValueError("%s: sat and black are one level or four, by CFA position (row & 1) * 2 + (col & 1), each an integer "
                         "0 .. 65535" % fn)
    sat, black = [int(v) for v in sat], [int(v) for v in black]
    if any(s <= b for s, b in zip(sat, black)):
        raise ValueError("%s: sat must be above black at every CFA position" % fn)
    if gain is None:
        raise ValueError("%s: gain is needed: (r, g, b) as the demosaic takes them, or four Q4.12 integers by CFA position" % fn)
    gain = list(gain)
    if len(gain) == 3:
        gain = highlight_gains(gain, key)
    elif len(gain) != 4 or any(v != int(v) or v < 256 or v > 65535 for v in gain):
        raise ValueError("%s: gain is (r, g, b), or four Q4.12 integers 256 .. 65535 by CFA position" % fn)
    lo = [b + (s - b) // 2 for s, b in zip(sat, black)] if lo is None else four(lo)
    if len(lo) != 4 or any(v != int(v) or v < 0 or v > 65535 for v in lo):
        raise ValueError("%s: lo is one level or four, each an integer 0 .. 65535" % fn)
    if top != int(top) or top < 1 or top > 65535:
        raise ValueError("%s: top must be an integer 1 .. 65535, not %r" % (fn, top))
    s = Highlights()
    s.mode, s.cfa, s.flags, s.top = _HL_MODES[mode], _CFA_CODES[key], 0, int(top)
    for i in range(4):
        s.black[i], s.sat[i], s.gain[i], s.lo[i] = black[i], sat[i], int(gain[i]), int(lo[i])
    s.rec, s.nrec, s.reserved = None, 0, 0
    return s


def _hl_kwargs(fn, highlights, white, black, cfa, gain):
    """The keyword arguments of Context.highlights() for highlights= of method `fn`: the dict's own, and for what it leaves out
    the method's: sat from white, black, cfa and gain.  Raises ValueError for what is no dict, an unknown key, a gain per frame
    with none in the dict (the stage takes one gain for the batch) and a fractional white without a sat."""
    import numpy as np
    if not isinstance(highlights, dict):
        raise ValueError("%s: highlights must be a dict of highlights()' keyword arguments (without out)" % fn)
    unknown = [k for k in highlights if k not in _HL_KEYS]
    if unknown:
        raise ValueError("%s: highlights has no key %r (%s)" % (fn, unknown[0], ", ".join(_HL_KEYS)))
    kw = dict(highlights)
    if "gain" not in kw:
        g = None if gain is None else np.asarray(gain.cpu() if hasattr(gain, "cpu") else gain, dtype=np.float64)
        if g is not None and g.ndim > 1:
            raise ValueError("%s: highlights takes one gain for the batch; with a gain per frame give it one of its own "
                             "('gain': (r, g, b))" % fn)
        kw["gain"] = (1.0, 1.0, 1.0) if g is None else tuple(float(v) for v in g)
    if "sat" not in kw:
        if white != int(white):
            raise ValueError("%s: highlights needs an integer 'sat' when white=%r is none" % (fn, white))
        kw["sat"] = int(white)
    kw.setdefault("black", black)
    kw.setdefault("cfa", cfa)
    return kw


# noise-adaptive denoising of mosaics (mcraw_denoise_batch)
class Denoise(C.Structure):
    """struct mcraw_denoise (include/mcraw_hip.h): radius, amount in Q8, the table's size and shift, how many tables, and the
    device table (nluts, 4, L) of uint16."""
    _fields_ = [("radius", C.c_uint32), ("amount", C.c_uint32), ("lut_log2", C.c_uint32), ("shift", C.c_uint32),
                ("nluts", C.c_uint32), ("reserved", C.c_uint32 * 3), ("lut", C.c_void_p)]


# noise-adaptive temporal merge of mosaics (mcraw_merge_batch)
class Merge(C.Structure):
    """struct mcraw_merge (include/mcraw_hip.h): the window, the outputs, the motion measure, amount in Q8, the table's size
    and shift, how many tables, the device table (nluts, 4, L) of uint16 and the device positions (n, 2) of int16 or NULL."""
    _fields_ = [("before", C.c_uint32), ("after", C.c_uint32), ("first", C.c_uint32), ("count", C.c_uint32),
                ("support", C.c_uint32), ("amount", C.c_uint32), ("lut_log2", C.c_uint32), ("shift", C.c_uint32),
                ("nluts", C.c_uint32), ("reserved", C.c_uint32), ("lut", C.c_void_p), ("pos", C.c_void_p)]


# per-frame global shifts of mosaics (mcraw_align_batch)
class Align(C.Structure):
    """struct mcraw_align (include/mcraw_hip.h): the pyramid's levels, the coarsest level's radius, the reference frame (-1: a
    chain), the blacks, the device outputs pos (n, 2) int16 and sad (n) uint64 or NULL, and the device scratch with its size."""
    _fields_ = [("levels", C.c_uint32), ("radius", C.c_uint32), ("ref", C.c_int32), ("reserved", C.c_uint32),
                ("black", C.c_uint16 * 4), ("pos", C.c_void_p), ("sad", C.c_void_p), ("work", C.c_void_p),
                ("work_bytes", C.c_size_t)]


# a field of local shifts, one per cell of every frame (mcraw_align_cells_batch), and the merge that follows it (mcraw_merge_cells_batch)
class AlignCells(C.Structure):
    """struct mcraw_align_cells (include/mcraw_hip.h): the pyramid's levels (1 .. 3), the coarsest level's radius (1 .. 4), the
    reference frame (-1: a chain), the cell in samples, the blacks, the device centres gpos (n, 2) int16 or NULL, the device
    outputs pos (n, cells_y, cells_x, 2) int16 and sad (n, cells_y, cells_x) uint64 or NULL, and the device scratch with its size."""
    _fields_ = [("levels", C.c_uint32), ("radius", C.c_uint32), ("ref", C.c_int32), ("reserved", C.c_uint32),
                ("cell_h", C.c_uint32), ("cell_w", C.c_uint32), ("black", C.c_uint16 * 4), ("gpos", C.c_void_p),
                ("pos", C.c_void_p), ("sad", C.c_void_p), ("work", C.c_void_p), ("work_bytes", C.c_size_t)]


class Cells(C.Structure):
    """struct mcraw_cells (include/mcraw_hip.h): the cell in samples, the grid's size and the device field (n, cells_y, cells_x,
    2) of int16 that mcraw_merge_cells_batch reads."""
    _fields_ = [("cell_h", C.c_uint32), ("cell_w", C.c_uint32), ("cells_y", C.c_uint32), ("cells_x", C.c_uint32),
                ("reserved", C.c_uint32), ("pos", C.c_void_p)]


def cell_grid(height, width, cell=(64, 256)):
    """(cells_y, cells_x) of the position field of height x width frames for cells of cell = (cell_h, cell_w) samples: the
    ceilings.  Raises ValueError for a cell_h that is no multiple of 32 or a cell_w that is no multiple of 256 (host only)."""
    try:
        ch, cw = cell
    except (TypeError, ValueError):
        raise ValueError("cell must be (cell_h, cell_w), not %r" % (cell,))
    for name, v, g in (("cell_h", ch, 32), ("cell_w", cw, 256)):
        if isinstance(v, bool) or v != int(v) or int(v) < g or int(v) % g or int(v) > 65536:
            raise ValueError("cell: %s must be a multiple of %d in %d .. 65536, not %r" % (name, g, g, v))
    return (int(height) + int(ch) - 1) // int(ch), (int(width) + int(cw) - 1) // int(cw)


def align_window(height, width, levels=4, radius=4):
    """(rows, columns) of the level-0 comparison window of Context.align for frames of height x width: what its `sad` is summed
    over, (height // 2 - 2 * B0, width // 2 - 2 * B0) with B(levels - 1) = radius, B(l) = 2 * B(l + 1) + 1.  Raises ValueError
    for levels outside 1 .. 6, radius outside 1 .. 8, and for frames so small that the window is empty at a level: what the
    library would reject (host only, no GPU needed)."""
    for name, v, lo, hi in (("levels", levels, 1, 6), ("radius", radius, 1, 8)):
        if isinstance(v, bool) or v != int(v) or not lo <= int(v) <= hi:
            raise ValueError("align: %s must be an integer %d .. %d, not %r" % (name, lo, hi, v))
    levels, B = int(levels), int(radius)
    if isinstance(height, bool) or isinstance(width, bool) or height != int(height) or width != int(width) \
            or not (1 <= int(height) <= 65536 and 1 <= int(width) <= 65536):
        raise ValueError("align: height and width must be integers 1 .. 65536, not %r x %r" % (height, width))
    h, w = int(height) // 2, int(width) // 2
    for l in range(levels - 1, -1, -1):  # coarsest first
        if (h >> l) - 2 * B < 1 or (w >> l) - 2 * B < 1:
            raise ValueError("align: %d x %d frames leave no comparison window at level %d (a %d x %d plane, margin %d): fewer "
                             "levels, a smaller radius or larger frames" % (height, width, l, h >> l, w >> l, B))
        if l:
            B = 2 * B + 1
    return h - 2 * B, w - 2 * B


def noise_lut(S, O, black, white, strength=3.0, entries=256, top=None):
    """The table of Context.denoise / denoise= from a noise profile: variance = S * x + O on values x normalised to [0, 1],
    the form in which Android's noiseProfile and DNG's NoiseProfile state it.  S, O, black: scalars or four values by CFA
    position (row & 1) * 2 + (col & 1); white: the white level; top: the largest value the table has to tell apart (white
    unless given).  Returns (lut, shift): shift is the smallest one with (top >> shift) < entries, lut is uint16 (4,
    entries); entry i of position p, in float64, with m = (i << shift) + (1 << shift) / 2 and R = white - black[p]:
    var = S[p] * R * max(m - black[p], 0) + O[p] * R * R in DN^2, entry = clip(rint(4096 / (strength * sqrt(var))), 1,
    65535), and 65535 where var is 0 -- the weight of a neighbour reaches 0 at `strength` standard deviations.  Raises
    ValueError for entries that is not a power of two in 64 .. 1024, white <= black, a negative S or O, or strength <= 0."""
    import numpy as np

    def four(v, name):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(4, float(a))
        if a.shape != (4,) or not np.isfinite(a).all():
            raise ValueError("noise_lut: %s is one finite value or four, by CFA position" % name)
        return a

    S, O, black = four(S, "S"), four(O, "O"), four(black, "black")
    entries = int(entries)
    if entries not in (64, 128, 256, 512, 1024):
        raise ValueError("noise_lut: entries must be a power of two in 64 .. 1024, not %r" % (entries,))
    white = float(white)
    if not np.isfinite(white) or (white <= black).any():
        raise ValueError("noise_lut: white must be above every black level")
    if (S < 0).any() or (O < 0).any():
        raise ValueError("noise_lut: S and O must not be negative")
    strength = float(strength)
    if not strength > 0 or not np.isfinite(strength):
        raise ValueError("noise_lut: strength must be above 0, not %r" % (strength,))
    top = int(white if top is None else top)
    if top < 0 or top > 65535:
        raise ValueError("noise_lut: top must be 0 .. 65535")
    shift = 0
    while (top >> shift) >= entries:
        shift += 1
    m = (np.arange(entries, dtype=np.float64) * (1 << shift) + (1 << shift) / 2.0)[None, :]
    R = (white - black)[:, None]
    var = S[:, None] * R * np.maximum(m - black[:, None], 0.0) + O[:, None] * R * R
    with np.errstate(divide="ignore"):
        e = np.where(var > 0, np.clip(np.rint(4096.0 / (strength * np.sqrt(var))), 1, 65535), 65535)
    return np.ascontiguousarray(e, dtype=np.uint16), shift


def _yuv_rule_ok(rows, sh, in_bits):
    """The overflow rule of mcraw_demosaic_yuv_batch: no int32 sum can wrap."""
    return all(4 * ((1 << in_bits) - 1) * sum(abs(int(c)) for c in r) + (1 << (sh + 1)) < (1 << 31) for r in rows)


def yuv_matrix(standard="bt709", range="limited", bits=8, in_bits=8):
    """(cy, cb, cr, sh, y_off, c_off) as Python ints for mcraw_demosaic_yuv_batch: the R'G'B' -> Y'CbCr matrix of
    `standard` ("bt601", "bt709", "bt2020") for LUT entries of `in_bits` (8 .. 16) bits and codes of `bits` (8 or 10) bits,
    range "limited" (luma 16 .. 235, chroma 16 .. 240, times 2^(bits - 8)) or "full" (0 .. 2^bits - 1, chroma centred on
    2^(bits - 1)).  sh is the largest the overflow rule admits; the coefficients are the scaled ones rounded to nearest,
    then the G entry of each row is corrected so that sum(cb) == sum(cr) == 0 and sum(cy) == rint(luma_span * 2^sh /
    (2^in_bits - 1)): greys are exactly neutral, and black and white land exactly on the ends of the range."""
    key = standard.lower() if isinstance(standard, str) else None
    if key not in _YUV_KR_KB:
        raise ValueError("yuv_matrix: standard must be 'bt601', 'bt709' or 'bt2020', not %r" % (standard,))
    if range not in ("limited", "full"):
        raise ValueError("yuv_matrix: range must be 'limited' or 'full', not %r" % (range,))
    if isinstance(bits, bool) or bits not in (8, 10):
        raise ValueError("yuv_matrix: bits must be 8 or 10, not %r" % (bits,))
    if isinstance(in_bits, bool) or in_bits not in (8, 9, 10, 11, 12, 13, 14, 15, 16):
        raise ValueError("yuv_matrix: in_bits must be 8 .. 16, not %r" % (in_bits,))
    return _yuv_matrix(key, range == "limited", int(bits), int(in_bits))


@functools.lru_cache(maxsize=None)
def _yuv_matrix(key, limited, bits, in_bits):
    """yuv_matrix behind its argument checks, in exact rational arithmetic (once per combination: demosaic_yuv asks on
    every call)."""
    from fractions import Fraction as F
    kr, kb = (F(str(v)) for v in _YUV_KR_KB[key])
    kg = 1 - kr - kb
    if limited:
        luma, chroma, y_off, c_off = 219 << (bits - 8), 224 << (bits - 8), 16 << (bits - 8), 128 << (bits - 8)
    else:
        luma, chroma, y_off, c_off = (1 << bits) - 1, (1 << bits) - 1, 0, 1 << (bits - 1)
    top_in = (1 << in_bits) - 1
    fy = [k * luma / top_in for k in (kr, kg, kb)]
    fcb = [k * chroma / (2 * (1 - kb)) / top_in for k in (-kr, -kg, 1 - kb)]
    fcr = [k * chroma / (2 * (1 - kr)) / top_in for k in (1 - kr, -kg, -kb)]
    rint = lambda v: int(round(v))  # (Fraction: exact, ties to even)
    for sh in _YUV_SH:
        cy, cb, cr = ([rint(v * (1 << sh)) for v in row] for row in (fy, fcb, fcr))
        cy[1] = rint(F(luma << sh, top_in)) - cy[0] - cy[2]
        cb[1] = -(cb[0] + cb[2])
        cr[1] = -(cr[0] + cr[2])
        if _yuv_rule_ok((cy, cb, cr), sh, in_bits):
            return tuple(cy), tuple(cb), tuple(cr), sh, y_off, c_off
    raise ValueError("yuv_matrix: no sh satisfies the overflow rule")  # (not reachable for the arguments accepted above)


def yuv_planes(t, Ho):
    """(Y, CbCr) as views of a demosaic_yuv / decode_yuv result (N, Ho * 3 // 2, Wo): Y (N, Ho, Wo) and the interleaved
    chroma (N, Ho / 2, Wo / 2, 2), [..., 0] = Cb, [..., 1] = Cr (a result without N gives planes without N)."""
    Ho = int(Ho)
    if t.shape[-2] != Ho * 3 // 2 or Ho % 2 or t.shape[-1] % 2:
        raise ValueError("yuv_planes: %s is no (.., Ho * 3 // 2, Wo) result for Ho = %d" % (tuple(t.shape), Ho))
    return t[..., :Ho, :], t[..., Ho:, :].reshape(tuple(t.shape[:-2]) + (Ho // 2, t.shape[-1] // 2, 2))


def _srgb_oetf(x):
    import numpy as np
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)


def _bt709_oetf(x):
    import numpy as np
    return np.where(x < 0.018, 4.5 * x, 1.099 * np.power(x, 0.45) - 0.099)


def transfer_lut(curve="srgb", size=4096, bits=8):
    """uint16 numpy array of `size` entries: code[k] = rint(f(k / (size - 1)) * (2**bits - 1)), f evaluated in float64 and
    clamped to [0, 1].  curve: "linear", "srgb" (IEC 61966-2-1), "bt709" (4.5 x below 0.018, else 1.099 x^0.45 - 0.099), a
    number g for x ** (1 / g), or a callable on [0, 1] (numpy array in, array out).  size: a power of two, 256 .. 65536;
    bits: 8, 10, 12 or 16."""
    import numpy as np
    size, bits = int(size), int(bits)
    if size < 256 or size > 65536 or size & (size - 1):
        raise ValueError("transfer_lut: size must be a power of two, 256 .. 65536, not %d" % size)
    if bits not in (8, 10, 12, 16):
        raise ValueError("transfer_lut: bits must be 8, 10, 12 or 16, not %d" % bits)
    x = np.arange(size, dtype=np.float64) / float(size - 1)
    if callable(curve):
        f = curve
    elif isinstance(curve, str):
        f = {"linear": lambda v: v, "srgb": _srgb_oetf, "bt709": _bt709_oetf}.get(curve.lower())
        if f is None:
            raise ValueError("transfer_lut: unknown curve %r (linear, srgb, bt709, a gamma or a callable)" % (curve,))
    elif isinstance(curve, (int, float)) and not isinstance(curve, bool):
        g = float(curve)
        if not (g > 0.0) or g == float("inf"):
            raise ValueError("transfer_lut: the gamma must be finite and positive, not %r" % (curve,))
        f = lambda v: np.power(v, 1.0 / g)
    else:
        raise ValueError("transfer_lut: curve must be a name, a number or a callable, not %r" % (curve,))
    y = np.asarray(f(x), dtype=np.float64)
    if y.shape != x.shape or not np.isfinite(y).all():
        raise ValueError("transfer_lut: the curve must give one finite value per input")
    return np.rint(np.clip(y, 0.0, 1.0) * float((1 << bits) - 1)).astype(np.uint16)


def _rgb_colors(gain, matrix, n, fn):
    """(RgbColor array, ncolors) of gain (3,) / (N, 3) and matrix (3, 3) / (N, 3, 3): one set, or one per frame."""
    import numpy as np
    gain = np.ones(3, np.float32) if gain is None else np.asarray(gain, dtype=np.float32)
    matrix = np.eye(3, dtype=np.float32) if matrix is None else np.asarray(matrix, dtype=np.float32)
    per = gain.ndim == 2 or matrix.ndim == 3
    if gain.shape not in ((3,), (n, 3)) or matrix.shape not in ((3, 3), (n, 3, 3)):
        raise ValueError("%s: gain (3,) or (N, 3), matrix (3, 3) or (N, 3, 3)" % fn)
    nc = n if per else 1
    gains = np.broadcast_to(gain, (nc, 3)) if gain.ndim == 1 else gain
    mats = np.broadcast_to(matrix, (nc, 3, 3)) if matrix.ndim == 2 else matrix
    cols = (RgbColor * nc)()
    for i in range(nc):
        for c in range(3):
            cols[i].gain[c] = float(gains[i, c])
        for j in range(9):
            cols[i].m[j] = float(mats[i].ravel()[j])
    return cols, nc


def _rgb_params(algo, dtype_code, flags, cfa_key, white, black):
    prm = RgbParams()
    prm.algo, prm.dtype, prm.flags, prm.cfa = _RGB_ALGOS[algo], dtype_code, flags, _CFA_CODES[cfa_key]
    black = list(black)
    if len(black) != 4:
        raise ValueError("black: four levels, by CFA position (y & 1) * 2 + (x & 1)")
    for i in range(4):
        prm.black[i] = int(black[i])
    prm.white = float(white)
    return prm


def _xyz_d50_to_srgb():
    """Linear sRGB (D65) from XYZ (D50): Bradford adaptation D50 -> D65, then the inverse of the sRGB primaries' matrix."""
    import numpy as np
    d50 = np.array([0.96422, 1.0, 0.82521])
    d65 = np.array([0.95047, 1.0, 1.08883])
    xy = np.array([[0.64, 0.33], [0.30, 0.60], [0.15, 0.06]])
    prim = np.stack([xy[:, 0] / xy[:, 1], np.ones(3), (1 - xy[:, 0] - xy[:, 1]) / xy[:, 1]])  # columns: XYZ of R, G, B
    rgb_to_xyz = prim * np.linalg.solve(prim, d65)[None, :]
    brad = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]])
    adapt = np.linalg.inv(brad) @ np.diag((brad @ d65) / (brad @ d50)) @ brad
    return np.linalg.inv(rgb_to_xyz) @ adapt


def rgb_color(container_meta, frame_meta=None, space="srgb"):
    """(gain[3], m[3][3]) as float32 for Context.demosaic / decode_rgb, from the clip's metadata, computed in float64 and
    rounded once.  gain = 1 / asShotNeutral of the frame (ones without frame metadata).  space: "camera" (identity: white-
    balanced camera RGB), "xyz" (forwardMatrix1: white-balanced camera RGB to XYZ D50) or "srgb" (linear sRGB, D65: the
    Bradford-adapted XYZ(D50) -> sRGB matrix times forwardMatrix1).  The DNG calibration illuminant 1 of these clips is D65;
    interpolating between forwardMatrix1 and forwardMatrix2 by colour temperature is not done.  A missing or all-zero
    forwardMatrix1 raises ValueError (for "xyz" and "srgb")."""
    import numpy as np
    if space not in ("camera", "xyz", "srgb"):
        raise ValueError("space must be 'camera', 'xyz' or 'srgb', not %r" % (space,))
    if frame_meta is not None and frame_meta.get("asShotNeutral") is not None:
        neutral = np.asarray(frame_meta["asShotNeutral"], dtype=np.float64).ravel()
        if neutral.size != 3 or not np.all(np.isfinite(neutral)) or np.any(neutral <= 0):
            raise ValueError("asShotNeutral must be three positive numbers, not %r" % (frame_meta["asShotNeutral"],))
        gain = 1.0 / neutral
    else:
        gain = np.ones(3)
    if space == "camera":
        m = np.eye(3)
    else:
        fm = container_meta.get("forwardMatrix1") if container_meta is not None else None
        fm = None if fm is None else np.asarray(fm, dtype=np.float64).ravel()
        if fm is None or fm.size != 9 or not np.any(fm) or not np.all(np.isfinite(fm)):
            raise ValueError("the container has no usable forwardMatrix1 (nine numbers, not all zero)")
        m = fm.reshape(3, 3)
        if space == "srgb":
            m = _xyz_d50_to_srgb() @ m
    return gain.astype(np.float32), m.astype(np.float32)


class Frame(C.Structure):
    """struct mcraw_frame (include/mcraw_hip.h)."""
    _fields_ = [("in_", C.c_void_p), ("len", C.c_size_t), ("width", C.c_int32), ("height", C.c_int32),
                ("type", C.c_int32), ("reserved", C.c_int32), ("out", C.c_void_p), ("out_capacity", C.c_size_t)]


class EncFrame(C.Structure):
    """struct mcraw_enc_frame (include/mcraw_hip.h)."""
    _fields_ = [("in_", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("out", C.c_void_p),
                ("out_capacity", C.c_size_t), ("len_out", C.c_void_p)]


def lib_path():
    # MCRAW_LIB_PATH: load another build of the same ABI (A/B timing of kernel variants on one box)
    return os.environ.get("MCRAW_LIB_PATH") or os.path.join(_PKG, "lib", "libmcraw_hip.so")


_lib = None


def load():
    """Load libmcraw_hip.so; raises McrawError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p) and "MCRAW_LIB_PATH" not in os.environ:
        try:  # a fresh checkout: compile the kernels now (hipcc, ~40 s); this is a build step, not a fallback
            from . import build as _build
            _build.build_hip()
        except Exception as e:
            raise McrawError("HIP decode library not built and building it failed (%s): %s; "
                             "there is no CPU fallback" % (e, p))
    if not os.path.exists(p):
        raise McrawError("HIP decode library not built: %s (run `python -m motioncam_decoder_amd.build`); "
                         "there is no CPU fallback" % p)
    # A process that also uses torch must share ONE HIP runtime with it: torch bundles its
    # own libamdhip64 (same SONAME as /opt/rocm's).  Loading torch first makes this library
    # bind to the runtime torch initialises; the other order maps two runtimes and the
    # second one sees no device.  (A C++ host without torch simply uses /opt/rocm's.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    lib.mcraw_ctx_create.restype = C.c_int
    lib.mcraw_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.mcraw_ctx_destroy.restype = None
    lib.mcraw_ctx_destroy.argtypes = [C.c_void_p]
    lib.mcraw_last_error.restype = C.c_char_p
    lib.mcraw_last_error.argtypes = []
    for name in ("mcraw_decode7", "mcraw_decode6"):
        fn = getattr(lib, name)
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.mcraw_decode_batch.restype = C.c_int
    lib.mcraw_decode_batch.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int, C.c_int, C.c_void_p,
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    lib.mcraw_ctx_synchronize.restype = C.c_int
    lib.mcraw_ctx_synchronize.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    lib.mcraw_ctx_last_serial.restype = C.c_uint64
    lib.mcraw_ctx_last_serial.argtypes = [C.c_void_p]
    lib.mcraw_ctx_batch_status.restype = C.c_int
    lib.mcraw_ctx_batch_status.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.c_int]
    lib.mcraw_ctx_errors.restype = C.c_int32
    lib.mcraw_ctx_errors.argtypes = [C.c_void_p, C.c_int]
    lib.mcraw_ctx_profile.restype = C.c_int
    lib.mcraw_ctx_profile.argtypes = [C.c_void_p, C.c_int]
    lib.mcraw_ctx_profile_every.restype = C.c_int
    lib.mcraw_ctx_profile_every.argtypes = [C.c_void_p, C.c_int]
    lib.mcraw_ctx_kernel_ms.restype = C.c_int
    lib.mcraw_ctx_kernel_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]
    lib.mcraw_host_alloc.restype = C.c_void_p
    lib.mcraw_host_alloc.argtypes = [C.c_size_t]
    lib.mcraw_host_free.restype = None
    lib.mcraw_host_free.argtypes = [C.c_void_p]
    lib.mcraw_decode_batch_async.restype = C.c_int
    lib.mcraw_decode_batch_async.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int, C.POINTER(C.c_void_p)]
    lib.mcraw_ticket_wait.restype = C.c_int
    lib.mcraw_ticket_wait.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    lib.mcraw_ctx_set_post.restype = C.c_int
    lib.mcraw_ctx_set_post.argtypes = [C.c_void_p, C.POINTER(Post)]
    lib.mcraw_shard_of.restype = C.c_int
    lib.mcraw_shard_of.argtypes = [C.c_long, C.c_int]
    lib.mcraw_shard_count.restype = C.c_int
    lib.mcraw_shard_count.argtypes = [C.c_long, C.c_int, C.c_int]
    lib.mcraw_pool_create.restype = C.c_int
    lib.mcraw_pool_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
    lib.mcraw_pool_destroy.restype = None
    lib.mcraw_pool_destroy.argtypes = [C.c_void_p]
    lib.mcraw_pool_last_error.restype = C.c_char_p
    lib.mcraw_pool_last_error.argtypes = []
    for name in ("mcraw_pool_size",):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [C.c_void_p]
    for name in ("mcraw_pool_device", "mcraw_pool_numa_cpus"):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [C.c_void_p, C.c_int]
    lib.mcraw_pool_ctx.restype = C.c_void_p
    lib.mcraw_pool_ctx.argtypes = [C.c_void_p, C.c_int]
    lib.mcraw_pool_set_post.restype = C.c_int
    lib.mcraw_pool_set_post.argtypes = [C.c_void_p, C.POINTER(Post)]
    lib.mcraw_pool_host_alloc.restype = C.c_void_p
    lib.mcraw_pool_host_alloc.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    lib.mcraw_pool_decode_batch.restype = C.c_int
    lib.mcraw_pool_decode_batch.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    lib.mcraw_tile_order.restype = C.c_uint32
    lib.mcraw_tile_order.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.mcraw_pool_synchronize.restype = C.c_int
    lib.mcraw_pool_synchronize.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    lib.mcraw_ctx_xcd_runs.restype = C.c_int
    lib.mcraw_ctx_xcd_runs.argtypes = [C.c_void_p]
    lib.mcraw_ctx_side_parts.restype = C.c_int
    lib.mcraw_ctx_side_parts.argtypes = [C.c_void_p]
    lib.mcraw_ctx_host_way.restype = C.c_int
    lib.mcraw_ctx_host_way.argtypes = [C.c_void_p]
    lib.mcraw_pool_decode_batch_device.restype = C.c_int
    lib.mcraw_pool_decode_batch_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    lib.mcraw_pool_decode_batch_async.restype = C.c_int
    lib.mcraw_pool_decode_batch_async.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int, C.POINTER(C.c_void_p)]
    lib.mcraw_pool_ticket_wait.restype = C.c_int
    lib.mcraw_pool_ticket_wait.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    lib.mcraw_encode_bound7.restype = C.c_size_t
    lib.mcraw_encode_bound7.argtypes = [C.c_int, C.c_int]
    lib.mcraw_encode_batch.restype = C.c_int
    lib.mcraw_encode_batch.argtypes = [C.c_void_p, C.POINTER(EncFrame), C.c_int, C.c_int, C.c_void_p,
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    lib.mcraw_ctx_set_float_out.restype = C.c_int
    lib.mcraw_ctx_set_float_out.argtypes = [C.c_void_p, C.POINTER(FloatOut)]
    lib.mcraw_pool_set_float_out.restype = C.c_int
    lib.mcraw_pool_set_float_out.argtypes = [C.c_void_p, C.POINTER(FloatOut)]
    lib.mcraw_demosaic_batch.restype = C.c_int
    lib.mcraw_demosaic_batch.argtypes = [C.c_void_p, C.POINTER(RgbParams), C.POINTER(RgbColor), C.c_int, C.c_void_p, C.c_size_t,
                                         C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mcraw_demosaic_display_batch.restype = C.c_int
    lib.mcraw_demosaic_display_batch.argtypes = [C.c_void_p, C.POINTER(RgbParams), C.POINTER(Display), C.POINTER(RgbColor),
                                                 C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mcraw_demosaic_yuv_batch.restype = C.c_int
    lib.mcraw_demosaic_yuv_batch.argtypes = [C.c_void_p, C.POINTER(RgbParams), C.POINTER(Yuv), C.POINTER(RgbColor), C.c_int,
                                             C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_size_t, C.c_void_p]
    lib.mcraw_shade_batch.restype = C.c_int
    lib.mcraw_shade_batch.argtypes = [C.c_void_p, C.POINTER(Shade), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    lib.mcraw_stats_record_bytes.restype = C.c_size_t
    lib.mcraw_stats_record_bytes.argtypes = [C.c_uint32]
    lib.mcraw_stats_batch.restype = C.c_int
    lib.mcraw_stats_batch.argtypes = [C.c_void_p, C.POINTER(Stats), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mcraw_noise_record_bytes.restype = C.c_size_t
    lib.mcraw_noise_record_bytes.argtypes = []
    lib.mcraw_noise_energy_bin.restype = C.c_uint32
    lib.mcraw_noise_energy_bin.argtypes = [C.c_uint64]
    lib.mcraw_noise_batch.restype = C.c_int
    lib.mcraw_noise_batch.argtypes = [C.c_void_p, C.POINTER(Noise), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mcraw_fixpix_batch.restype = C.c_int
    lib.mcraw_fixpix_batch.argtypes = [C.c_void_p, C.POINTER(FixPix), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    lib.mcraw_highlights_measure_batch.restype = C.c_int
    lib.mcraw_highlights_measure_batch.argtypes = [C.c_void_p, C.POINTER(Highlights), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                                                   C.c_int, C.c_void_p]
    lib.mcraw_highlights_batch.restype = C.c_int
    lib.mcraw_highlights_batch.argtypes = [C.c_void_p, C.POINTER(Highlights), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    lib.mcraw_denoise_batch.restype = C.c_int
    lib.mcraw_denoise_batch.argtypes = [C.c_void_p, C.POINTER(Denoise), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    lib.mcraw_merge_batch.restype = C.c_int
    lib.mcraw_merge_batch.argtypes = [C.c_void_p, C.POINTER(Merge), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    lib.mcraw_align_work_bytes.restype = C.c_size_t
    lib.mcraw_align_work_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32]
    lib.mcraw_align_batch.restype = C.c_int
    lib.mcraw_align_batch.argtypes = [C.c_void_p, C.POINTER(Align), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p]
    lib.mcraw_align_cells_work_bytes.restype = C.c_size_t
    lib.mcraw_align_cells_work_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.mcraw_align_cells_batch.restype = C.c_int
    lib.mcraw_align_cells_batch.argtypes = [C.c_void_p, C.POINTER(AlignCells), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                                            C.c_int, C.c_void_p]
    lib.mcraw_merge_cells_batch.restype = C.c_int
    lib.mcraw_merge_cells_batch.argtypes = [C.c_void_p, C.POINTER(Merge), C.POINTER(Cells), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    lib.mcraw_area_work_bytes.restype = C.c_size_t
    lib.mcraw_area_work_bytes.argtypes = [C.POINTER(Area)]
    lib.mcraw_resample_work_bytes.restype = C.c_size_t
    lib.mcraw_resample_work_bytes.argtypes = [C.POINTER(Resample)]
    lib.mcraw_demosaic_resample_batch.restype = C.c_int
    lib.mcraw_demosaic_resample_batch.argtypes = [C.c_void_p, C.POINTER(RgbParams), C.POINTER(Resample), C.POINTER(Display),
                                                  C.POINTER(Yuv), C.POINTER(RgbColor), C.c_int, C.c_void_p, C.c_size_t, C.c_size_t,
                                                  C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mcraw_demosaic_warp_batch.restype = C.c_int
    lib.mcraw_demosaic_warp_batch.argtypes = [C.c_void_p, C.POINTER(RgbParams), C.POINTER(Warp), C.POINTER(Display), C.POINTER(Yuv),
                                              C.POINTER(RgbColor), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_size_t,
                                              C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mcraw_mesh_nodes.restype = C.c_size_t
    lib.mcraw_mesh_nodes.argtypes = [C.POINTER(Mesh)]
    lib.mcraw_mesh_check.restype = C.c_int
    lib.mcraw_mesh_check.argtypes = [C.POINTER(Mesh), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int]
    lib.mcraw_demosaic_mesh_batch.restype = C.c_int
    lib.mcraw_demosaic_mesh_batch.argtypes = [C.c_void_p, C.POINTER(RgbParams), C.POINTER(Mesh), C.POINTER(Display), C.POINTER(Yuv),
                                              C.POINTER(RgbColor), C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                              C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mcraw_demosaic_area_batch.restype = C.c_int
    lib.mcraw_demosaic_area_batch.argtypes = [C.c_void_p, C.POINTER(RgbParams), C.POINTER(Area), C.POINTER(Display), C.POINTER(Yuv),
                                              C.POINTER(RgbColor), C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.mcraw_encode7.restype = C.c_size_t
    lib.mcraw_encode7.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    _lib = lib
    return lib


def _kernel_id(name):
    for table in (KERNELS, ENC_KERNELS, RGB_KERNELS):
        if name in table:
            return table[name]
    raise KeyError(name)


def encode_bound7(w, h):
    """Exact worst-case size in bytes of a type-7 frame of w x h samples (host only, no GPU needed)."""
    return int(load().mcraw_encode_bound7(int(w), int(h)))


class Pool:
    """Owner of one ``mcraw_pool``: several GPUs of one node, frame i -> member i mod size."""

    def __init__(self, devices=None):
        self._lib = load()
        h = C.c_void_p()
        devices = list(devices or [])
        arr = (C.c_int * max(len(devices), 1))(*devices)
        rc = self._lib.mcraw_pool_create(arr if devices else None, len(devices), C.byref(h))
        if rc != 0 or not h.value:
            raise McrawError("mcraw_pool_create failed (%d): %s" % (rc, self._lib.mcraw_pool_last_error().decode()))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mcraw_pool_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return self._lib.mcraw_pool_size(self._h)

    def devices(self):
        return [self._lib.mcraw_pool_device(self._h, m) for m in range(self.size)]

    def numa_cpus(self):
        return [self._lib.mcraw_pool_numa_cpus(self._h, m) for m in range(self.size)]

    def host_alloc(self, member, nbytes):
        return self._lib.mcraw_pool_host_alloc(self._h, member, nbytes)

    def set_post(self, black=None, pack12=False, bits=None):
        nb = int(bits) if bits else (12 if pack12 else 16)
        if black is None and nb == 16:
            rc = self._lib.mcraw_pool_set_post(self._h, None)
        else:
            p = Post()
            if black is not None:
                p.flags |= POST_BLACK
                for i in range(4):
                    p.black[i] = int(black[i])
            p.flags |= _PACK_FLAG[nb]
            rc = self._lib.mcraw_pool_set_post(self._h, C.byref(p))
        if rc != 0:  # (a rejected stage must not decode plain mosaics silently)
            raise McrawError("mcraw_pool_set_post failed (%d): %s" % (rc, self._lib.mcraw_last_error().decode()))

    def set_float_out(self, dtype, white, layout="planes", black=(0, 0, 0, 0), clip=False, plane=None):
        """Normalised float output on every member (Context.set_float_out); set_post() goes back to uint16 mosaics."""
        f = float_out(dtype, white, layout, black, clip, plane)
        rc = self._lib.mcraw_pool_set_float_out(self._h, C.byref(f))
        if rc != 0:
            raise McrawError("mcraw_pool_set_float_out failed (%d): %s" % (rc, self._lib.mcraw_pool_last_error().decode()))

    def decode_batch_device(self, frames, want_status=True):
        """frames: ctypes array from Context.make_frames whose in / out pointers live in the HBM of the GPU that decodes
        the frame: frame i on ``devices()[i % size]``.  Returns (written, status); with want_status=False the members
        only queue their shares (synchronize() waits and returns the statuses)."""
        n = len(frames)
        written = (C.c_size_t * max(n, 1))()
        status = (C.c_int32 * max(n, 1))()
        rc = self._lib.mcraw_pool_decode_batch_device(self._h, frames, n, written if want_status else None, status if want_status else None)
        if rc != 0:
            raise McrawError("mcraw_pool_decode_batch_device failed (%d): %s" % (rc, self._lib.mcraw_pool_last_error().decode()))
        return (list(written)[:n], list(status)[:n]) if want_status else None

    def synchronize(self, n):
        """Waits for everything queued; returns the statuses of the calling thread's last queued resident batch.
        ``self.errors``: OR of the statuses of all frames of all queued batches whose outcome became known with this call."""
        status = (C.c_int32 * max(n, 1))()
        rc = self._lib.mcraw_pool_synchronize(self._h, status, n)
        if rc < 0:
            raise McrawError("mcraw_pool_synchronize failed (%d): %s" % (rc, self._lib.mcraw_pool_last_error().decode()))
        self.errors = rc
        return list(status)[:n]

    def decode_batch(self, frames):
        """frames: ctypes array from Context.make_frames (host pointers).  Returns (written, status)."""
        n = len(frames)
        written = (C.c_size_t * max(n, 1))()
        status = (C.c_int32 * max(n, 1))()
        rc = self._lib.mcraw_pool_decode_batch(self._h, frames, n, written, status)
        if rc != 0:
            raise McrawError("mcraw_pool_decode_batch failed (%d): %s" % (rc, self._lib.mcraw_pool_last_error().decode()))
        return list(written)[:n], list(status)[:n]

    def decode_batch_async(self, frames):
        t = C.c_void_p()
        rc = self._lib.mcraw_pool_decode_batch_async(self._h, frames, len(frames), C.byref(t))
        if rc != 0:
            raise McrawError("mcraw_pool_decode_batch_async failed (%d): %s" % (rc, self._lib.mcraw_pool_last_error().decode()))
        return (t, len(frames))

    def wait(self, ticket):
        t, n = ticket
        written = (C.c_size_t * max(n, 1))()
        status = (C.c_int32 * max(n, 1))()
        rc = self._lib.mcraw_pool_ticket_wait(t, written, status)
        if rc != 0:
            raise McrawError("mcraw_pool_ticket_wait failed (%d): %s" % (rc, self._lib.mcraw_pool_last_error().decode()))
        return list(written)[:n], list(status)[:n]


class Context:
    """Owner of one ``mcraw_ctx`` (one HIP device)."""

    def __init__(self, device=-1):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.mcraw_ctx_create(device, C.byref(h))
        if rc != 0 or not h.value:
            raise McrawError("mcraw_ctx_create failed (%d): %s" % (rc, self._lib.mcraw_last_error().decode()))
        self._h = h
        self._device = device
        self._stage = None  # the stage last set: None (plain mosaic), ("post", kwargs) or ("float", kwargs)

    def xcd_runs(self):
        """The XCD mapping the library chose for the current large resident batches (mcraw_ctx_xcd_runs)."""
        return self._lib.mcraw_ctx_xcd_runs(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mcraw_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def make_frames(descs):
        """descs: iterable of (in_ptr, len, width, height, type, out_ptr, out_capacity)."""
        descs = list(descs)
        arr = (Frame * len(descs))()
        for i, (inp, ln, w, h, t, outp, cap) in enumerate(descs):
            arr[i] = Frame(inp, ln, w, h, t, 0, outp, cap)
        return arr

    def decode_batch(self, frames, mem=MEM_DEVICE, stream=None, want_status=True):
        """frames: ctypes array from make_frames.  Returns (written, status) lists when
        want_status (synchronises), else None (asynchronous on `stream`)."""
        n = len(frames)
        if want_status:
            written = (C.c_size_t * n)()
            status = (C.c_int32 * n)()
            rc = self._lib.mcraw_decode_batch(self._h, frames, n, mem, stream, written, status)
        else:
            rc = self._lib.mcraw_decode_batch(self._h, frames, n, mem, stream, None, None)
        if rc != 0:
            raise McrawError("mcraw_decode_batch failed (%d): %s" % (rc, self._lib.mcraw_last_error().decode()))
        if want_status:
            return list(written), list(status)
        return None

    @staticmethod
    def make_enc_frames(descs):
        """descs: iterable of (in_ptr, width, height, out_ptr, out_capacity[, len_out_ptr])."""
        descs = list(descs)
        arr = (EncFrame * len(descs))()
        for i, d in enumerate(descs):
            inp, w, h, outp, cap = d[:5]
            arr[i] = EncFrame(inp, w, h, outp, cap, d[5] if len(d) > 5 else None)
        return arr

    def encode_batch(self, frames, mem=MEM_DEVICE, stream=None, want_status=True):
        """frames: ctypes array from make_enc_frames.  Returns (written bytes, status) lists when
        want_status (synchronises), else None (asynchronous on `stream`; len_out gives the sizes)."""
        n = len(frames)
        if want_status:
            written = (C.c_size_t * max(n, 1))()
            status = (C.c_int32 * max(n, 1))()
            rc = self._lib.mcraw_encode_batch(self._h, frames, n, mem, stream, written, status)
        else:
            rc = self._lib.mcraw_encode_batch(self._h, frames, n, mem, stream, None, None)
        if rc != 0:
            raise McrawError("mcraw_encode_batch failed (%d): %s" % (rc, self._lib.mcraw_last_error().decode()))
        if want_status:
            return list(written)[:n], list(status)[:n]
        return None

    def decode_batch_async(self, frames):
        """Host-memory batch, queued: returns a ticket for wait()."""
        t = C.c_void_p()
        rc = self._lib.mcraw_decode_batch_async(self._h, frames, len(frames), C.byref(t))
        if rc != 0:
            raise McrawError("mcraw_decode_batch_async failed (%d): %s" % (rc, self._lib.mcraw_last_error().decode()))
        return (t, len(frames))

    def wait(self, ticket):
        """Blocks for that batch; returns (written, status)."""
        t, n = ticket
        written = (C.c_size_t * max(n, 1))()
        status = (C.c_int32 * max(n, 1))()
        rc = self._lib.mcraw_ticket_wait(t, written, status)
        if rc != 0:
            raise McrawError("mcraw_ticket_wait failed (%d): %s" % (rc, self._lib.mcraw_last_error().decode()))
        return list(written)[:n], list(status)[:n]

    def synchronize(self, nframes=0):
        status = (C.c_int32 * max(nframes, 1))()
        rc = self._lib.mcraw_ctx_synchronize(self._h, status if nframes else None, nframes)
        if rc != 0:
            raise McrawError("mcraw_ctx_synchronize failed (%d): %s" % (rc, self._lib.mcraw_last_error().decode()))
        return list(status)[:nframes]

    def side_parts(self):
        """(parts of the bits stream, parts of the refs stream) k7_side was measured to run fastest with, or None."""
        v = int(self._lib.mcraw_ctx_side_parts(self._h))
        return None if v < 0 else (v >> 4, v & 15)

    def host_way(self):
        """How the status words of large host-memory batches come home: 0 fetched, 1 sent behind the kernels, None: still comparing."""
        v = int(self._lib.mcraw_ctx_host_way(self._h))
        return None if v < 0 else v

    def last_serial(self):
        return int(self._lib.mcraw_ctx_last_serial(self._h))

    def batch_status(self, serial, nframes):
        """Statuses of the device-memory batch `serial` that was submitted without a status request (None: not one of the last 64)."""
        status = (C.c_int32 * max(nframes, 1))()
        rc = self._lib.mcraw_ctx_batch_status(self._h, serial, status, nframes)
        if rc < 0:
            raise McrawError("mcraw_ctx_batch_status failed (%d): %s" % (rc, self._lib.mcraw_last_error().decode()))
        return None if rc else list(status)[:nframes]

    def errors(self, reset=True):
        return int(self._lib.mcraw_ctx_errors(self._h, 1 if reset else 0))

    def set_post(self, black=None, pack12=False, bits=None):
        """Fused post-decode stage of the batches to come: black levels (4 values, CFA order
        (row & 1) * 2 + (col & 1)) and/or strip rows of `bits` = 10, 12 or 14 bits per sample (pack12=True: 12);
        no arguments = the plain uint16 mosaic."""
        nb = int(bits) if bits else (12 if pack12 else 16)
        if black is None and nb == 16:
            rc = self._lib.mcraw_ctx_set_post(self._h, None)
        else:
            p = Post()
            if black is not None:
                p.flags |= POST_BLACK
                for i in range(4):
                    p.black[i] = int(black[i])
            p.flags |= _PACK_FLAG[nb]
            rc = self._lib.mcraw_ctx_set_post(self._h, C.byref(p))
        if rc != 0:
            raise McrawError("mcraw_ctx_set_post failed (%d): %s" % (rc, self._lib.mcraw_last_error().decode()))
        self._stage = ("post", dict(black=black, pack12=pack12, bits=bits)) if (black is not None or nb != 16) else None

    def set_float_out(self, dtype, white, layout="planes", black=(0, 0, 0, 0), clip=False, plane=None):
        """Normalised float output for the batches to come, in place of the uint16 mosaic (and of any set_post stage):
        (sample - black[p]) / (white - black[p]) as torch.float32 / float16 / bfloat16 (or "f32" / "f16" / "bf16"),
        clamped to [0, 1] with clip; layout "mosaic" (width x height) or "planes" (4 planes of height/2 x width/2,
        CFA position p to plane[p]; cfa_planes() gives R, G, G, B).  set_post() goes back to the uint16 mosaic."""
        f = float_out(dtype, white, layout, black, clip, plane)
        rc = self._lib.mcraw_ctx_set_float_out(self._h, C.byref(f))
        if rc != 0:
            raise McrawError("mcraw_ctx_set_float_out failed (%d): %s" % (rc, self._lib.mcraw_last_error().decode()))
        self._stage = ("float", dict(dtype=dtype, white=white, layout=layout, black=tuple(black), clip=clip, plane=plane))

    def _restore_stage(self, stage):
        if stage is None:
            self.set_post()
        elif stage[0] == "post":
            self.set_post(**stage[1])
        else:
            self.set_float_out(**stage[1])

    def _torch_device(self, torch):
        if self._device >= 0:
            return torch.device("cuda", self._device)
        env = os.environ.get("MCRAW_DEVICE")
        return torch.device("cuda", int(env)) if env else torch.device("cuda", torch.cuda.current_device())

    def decode_tensor(self, inputs, width, height, type, *, dtype, white, layout="planes", black=(0, 0, 0, 0), clip=False,
                      plane=None, out=None, check=True):
        """Decode frames of one geometry that are resident in HBM straight into a normalised float tensor on the
        context's device: (N, 4, height/2, width/2) for layout "planes", (N, height, width) for "mosaic".

        inputs: uint8 CUDA tensors, or (device pointer, length) pairs.  The batch is enqueued on
        torch.cuda.current_stream(), so torch work queued behind it on that stream sees the result.  check=True
        synchronises and raises McrawError naming the frames that failed; check=False returns at once.  The stage the
        context had before the call is restored afterwards."""
        import torch
        width, height, n = int(width), int(height), len(inputs)
        if layout not in _LAYOUTS:
            raise ValueError("layout must be 'planes' or 'mosaic', not %r" % (layout,))
        if width <= 0 or height <= 0 or (layout == "planes" and (width % 2 or height % 2)):
            raise ValueError("decode_tensor: %dx%d frames (the planes layout needs an even width and height)" % (width, height))
        tdtype = {FLOAT_F32: torch.float32, FLOAT_F16: torch.float16, FLOAT_BF16: torch.bfloat16}[_float_code(dtype)]
        dev = self._torch_device(torch)
        shape = (n, 4, height // 2, width // 2) if layout == "planes" else (n, height, width)
        if out is None:
            out = torch.empty(shape, dtype=tdtype, device=dev)
        elif tuple(out.shape) != shape or out.dtype != tdtype or out.device != dev or not out.is_contiguous():
            raise ValueError("decode_tensor: out must be a contiguous %s tensor of shape %s on %s" % (tdtype, shape, dev))
        frame_bytes = width * height * out.element_size()
        descs = []
        for x in inputs:
            if isinstance(x, torch.Tensor):
                if x.dtype != torch.uint8 or x.device != dev or not x.is_contiguous():
                    raise ValueError("decode_tensor: inputs must be contiguous uint8 tensors on %s" % dev)
                ptr, ln = x.data_ptr(), x.numel()
            else:
                ptr, ln = int(x[0]), int(x[1])
            descs.append((ptr, ln, width, height, int(type), out.data_ptr() + len(descs) * frame_bytes, frame_bytes // 2))
        if n == 0:
            return out
        cur = torch.cuda.current_stream(dev)
        # (torch's default stream is the null stream, which the library reads as "the context's own": such a batch runs on a
        # side stream of this context's that waits for the current stream and is waited for by it -- still no host sync)
        run = cur
        if not cur.cuda_stream:
            if getattr(self, "_side", None) is None:
                self._side = torch.cuda.Stream(dev)
            run = self._side
            run.wait_stream(cur)
        prev = self._stage
        self.set_float_out(dtype, white, layout, black, clip, plane)
        try:
            res = self.decode_batch(self.make_frames(descs), mem=MEM_DEVICE, stream=C.c_void_p(run.cuda_stream), want_status=check)
        finally:
            self._restore_stage(prev)
            if run is not cur:
                cur.wait_stream(run)
        if check:
            bad = [(i, st) for i, st in enumerate(res[1]) if st != 0]
            if bad:
                raise McrawError("decode_tensor: %d of %d frames failed: %s" % (
                    len(bad), n, ", ".join("frame %d status 0x%x" % b for b in bad[:16])))
        return out

    def _run_stream(self, torch, dev):
        """(current stream, stream to run on): torch's default stream is the null stream, which the library reads as "the
        context's own", so work for it runs on a side stream of this context's that waits for the current stream (the
        caller then makes the current stream wait for it: still no host sync)."""
        cur = torch.cuda.current_stream(dev)
        if cur.cuda_stream:
            return cur, cur
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(dev)
        self._side.wait_stream(cur)
        return cur, self._side

    def _mosaic_arg(self, torch, dev, fn, mosaic, dims=(2, 3)):
        """The mosaic argument of method `fn`, checked, as (mos, single, n, h, w): mos is (N, H, W); single: the caller's was
        (H, W)."""
        if not isinstance(mosaic, torch.Tensor) or mosaic.dtype != torch.uint16 or mosaic.device != dev or mosaic.dim() not in dims:
            raise ValueError("%s: mosaic must be a uint16 tensor (N, H, W)%s on %s" % (fn, " or (H, W)" if 2 in dims else "", dev))
        single = mosaic.dim() == 2
        mos = mosaic.unsqueeze(0) if single else mosaic
        n, h, w = (int(v) for v in mos.shape)
        return mos, single, n, h, w

    @staticmethod
    def _out_arg(torch, dev, fn, out, shape, dtype=None, contiguous=False):
        """The `out` argument of method `fn`: a new contiguous tensor of `shape`, or the caller's, checked."""
        dtype = torch.uint16 if dtype is None else dtype
        if out is None:
            return torch.empty(tuple(shape), dtype=dtype, device=dev)
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev \
                or (contiguous and not out.is_contiguous()):
            raise ValueError("%s: out must be a %s%s tensor of shape %s on %s" % (
                fn, "contiguous " if contiguous else "", str(dtype).replace("torch.", ""), tuple(shape), dev))
        return out

    @staticmethod
    def _strided(fn, what, t, h, w):
        """A batch of mosaics (frames, H, W) as the library takes it: (pointer, pitch, frame stride), in elements.  Rows must be
        contiguous; the stride of a dimension of one entry means nothing and is replaced by the packed one."""
        if w > 1 and t.stride(2) != 1:
            raise ValueError("%s: the rows of %s must be contiguous" % (fn, what))
        pitch = int(t.stride(1)) if h > 1 else w
        return C.c_void_p(t.data_ptr()), pitch, (int(t.stride(0)) if int(t.shape[0]) > 1 else pitch * h)

    def _noise_table(self, torch, dev, fn, lut, n):
        """The noise table of denoise / merge (a CUDA uint16 tensor, or a host array from noise_lut, uploaded on the current
        stream) as (tensor, nluts, L)."""
        import numpy as np
        if isinstance(lut, np.ndarray):
            if lut.dtype != np.uint16:
                raise ValueError("%s: a lut array must be uint16 (noise_lut makes one)" % fn)
            lut = torch.from_numpy(np.ascontiguousarray(lut).view(np.int16)).to(dev).view(torch.uint16)
        if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint16 or lut.device != dev or lut.dim() not in (2, 3) \
                or not lut.is_contiguous():
            raise ValueError("%s: lut must be a contiguous uint16 tensor (4, L) or (N, 4, L) on %s" % (fn, dev))
        nluts, L = (int(lut.shape[0]) if lut.dim() == 3 else 1), int(lut.shape[-1])
        if int(lut.shape[-2]) != 4 or L not in (64, 128, 256, 512, 1024) or (lut.dim() == 3 and nluts != n):
            raise ValueError("%s: lut must hold four planes of 64 .. 1024 (a power of two) entries, for all frames or for "
                             "each of the %d" % (fn, n))
        return lut, nluts, L

    def _call(self, torch, dev, symbol, tensors, *args):
        """One call of the library's `symbol`(context, *args, stream) on _run_stream's stream.  When that is the side stream, the
        tensors that take part (None: skipped) are recorded on it and the current stream waits for it.  A non-zero return raises
        McrawError."""
        cur, run = self._run_stream(torch, dev)
        try:
            rc = getattr(self._lib, symbol)(self._h, *args, C.c_void_p(run.cuda_stream))
        finally:
            if run is not cur:
                for t in tensors:
                    if t is not None:
                        t.record_stream(run)
                cur.wait_stream(run)
        if rc != 0:
            raise McrawError("%s failed (%d): %s" % (symbol, rc, self._lib.mcraw_last_error().decode()))

    def _shading_tensor(self, torch, dev, shading, n, fn):
        """The device gain map of `shading` (a CUDA uint16 tensor, or a host array from gain_map, uploaded on the current
        stream) as (tensor, maps, gh, gw)."""
        import numpy as np
        if isinstance(shading, np.ndarray):
            if shading.dtype != np.uint16:
                raise ValueError("%s: a shading array must be uint16 (gain_map makes one)" % fn)
            shading = torch.from_numpy(np.ascontiguousarray(shading).view(np.int16)).to(dev).view(torch.uint16)
        if not isinstance(shading, torch.Tensor) or shading.dtype != torch.uint16 or shading.device != dev \
                or shading.dim() not in (3, 4) or not shading.is_contiguous():
            raise ValueError("%s: shading must be a contiguous uint16 tensor (4, gh, gw) or (N, 4, gh, gw) on %s" % (fn, dev))
        maps = int(shading.shape[0]) if shading.dim() == 4 else 1
        if int(shading.shape[-3]) != 4 or maps not in (1, n):
            raise ValueError("%s: shading must hold four planes, for all frames or for each of the %d" % (fn, n))
        return shading, maps, int(shading.shape[-2]), int(shading.shape[-1])

    def shade(self, mosaic, shading, *, black=(0, 0, 0, 0), top=65535, out=None):
        """Apply a lens-shading gain map to uint16 mosaics resident on the context's device (mcraw_shade_batch): what a
        sample holds above its black level is multiplied by the gain that the map gives for its place, bilinearly
        interpolated per CFA position in integers, and the result saturates at `top`; the black level of the output is the
        black level of the input, so everything that takes a mosaic takes the result with the parameters it would take
        anyway.  mosaic: (N, H, W) or (H, W), rows contiguous (rows and frames may be strided), odd sizes are fine.
        shading: a uint16 Q3.12 map (4, gh, gw) for all frames or (N, 4, gh, gw) per frame, gh, gw <= 64, planes by CFA
        position (gain_map / shading_map make one): a CUDA tensor, read when the kernel runs (in stream order), or a host
        array, uploaded on the current stream.  out: None (a new contiguous tensor), a uint16 tensor of the mosaic's
        shape, or the mosaic itself (in place).  Queued on torch.cuda.current_stream(); nothing synchronises."""
        import torch
        dev = self._torch_device(torch)
        mos, single, n, h, w = self._mosaic_arg(torch, dev, "shade", mosaic)
        out = self._out_arg(torch, dev, "shade", out, mosaic.shape)
        if n == 0 or h == 0 or w == 0:
            return out
        src = self._strided("shade", "the mosaic", mos, h, w)
        dst = self._strided("shade", "out", out.unsqueeze(0) if single else out, h, w)
        shading, maps, gh, gw = self._shading_tensor(torch, dev, shading, n, "shade")
        black = list(black)
        if len(black) != 4:
            raise ValueError("black: four levels, by CFA position (row & 1) * 2 + (col & 1)")
        s = Shade()
        s.map_w, s.map_h, s.nmaps, s.top = gw, gh, maps, int(top)
        for i in range(4):
            s.black[i] = int(black[i])
        s.reserved[0] = s.reserved[1] = 0
        s.map = shading.data_ptr()
        self._call(torch, dev, "mcraw_shade_batch", (mos, out, shading), C.byref(s), *src, w, h, n, *dst)
        return out

    def fix_pixels(self, mosaic, *, black=(0, 0, 0, 0), abs_thr, rel_thr=0.0, rank=2, hot=True, cold=True, pixels=None,
                   counts=False, out=None):
        """Take the defective pixels out of uint16 mosaics resident on the context's device (mcraw_fixpix_batch).  A pixel
        is compared with the rank-th largest (hot) / smallest (cold) of its eight neighbours of the same colour (distance
        2, reflected at the edges) and replaced when it is beyond it by more than abs_thr + rel_thr * (that neighbour
        above black); the replacement is the mean of the opposite pair that differs least.  The black level of the output
        is that of the input.  mosaic: (N, H, W) or (H, W), rows contiguous (rows and frames may be strided), odd sizes are
        fine.  black, abs_thr: one level or four, by CFA position (row & 1) * 2 + (col & 1), integers 0 .. 65535 (a
        fractional level raises ValueError, also one that defects= forwards from the enclosing call's black=).  rel_thr: a float,
        kept as rint(rel_thr * 256) in 0 .. 65535.  rank: 1 or 2 (2 finds two adjacent defects of one colour).  pixels: a
        static list that is replaced unconditionally, in every frame, from neighbours that are not listed: an (K, 2)
        integer array of (x, y) (packed by pack_pixels and uploaded on the current stream) or a 1-D uint32 / int32 CUDA
        tensor of packed entries y << 16 | x, taken as it is and read when the kernels run (in stream order).  hot=False,
        cold=False leaves the list alone at work.  out: None (a new contiguous tensor) or a uint16 tensor of the mosaic's
        shape that does not overlap it (there is no in-place form).  counts=True also returns an int32 tensor (N, 2, 4)
        ((2, 4) for an (H, W) mosaic): per frame the hot and the cold pixels the detector flagged, by CFA position, listed
        pixels left out.  Queued on torch.cuda.current_stream(); nothing synchronises."""
        import numpy as np
        import torch
        dev = self._torch_device(torch)
        mos, single, n, h, w = self._mosaic_arg(torch, dev, "fix_pixels", mosaic)
        four = lambda v: [v] * 4 if not hasattr(v, "__len__") else list(v)
        black, abs_thr = four(black), four(abs_thr)
        if len(black) != 4 or len(abs_thr) != 4 or any(v != int(v) or v < 0 or v > 65535 for v in black + abs_thr):
            raise ValueError("fix_pixels: black and abs_thr are one level or four, by CFA position (row & 1) * 2 + (col & 1), "
                             "each an integer 0 .. 65535 (the stage works on integers: a fractional level is not rounded for you)")
        black, abs_thr = [int(v) for v in black], [int(v) for v in abs_thr]
        rel = float(rel_thr)
        if not np.isfinite(rel) or np.rint(rel * 256.0) < 0 or np.rint(rel * 256.0) > 65535:
            raise ValueError("fix_pixels: rel_thr * 256 must round into 0 .. 65535, not %r" % (rel_thr,))
        if rank not in (1, 2):
            raise ValueError("fix_pixels: rank must be 1 or 2, not %r" % (rank,))
        out = self._out_arg(torch, dev, "fix_pixels", out, mosaic.shape)
        cnt = torch.empty((n, 2, 4), dtype=torch.int32, device=dev) if counts else None  # (the call initialises the records)
        res = (out, cnt[0] if single else cnt) if counts else out
        if n == 0 or h == 0 or w == 0:
            if counts:
                cnt.zero_()
            return res
        src = self._strided("fix_pixels", "the mosaic", mos, h, w)
        dst = self._strided("fix_pixels", "out", out.unsqueeze(0) if single else out, h, w)
        lst = None
        if pixels is not None:
            if isinstance(pixels, torch.Tensor):
                if pixels.device != dev or pixels.dim() != 1 or pixels.dtype not in (torch.uint32, torch.int32) or not pixels.is_contiguous():
                    raise ValueError("fix_pixels: a pixels tensor must be a contiguous 1-D uint32 tensor of y << 16 | x on %s" % dev)
                lst = pixels
            else:
                lst = torch.from_numpy(pack_pixels(pixels).view(np.int32)).to(dev)
            if int(lst.numel()) > FIXPIX_MAX_LIST:
                raise ValueError("fix_pixels: more than %d listed pixels" % FIXPIX_MAX_LIST)
        s = FixPix()
        s.flags = (FIXPIX_HOT if hot else 0) | (FIXPIX_COLD if cold else 0)
        s.rank, s.rel_thr = int(rank), int(np.rint(rel * 256.0))
        s.nlist = int(lst.numel()) if lst is not None else 0
        for i in range(4):
            s.black[i], s.abs_thr[i] = black[i], abs_thr[i]
        s.list = lst.data_ptr() if s.nlist else None
        s.counts = cnt.data_ptr() if counts else None
        s.reserved[0] = s.reserved[1] = 0
        self._call(torch, dev, "mcraw_fixpix_batch", (mos, out, lst, cnt), C.byref(s), *src, w, h, n, *dst)
        return res

    def _fix_defects(self, mos, defects, black, fn):
        """defects= of the demosaic / decode methods: fix_pixels() with these keyword arguments (black: the call's own
        unless given) into a scratch tensor of the caching allocator."""
        if not isinstance(defects, dict) or "counts" in defects or "out" in defects:
            raise ValueError("%s: defects must be a dict of fix_pixels' keyword arguments (without counts and out)" % fn)
        return self.fix_pixels(mos, **{"black": black, **defects})

    def highlight_chroma(self, mosaic, *, sat, black=(0, 0, 0, 0), gain, cfa="rggb", lo=None, scope="frame", into=None):
        """Measure the colour that highlights() keeps when it rebuilds clipped samples (mcraw_highlights_measure_batch): per
        CFA position the sum and the count of v - ref over the pixels with lo <= sample < sat whose eight neighbours are all
        below their sat, where v is the white-balanced sample and ref the mean of the neighbours' other colours.  mosaic:
        (N, H, W) or (H, W), H, W >= 2, rows contiguous (rows and frames may be strided).  sat, black: one level or four, by CFA
        position (row & 1) * 2 + (col & 1).  gain: (r, g, b) as the demosaic takes them (highlight_gains makes the Q4.12 integers),
        or four Q4.12 integers by CFA position.  lo=None: black + (sat - black) // 2.  scope "frame": one record per frame;
        "batch": one for all frames.  into: a HighlightChroma (or its raw int64 tensor (R, 8), R as scope says) whose records
        are added to instead of started anew: one record over a clip, against flicker.  Returns a HighlightChroma.  Queued on
        torch.cuda.current_stream(); nothing synchronises."""
        import torch
        fn = "highlight_chroma"
        dev = self._torch_device(torch)
        mos, single, n, h, w = self._mosaic_arg(torch, dev, fn, mosaic)
        if scope not in ("frame", "batch"):
            raise ValueError("%s: scope must be 'frame' or 'batch', not %r" % (fn, scope))
        s = _hl_struct(fn, sat, black, gain, cfa, lo, 65535, "rebuild")
        if h < 2 or w < 2:
            raise ValueError("%s: frames must be at least 2 x 2" % fn)
        nrec = 1 if scope == "batch" else n
        raw = into.raw if isinstance(into, HighlightChroma) else into
        if raw is None:
            raw = torch.zeros((nrec, 8), dtype=torch.int64, device=dev)  # (the call initialises them; an empty batch leaves zeros)
        elif not isinstance(raw, torch.Tensor) or raw.dtype != torch.int64 or raw.device != dev or tuple(raw.shape) != (nrec, 8) \
                or not raw.is_contiguous():
            raise ValueError("%s: into must hold a contiguous int64 tensor %r on %s" % (fn, (nrec, 8), dev))
        res = into if isinstance(into, HighlightChroma) else HighlightChroma(raw)
        if n == 0:
            return res
        s.flags = HL_ACCUMULATE if into is not None else 0
        s.rec, s.nrec = raw.data_ptr(), nrec
        src = self._strided(fn, "the mosaic", mos, h, w)
        self._call(torch, dev, "mcraw_highlights_measure_batch", (mos, raw), C.byref(s), *src, w, h, n)
        return res

    def highlights(self, mosaic, *, sat, black=(0, 0, 0, 0), gain, cfa="rggb", mode="rebuild", chroma="frame", lo=None, top=65535,
                   out=None):
        """Take the magenta out of clipped highlights of uint16 mosaics resident on the context's device (mcraw_highlights_batch),
        in front of shading= and the demosaic.  A sample >= sat is clipped.  mode "clip": every CFA position is cut at the
        level where the lowest white-balanced clip level lies, so a blown region becomes exactly neutral; no sample is raised.
        mode "rebuild": a clipped sample becomes what its eight neighbours' other colours say, ref + chroma in white-balanced
        units taken back to the sample's scale, where that is above the sample (and at most `top`); unclipped samples are
        copied bit for bit and no sample is lowered.  The result is a mosaic of the same black level whose samples may exceed
        sat; leave the demosaic's white= as it was, and rebuilt samples lie above 1.0 in front of the matrix.  sat, black, gain,
        cfa, lo: as highlight_chroma().  chroma: "frame" or "batch" (highlight_chroma() with that scope runs first, back to back
        on the same stream), None (no colour: the neighbours' mean as it is) or records that highlight_chroma() returned, one
        or N.  out: None (a new contiguous tensor) or a uint16 tensor of the mosaic's shape that does not overlap it (there is
        no in-place form).  Queued on torch.cuda.current_stream(); nothing synchronises."""
        import torch
        fn = "highlights"
        dev = self._torch_device(torch)
        mos, single, n, h, w = self._mosaic_arg(torch, dev, fn, mosaic)
        s = _hl_struct(fn, sat, black, gain, cfa, lo, top, mode)
        raw = None
        if s.mode == HL_REBUILD and chroma is not None:
            if isinstance(chroma, str):
                if chroma not in ("frame", "batch"):
                    raise ValueError("%s: chroma must be 'frame', 'batch', None or highlight_chroma()'s records, not %r" % (fn, chroma))
            else:
                raw = chroma.raw if isinstance(chroma, HighlightChroma) else chroma
                if not isinstance(raw, torch.Tensor) or raw.dtype != torch.int64 or raw.device != dev or raw.dim() != 2 \
                        or int(raw.shape[1]) != 8 or int(raw.shape[0]) not in (1, n) or not raw.is_contiguous():
                    raise ValueError("%s: chroma records must be a contiguous int64 tensor (1, 8) or (%d, 8) on %s" % (fn, n, dev))
        out = self._out_arg(torch, dev, fn, out, mosaic.shape)
        if n == 0 or h == 0 or w == 0:
            return out
        if h < 2 or w < 2:
            raise ValueError("%s: frames must be at least 2 x 2" % fn)
        if s.mode == HL_REBUILD and isinstance(chroma, str):
            raw = self.highlight_chroma(mos, sat=list(s.sat), black=list(s.black), gain=list(s.gain), cfa=cfa, lo=list(s.lo), scope=chroma).raw
        if raw is not None:
            s.rec, s.nrec = raw.data_ptr(), int(raw.shape[0])
        src = self._strided(fn, "the mosaic", mos, h, w)
        dst = self._strided(fn, "out", out.unsqueeze(0) if single else out, h, w)
        self._call(torch, dev, "mcraw_highlights_batch", (mos, out, raw), C.byref(s), *src, w, h, n, *dst)
        return out

    def _highlights_stage(self, mos, highlights, fn, white, black, cfa, gain):
        """highlights= of the demosaic / decode methods: highlights() with these keyword arguments (_hl_kwargs fills in the
        method's own) into a scratch tensor of the caching allocator."""
        return self.highlights(mos, **_hl_kwargs(fn, highlights, white, black, cfa, gain))

    def denoise(self, mosaic, lut, shift, radius=2, amount=1.0, out=None):
        """Noise-adaptive smoothing of uint16 mosaics resident on the context's device (mcraw_denoise_batch): every pixel
        becomes the weighted mean of itself and its 8 (radius 1) or 24 (radius 2) neighbours of the same colour (distances
        2 and 4, reflected at the edges); a neighbour's weight is 1 - (difference / cut-off)^2, 0 beyond the cut-off, and
        the cut-off at the pixel's level and CFA position is what the table says (noise_lut makes one from a noise
        profile).  The black level of the output is that of the input.  mosaic: (N, H, W) or (H, W), rows contiguous (rows
        and frames may be strided), odd sizes are fine.  lut: uint16 (4, L) for all frames or (N, 4, L) per frame, L a
        power of two in 64 .. 1024, planes by CFA position (row & 1) * 2 + (col & 1): a CUDA tensor, read when the kernel
        runs (in stream order), or a host array, uploaded on the current stream.  shift: 0 .. 15, a pixel of value c uses
        entry min(c >> shift, L - 1).  amount: how much of the correction is applied, a float kept as rint(amount * 256) in
        1 .. 256.  out: None (a new contiguous tensor) or a uint16 tensor of the mosaic's shape that does not overlap it
        (there is no in-place form).  Queued on torch.cuda.current_stream(); nothing synchronises."""
        import numpy as np
        import torch
        dev = self._torch_device(torch)
        mos, single, n, h, w = self._mosaic_arg(torch, dev, "denoise", mosaic)
        if radius not in (1, 2):
            raise ValueError("denoise: radius must be 1 or 2, not %r" % (radius,))
        amt = float(amount)
        if not np.isfinite(amt) or np.rint(amt * 256.0) < 1 or np.rint(amt * 256.0) > 256:
            raise ValueError("denoise: amount * 256 must round into 1 .. 256, not %r" % (amount,))
        if shift != int(shift) or not 0 <= int(shift) <= 15:
            raise ValueError("denoise: shift must be an integer 0 .. 15, not %r" % (shift,))
        out = self._out_arg(torch, dev, "denoise", out, mosaic.shape)
        lut, nluts, L = self._noise_table(torch, dev, "denoise", lut, n)
        if n == 0 or h == 0 or w == 0:
            return out
        src = self._strided("denoise", "the mosaic", mos, h, w)
        dst = self._strided("denoise", "out", out.unsqueeze(0) if single else out, h, w)
        s = Denoise()
        s.radius, s.amount, s.lut_log2, s.shift, s.nluts = int(radius), int(np.rint(amt * 256.0)), L.bit_length() - 1, int(shift), nluts
        s.reserved[0] = s.reserved[1] = s.reserved[2] = 0
        s.lut = lut.data_ptr()
        self._call(torch, dev, "mcraw_denoise_batch", (mos, out, lut), C.byref(s), *src, w, h, n, *dst)
        return out

    def merge(self, mosaic, lut, shift, before=2, after=2, first=0, count=None, support=1, amount=1.0, pos=None, out=None, cell=None):
        """Noise-adaptive merge along time of uint16 mosaics resident on the context's device (mcraw_merge_batch): output j is
        the base frame first + j, every pixel the weighted mean of itself and the samples at its (shifted) position in the
        `before` frames in front of the base and the `after` frames behind it (clipped at the ends of the batch; before +
        after <= 15).  A sample's weight is 1 - (D / cut-off)^2, 0 beyond the cut-off: D is the difference to the base pixel
        (support 0) or the larger of an eighth of the summed differences over the 3x3 pixels around it and half the pixel's
        own (support 1); the cut-off is what denoise()'s table says at the base pixel's level and CFA position.  mosaic: (N,
        H, W), rows contiguous (rows and frames may be strided).  lut: uint16 (4, L) for all frames or (N, 4, L) per base
        frame, a CUDA tensor (read in stream order) or a host array (uploaded on the current stream).  count: None means N -
        first.  amount: a float kept as rint(amount * 256) in 1 .. 256.  pos: None, or the frames' global positions (N, 2)
        as (y, x): an int16 CUDA tensor (read in stream order), or a host array of integers in -32768 .. 32767, uploaded on
        the current stream; a member is read at the difference of the positions with the low bit dropped, so that a sample
        keeps its CFA position.  A 4-D pos (N, Cy, Cx, 2) with cell=(cell_h, cell_w) is a position field, what align_cells()
        returns (mcraw_merge_cells_batch): every cell_h x cell_w samples of a frame have a position of their own, (Cy, Cx) =
        cell_grid(H, W, cell), cell_h a multiple of 32 and cell_w of 256; a tensor or a host array as above.  out: None (a new
        contiguous tensor) or a uint16 tensor (count, H, W) that does not overlap the mosaic.  Returns (count, H, W).  Queued on
        torch.cuda.current_stream(); nothing synchronises."""
        import numpy as np
        import torch
        dev = self._torch_device(torch)
        mosaic, _, n, h, w = self._mosaic_arg(torch, dev, "merge", mosaic, dims=(3,))
        if pos is not None and not isinstance(pos, torch.Tensor):
            pos = np.asarray(pos)  # (a nested list is a host array too)
        field = pos is not None and pos.ndim == 4
        if field != (cell is not None):
            raise ValueError("merge: cell=(cell_h, cell_w) goes with a 4-D pos (N, Cy, Cx, 2), and only with one")
        pshape = (n,) + cell_grid(h, w, cell) + (2,) if field else (n, 2)
        for name, v in (("before", before), ("after", after), ("first", first)) + ((("count", count),) if count is not None else ()):
            if isinstance(v, bool) or v != int(v) or int(v) < 0:
                raise ValueError("merge: %s must be a non-negative integer, not %r" % (name, v))
        before, after, first = int(before), int(after), int(first)
        if before + after > 15:
            raise ValueError("merge: before + after must not exceed 15")
        if first > n:
            raise ValueError("merge: first must be 0 .. %d" % n)
        count = n - first if count is None else int(count)
        if first + count > n:
            raise ValueError("merge: first + count must not exceed the %d frames" % n)
        if support not in (0, 1):
            raise ValueError("merge: support must be 0 or 1, not %r" % (support,))
        amt = float(amount)
        if not np.isfinite(amt) or np.rint(amt * 256.0) < 1 or np.rint(amt * 256.0) > 256:
            raise ValueError("merge: amount * 256 must round into 1 .. 256, not %r" % (amount,))
        if shift != int(shift) or not 0 <= int(shift) <= 15:
            raise ValueError("merge: shift must be an integer 0 .. 15, not %r" % (shift,))
        out = self._out_arg(torch, dev, "merge", out, (count, h, w))
        lut, nluts, L = self._noise_table(torch, dev, "merge", lut, n)
        if pos is not None:
            if isinstance(pos, torch.Tensor):
                if pos.dtype != torch.int16 or pos.device != dev or tuple(pos.shape) != pshape or not pos.is_contiguous():
                    raise ValueError("merge: a pos tensor must be a contiguous int16 tensor %r on %s" % (pshape, dev))
            else:
                a = np.asarray(pos)
                if a.shape != pshape or a.dtype.kind not in "iu" or (a.size and (a.min() < -32768 or a.max() > 32767)):
                    raise ValueError("merge: pos must be %r integers (y, x) in -32768 .. 32767" % (pshape,))
                pos = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int16)).to(dev)
        if n == 0 or count == 0 or h == 0 or w == 0:
            return out
        src = self._strided("merge", "the mosaic", mosaic, h, w)
        dst = self._strided("merge", "out", out, h, w)  # (its frame stride counts for more than one OUTPUT)
        s = Merge()
        s.before, s.after, s.first, s.count, s.support = before, after, first, count, int(support)
        s.amount, s.lut_log2, s.shift, s.nluts, s.reserved = int(np.rint(amt * 256.0)), L.bit_length() - 1, int(shift), nluts, 0
        s.lut = lut.data_ptr()
        if field:
            g = Cells()
            g.cell_h, g.cell_w, g.cells_y, g.cells_x, g.reserved, g.pos = int(cell[0]), int(cell[1]), pshape[1], pshape[2], 0, pos.data_ptr()
            s.pos = None
            self._call(torch, dev, "mcraw_merge_cells_batch", (mosaic, out, lut, pos), C.byref(s), C.byref(g), *src, w, h, n, *dst)
            return out
        s.pos = pos.data_ptr() if pos is not None else None
        self._call(torch, dev, "mcraw_merge_batch", (mosaic, out, lut, pos), C.byref(s), *src, w, h, n, *dst)
        return out

    def stack(self, mosaic, lut, shift, ref=0, **kw):
        """The burst form of merge(): all N <= 16 frames of mosaic (N, H, W) merged onto frame `ref`.  The keyword arguments
        are merge()'s without before, after, first and count (pos= and cell= pass through: a field from align_cells(ref=ref)
        stacks along local motion); out, if given, is (H, W).  Returns (H, W)."""
        import torch
        if not isinstance(mosaic, torch.Tensor) or mosaic.dim() != 3 or not 1 <= int(mosaic.shape[0]) <= 16:
            raise ValueError("stack: mosaic must be a uint16 tensor (N, H, W) of 1 .. 16 frames")
        n = int(mosaic.shape[0])
        if isinstance(ref, bool) or ref != int(ref) or not 0 <= int(ref) < n:
            raise ValueError("stack: ref must be 0 .. %d, not %r" % (n - 1, ref))
        if any(k in kw for k in ("before", "after", "first", "count")):
            raise ValueError("stack: before, after, first and count are merge()'s; the window is the whole burst")
        out = kw.pop("out", None)
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dim() != 2:
                raise ValueError("stack: out must be a uint16 tensor (H, W)")
            out = out.unsqueeze(0)
        ref = int(ref)
        return self.merge(mosaic, lut, shift, before=ref, after=n - 1 - ref, first=ref, count=1, out=out, **kw)[0]

    def align(self, mosaic, *, black=(0, 0, 0, 0), levels=4, radius=4, ref=None, sad=False):
        """One global shift per frame of uint16 mosaics resident on the context's device (mcraw_align_batch): a coarse-to-fine
        search of the smallest sum of absolute differences between grey planes of half the mosaics' size (the mean of a quad's
        four samples above black), `levels` pyramid levels (1 .. 6) with a search radius of `radius` (1 .. 8) pixels of the
        coarsest, so shifts up to about radius * 2 ** levels samples between the frames of a pair are found.  mosaic: (N, H,
        W), rows contiguous (rows and frames may be strided), odd sizes are fine.  black: one level or four, by CFA position
        (row & 1) * 2 + (col & 1), integers 0 .. 65535.  ref=None: a chain, every frame against the one before it, the shifts
        summed from frame 0 on (a clip); ref=r: every frame against frame r (a burst for stack(ref=r)).  Returns the frames'
        positions, a contiguous int16 tensor (N, 2) as (y, x), clamped to -32768 .. 32767: what merge(pos=) and stack(pos=)
        take, so ctx.merge(m, lut, shift, pos=ctx.align(m, black=...)) is the whole recipe.  sad=True also returns an int64
        tensor (N,): the winning sum of absolute differences of the frame's pair over the align_window(H, W, levels, radius)
        pixels of the grey plane, 0 for the frame without a pair; a scene cut shows as a jump.  Frames too small for the
        levels and the radius raise ValueError.  The scratch is a tensor of torch's caching allocator.  Queued on
        torch.cuda.current_stream(); nothing synchronises."""
        import torch
        dev = self._torch_device(torch)
        mosaic, _, n, h, w = self._mosaic_arg(torch, dev, "align", mosaic, dims=(3,))
        black = [black] * 4 if not hasattr(black, "__len__") else list(black)
        if len(black) != 4 or any(v != int(v) or v < 0 or v > 65535 for v in black):
            raise ValueError("align: black is one level or four, by CFA position (row & 1) * 2 + (col & 1), each an integer 0 .. 65535")
        if ref is not None and (isinstance(ref, bool) or ref != int(ref) or not 0 <= int(ref) < max(n, 1)):
            raise ValueError("align: ref must be None (a chain) or 0 .. %d, not %r" % (n - 1, ref))
        align_window(max(h, 1), max(w, 1), levels, radius)
        pos = torch.empty((n, 2), dtype=torch.int16, device=dev)
        sums = torch.empty((n,), dtype=torch.int64, device=dev) if sad else None
        if n == 0:
            return (pos, sums) if sad else pos
        src = self._strided("align", "the mosaic", mosaic, h, w)
        need = int(self._lib.mcraw_align_work_bytes(w, h, n, int(levels), int(radius)))
        work = torch.empty((need,), dtype=torch.uint8, device=dev)
        a = Align()
        a.levels, a.radius, a.ref, a.reserved = int(levels), int(radius), (-1 if ref is None else int(ref)), 0
        for i in range(4):
            a.black[i] = int(black[i])
        a.pos, a.sad, a.work, a.work_bytes = pos.data_ptr(), (sums.data_ptr() if sad else None), work.data_ptr(), need
        self._call(torch, dev, "mcraw_align_batch", (mosaic, pos, sums, work), C.byref(a), *src, w, h, n)
        return (pos, sums) if sad else pos

    def align_cells(self, mosaic, *, pos=None, black=(0, 0, 0, 0), cell=(64, 256), levels=3, radius=2, ref=None, sad=False):
        """A field of local shifts of uint16 mosaics resident on the context's device (mcraw_align_cells_batch): align()'s grey
        pyramid and coarse-to-fine search, with the sums kept per cell of cell = (cell_h, cell_w) samples (cell_h a multiple of
        32, cell_w of 256) instead of per frame, so roll, rolling-shutter wobble and parallax are followed where one shift per
        frame leaves them to the merge's weights.  mosaic: (N, H, W), rows contiguous (rows and frames may be strided), any
        size.  pos: None, or the frames' global positions (N, 2) as align() returns them (an int16 CUDA tensor read in stream
        order, or a host array of integers): the centre of every cell's search, so the field needs to find only what the parts
        of a frame do against the whole.  levels 1 .. 3, radius 1 .. 4 pixels of the coarsest level about that centre.  black,
        ref: align()'s.  Returns the field, a contiguous int16 tensor (N, Cy, Cx, 2) as (y, x) with (Cy, Cx) = cell_grid(H, W,
        cell), clamped to -32768 .. 32767: what merge(pos=, cell=) takes.  sad=True also returns an int64 tensor (N, Cy, Cx):
        the winning sum of absolute differences of each cell's level-0 pixels, 0 for the frame without a pair.  The scratch is
        a tensor of torch's caching allocator.  Queued on torch.cuda.current_stream(); nothing synchronises."""
        import numpy as np
        import torch
        dev = self._torch_device(torch)
        mosaic, _, n, h, w = self._mosaic_arg(torch, dev, "align_cells", mosaic, dims=(3,))
        black = [black] * 4 if not hasattr(black, "__len__") else list(black)
        if len(black) != 4 or any(v != int(v) or v < 0 or v > 65535 for v in black):
            raise ValueError("align_cells: black is one level or four, by CFA position (row & 1) * 2 + (col & 1), each an integer 0 .. 65535")
        if ref is not None and (isinstance(ref, bool) or ref != int(ref) or not 0 <= int(ref) < max(n, 1)):
            raise ValueError("align_cells: ref must be None (a chain) or 0 .. %d, not %r" % (n - 1, ref))
        for name, v, hi in (("levels", levels, 3), ("radius", radius, 4)):
            if isinstance(v, bool) or v != int(v) or not 1 <= int(v) <= hi:
                raise ValueError("align_cells: %s must be an integer 1 .. %d, not %r" % (name, hi, v))
        if h == 0 or w == 0:
            raise ValueError("align_cells: empty frames have no positions")
        cy, cx = cell_grid(h, w, cell)
        if pos is not None:
            if isinstance(pos, torch.Tensor):
                if pos.dtype != torch.int16 or pos.device != dev or tuple(pos.shape) != (n, 2) or not pos.is_contiguous():
                    raise ValueError("align_cells: a pos tensor must be a contiguous int16 tensor (%d, 2) on %s" % (n, dev))
            else:
                g = np.asarray(pos)
                if g.shape != (n, 2) or g.dtype.kind not in "iu" or (g.size and (g.min() < -32768 or g.max() > 32767)):
                    raise ValueError("align_cells: pos must be (%d, 2) integers (y, x) in -32768 .. 32767" % n)
                pos = torch.from_numpy(np.ascontiguousarray(g, dtype=np.int16)).to(dev)
        field = torch.empty((n, cy, cx, 2), dtype=torch.int16, device=dev)
        sums = torch.empty((n, cy, cx), dtype=torch.int64, device=dev) if sad else None
        if n == 0:
            return (field, sums) if sad else field
        src = self._strided("align_cells", "the mosaic", mosaic, h, w)
        need = int(self._lib.mcraw_align_cells_work_bytes(w, h, n, int(levels), int(radius), int(cell[0]), int(cell[1])))
        work = torch.empty((need,), dtype=torch.uint8, device=dev)
        a = AlignCells()
        a.levels, a.radius, a.ref, a.reserved = int(levels), int(radius), (-1 if ref is None else int(ref)), 0
        a.cell_h, a.cell_w = int(cell[0]), int(cell[1])
        for i in range(4):
            a.black[i] = int(black[i])
        a.gpos = pos.data_ptr() if pos is not None else None
        a.pos, a.sad, a.work, a.work_bytes = field.data_ptr(), (sums.data_ptr() if sad else None), work.data_ptr(), need
        self._call(torch, dev, "mcraw_align_cells_batch", (mosaic, field, sums, work, pos), C.byref(a), *src, w, h, n)
        return (field, sums) if sad else field

    def _denoise_stage(self, mos, denoise, fn):
        """denoise= of the demosaic / decode methods: denoise() with these keyword arguments into a scratch tensor of the
        caching allocator."""
        if not isinstance(denoise, dict) or "out" in denoise or "mosaic" in denoise:
            raise ValueError("%s: denoise must be a dict of denoise()'s keyword arguments (without out)" % fn)
        return self.denoise(mos, **denoise)

    def stats(self, mosaic, *, bins=256, shift=None, sat=65535, roi=None, out=None, accumulate=False):
        """Per-frame statistics of uint16 mosaics resident on the context's device (mcraw_stats_batch), by CFA position
        p = (y & 1) * 2 + (x & 1): a histogram of `bins` (64 .. 4096, a power of two) bins with bin = min(v >> shift,
        bins - 1), the sample count, the count of saturated samples (v >= sat), the sum of the unsaturated ones, min and
        max.  mosaic: (N, H, W) or (H, W), rows contiguous (rows and frames may be strided), odd sizes are fine.
        shift=None: the smallest shift with (max(sat) >> shift) < bins, so every unsaturated level has a bin of its own
        scale.  sat: one level or four, by CFA position.  roi=(y0, x0, h, w): the window counted, in frame pixels (a window
        at an odd offset keeps the frame's CFA positions); None: the whole frame.  Returns a FrameStats over a new
        (N, record_bytes) uint8 tensor, or over `out` (a contiguous uint8 tensor of that shape, 8-byte aligned), which the
        call initialises itself.  accumulate=True adds to the records already in `out` instead (a clip over several batches,
        a frame over several windows): counters then wrap modulo 2^32 and FrameStats' int32 views are exact only below 2^31.
        An (H, W) mosaic drops N.  Queued on torch.cuda.current_stream(); nothing synchronises."""
        import torch
        dev = self._torch_device(torch)
        mos, single, n, h, w = self._mosaic_arg(torch, dev, "stats", mosaic)
        bins = int(bins)
        if bins < 64 or bins > 4096 or bins & (bins - 1):
            raise ValueError("stats: bins must be a power of two in 64 .. 4096, not %r" % (bins,))
        sat = [int(sat)] * 4 if not hasattr(sat, "__len__") else [int(v) for v in sat]
        if len(sat) != 4 or any(v < 0 or v > 65535 for v in sat):
            raise ValueError("sat: one level or four, by CFA position (row & 1) * 2 + (col & 1), each 0 .. 65535")
        if shift is None:
            shift = 0
            while (max(sat) >> shift) >= bins:
                shift += 1
        if h == 0 or w == 0:
            raise ValueError("stats: empty frames have no statistics")
        src = self._strided("stats", "the mosaic", mos, h, w)
        y0, x0, rh, rw = (0, 0, h, w) if roi is None else (int(v) for v in roi)
        if min(y0, x0) < 0 or rh < 1 or rw < 1 or y0 + rh > h or x0 + rw > w:
            raise ValueError("stats: roi (y0, x0, h, w) = %r leaves the %d x %d frame" % (roi, h, w))
        rec = 16 * bins + 96
        want = (rec,) if single else (n, rec)
        if out is None and accumulate:
            raise ValueError("stats: accumulate=True needs the records to add to (out=)")
        out = self._out_arg(torch, dev, "stats", out, want, torch.uint8, contiguous=True)
        res = FrameStats(out, bins, shift)
        if n == 0:
            return res
        s = Stats()
        s.bins_log2, s.shift, s.x0, s.y0, s.w, s.h = bins.bit_length() - 1, int(shift), x0, y0, rw, rh
        for i in range(4):
            s.sat[i] = sat[i]
        s.flags, s.reserved = (STATS_ACCUMULATE if accumulate else 0), 0
        self._call(torch, dev, "mcraw_stats_batch", (mos, out), C.byref(s), *src, w, h, n, C.c_void_p(out.data_ptr()), n * rec)
        return res

    def decode_stats(self, inputs, width, height, type, *, bins=256, shift=None, sat=65535, roi=None, out=None,
                     accumulate=False, check=True):
        """Decode frames of one geometry that are resident in HBM and count them (stats()): the plain uint16 mosaics go to a
        scratch tensor of torch's caching allocator, both steps are queued on torch.cuda.current_stream().  inputs: uint8
        CUDA tensors, or (device pointer, length) pairs.  check=True synchronises after the decode and raises McrawError
        naming the frames that failed; check=False returns at once.  The stage the context had before the call is restored
        afterwards.  Returns the FrameStats of the (N, H, W) batch."""
        scratch = self._decode_scratch(inputs, width, height, type, check, "decode_stats")
        return self.stats(scratch, bins=bins, shift=shift, sat=sat, roi=roi, out=out, accumulate=accumulate)

    def noise_stats(self, mosaic, *, shift=None, sat=65535, lo=0, roi=None, out=None, accumulate=False):
        """Per-frame histograms of the local noise energy of uint16 mosaics resident on the context's device
        (mcraw_noise_batch), by CFA position p = (y & 1) * 2 + (x & 1): the window is cut into blocks of 16 x 16 samples, each
        position's 8 x 8 plane of a block gives its sum s and the sum T of its 96 squared second differences, and
        hist[p][min((s >> 6) >> shift, 31)][energy bin of T] counts the block unless one of the plane's samples is >= sat[p] or
        < lo[p] (nrej counts those).  mosaic: (N, H, W) or (H, W), rows contiguous (rows and frames may be strided).
        shift=None: the smallest shift with (max(sat) >> shift) < 32.  sat, lo: one level or four, by CFA position.
        roi=(y0, x0, h, w): the window, y0 and x0 even, h and w at least 16; only its whole blocks count and are read; None:
        the whole frame.  Returns a NoiseStats over a new (N, 65568) uint8 tensor, or over `out` (a contiguous uint8 tensor of
        that shape, 8-byte aligned), which the call initialises itself; accumulate=True adds to the records already in `out`
        (a clip over several batches).  An (H, W) mosaic drops N.  noise_fit turns the result into the (S, O) of noise_lut.
        Queued on torch.cuda.current_stream(); nothing synchronises."""
        import torch
        dev = self._torch_device(torch)
        mos, single, n, h, w = self._mosaic_arg(torch, dev, "noise_stats", mosaic)

        def four(v, name):
            v = [int(v)] * 4 if not hasattr(v, "__len__") else [int(x) for x in v]
            if len(v) != 4 or any(x < 0 or x > 65535 for x in v):
                raise ValueError("%s: one level or four, by CFA position (row & 1) * 2 + (col & 1), each 0 .. 65535" % name)
            return v

        sat, lo = four(sat, "sat"), four(lo, "lo")
        if shift is None:
            shift = 0
            while (max(sat) >> shift) >= NOISE_LEVELS:
                shift += 1
        y0, x0, rh, rw = (0, 0, h, w) if roi is None else (int(v) for v in roi)
        if min(y0, x0) < 0 or (y0 | x0) & 1 or rh < 16 or rw < 16 or y0 + rh > h or x0 + rw > w:
            raise ValueError("noise_stats: the window (y0, x0, h, w) = %r must start on even coordinates, hold 16 x 16 samples "
                             "and lie inside the %d x %d frame" % ((y0, x0, rh, rw), h, w))
        src = self._strided("noise_stats", "the mosaic", mos, h, w)
        want = (NOISE_RECORD_BYTES,) if single else (n, NOISE_RECORD_BYTES)
        if out is None and accumulate:
            raise ValueError("noise_stats: accumulate=True needs the records to add to (out=)")
        out = self._out_arg(torch, dev, "noise_stats", out, want, torch.uint8, contiguous=True)
        res = NoiseStats(out, shift)
        if n == 0:
            return res
        s = Noise()
        s.shift, s.x0, s.y0, s.w, s.h = int(shift), x0, y0, rw, rh
        for i in range(4):
            s.sat[i], s.lo[i] = sat[i], lo[i]
        s.flags, s.reserved = (NOISE_ACCUMULATE if accumulate else 0), 0
        self._call(torch, dev, "mcraw_noise_batch", (mos, out), C.byref(s), *src, w, h, n, C.c_void_p(out.data_ptr()),
                   n * NOISE_RECORD_BYTES)
        return res

    def decode_noise_stats(self, inputs, width, height, type, *, shift=None, sat=65535, lo=0, roi=None, out=None,
                           accumulate=False, check=True):
        """Decode frames of one geometry that are resident in HBM and measure their noise (noise_stats()): the plain uint16
        mosaics go to a scratch tensor of torch's caching allocator, both steps are queued on torch.cuda.current_stream().
        inputs, check and the context's stage: as decode_stats.  Returns the NoiseStats of the (N, H, W) batch."""
        scratch = self._decode_scratch(inputs, width, height, type, check, "decode_noise_stats")
        return self.noise_stats(scratch, shift=shift, sat=sat, lo=lo, roi=roi, out=out, accumulate=accumulate)

    def estimate_noise(self, mosaic, black, white, *, sat=None, roi=None, quantile=0.15):
        """The noise profile (S, O) of uint16 mosaics resident on the context's device, each (4,) float64 by CFA position, pooled
        over the batch: noise_stats() with sat (white unless given) and lo = 1, so that blocks clipped at either end do not
        count, one copy of the records to the host (which synchronises), and noise_fit(black, white, quantile).
        `S, O = ctx.estimate_noise(m, black, white); lut, shift = noise_lut(S, O, black, white)` is the whole recipe for
        denoise() and merge().  It belongs in front of shade() and denoise(): a gain map scales the noise with the position in
        the frame, and a denoised frame has none left to measure.  One static frame of a flat wall is enough -- every level
        bin that is to count needs 200 blocks --, and a scene with texture is fine as long as a sixth of each level's blocks
        are smooth.  A clip whose ISO changes has no one profile: take noise_stats() and noise_fit(pool=False) per frame."""
        white_i = int(white)
        st = self.noise_stats(mosaic, sat=white_i if sat is None else sat, lo=1, roi=roi)
        return noise_fit(st.cpu(), black, white, quantile=quantile)

    def decode_merge(self, inputs, width, height, type, *, lut, shift, check=True, align=None, **merge_kw):
        """Decode frames of one geometry that are resident in HBM and merge them along time (merge()): the plain uint16
        mosaics go to a scratch tensor of torch's caching allocator, both steps are queued on torch.cuda.current_stream().
        inputs: uint8 CUDA tensors, or (device pointer, length) pairs.  check=True synchronises after the decode and raises
        McrawError naming the frames that failed; check=False returns at once.  The stage the context had before the call is
        restored afterwards.  merge_kw: merge()'s keyword arguments.  align: None, or a dict of align()'s keyword arguments
        (without sad): the decoded frames' positions are estimated and handed to the merge as pos.  With "cell": (cell_h,
        cell_w) among them, align() runs without it, align_cells() about its result with the same black and ref (its own levels
        and radius: "cell_levels", default 3, and "cell_radius", default 2), and the merge follows the field.  Returns merge()'s
        (count, H, W)."""
        if align is not None and (not isinstance(align, dict) or "sad" in align or "pos" in merge_kw or "cell" in merge_kw):
            raise ValueError("decode_merge: align must be a dict of align()'s keyword arguments (without sad), and excludes pos and cell")
        scratch = self._decode_scratch(inputs, width, height, type, check, "decode_merge")
        if align is not None:
            align = dict(align)
            cell = align.pop("cell", None)
            ckw = {"levels": align.pop("cell_levels", 3), "radius": align.pop("cell_radius", 2)}
            if cell is None and (ckw["levels"], ckw["radius"]) != (3, 2):
                raise ValueError("decode_merge: cell_levels and cell_radius go with cell")
            merge_kw["pos"] = self.align(scratch, **align)
            if cell is not None:
                ckw.update({k: align[k] for k in ("black", "ref") if k in align})
                merge_kw["pos"] = self.align_cells(scratch, pos=merge_kw["pos"], cell=cell, **ckw)
                merge_kw["cell"] = cell
        return self.merge(scratch, lut, shift, **merge_kw)

    def demosaic(self, mosaic, *, algo="mhc", dtype, white, black=(0, 0, 0, 0), cfa="rggb", gain=None, matrix=None,
                 clip=False, out=None, check=True, shading=None, defects=None, denoise=None, size=None, crop=None, filter=None, affine=None, highlights=None, mesh=None):
        """uint16 mosaics resident on the context's device -> planar linear RGB, (N, 3, H, W) for algo "mhc" (Malvar-He-
        Cutler) or (N, 3, H/2, W/2) for "bin2" (one pixel per 2x2 quad), as torch.float32 / float16 / bfloat16 ("f32" /
        "f16" / "bf16").  mosaic: a CUDA uint16 tensor (N, H, W) or (H, W) whose rows are contiguous (rows and frames may
        be strided); the result of an (H, W) mosaic is (3, Ho, Wo).  black: four levels by CFA position (y & 1) * 2 +
        (x & 1); cfa: the container's sensorArrangment; gain (3,) or (N, 3) and matrix (3, 3) or (N, 3, 3): white balance
        and colour matrix for all frames or per frame (rgb_color gives them); clip: clamp to [0, 1].  Queued on
        torch.cuda.current_stream(); nothing synchronises.  `check` is accepted for symmetry with decode_rgb (the
        arguments are always checked; there are no per-frame statuses).  shading: a lens-shading gain map as shade() takes
        it, applied in front of the demosaic with this call's black levels and top 65535, into a scratch tensor (the
        caller's mosaic is left as it is); None: no such stage.  defects: a dict of fix_pixels()' keyword arguments (black
        defaults to this call's): the defective pixels are taken out first, into a scratch tensor, in front of shading=
        (gains change the differences between neighbours); None: no such stage.  denoise: a dict of denoise()'s
        keyword arguments (lut, shift, radius, amount), applied behind defects= and in front of shading=, into a scratch
        tensor: the noise model holds for the sensor's values, not for the shaded ones; None: no such stage.  highlights: a dict
        of highlights()' keyword arguments (mode, chroma, sat, lo, top, black, gain, cfa), applied behind denoise= and in front
        of shading= (gains move the clip level by position), into a scratch tensor; what the dict leaves out comes from this
        call: sat from white, black, cfa and gain (one gain for the batch: with a gain per frame the dict must bring its own,
        else ValueError).  An unknown key raises ValueError.  white= stays what it is: rebuilt samples lie above it.  None: no
        such stage.
        algo "area" with size=(Ho, Wo) and crop=(y0, x0, h, w) (default: the whole frame; fit_crop gives a centred one of the
        output's aspect ratio) is an area downscale (mcraw_demosaic_area_batch): every output pixel is the average of the
        CFA quads under its footprint in the crop, 1 .. 16 quads per pixel along each axis, the origin and size of the crop
        even; the result is (N, 3, Ho, Wo), and with h = 2 Ho, w = 2 Wo it is "bin2" of the crop, bit for bit.  The stages in
        front run on the whole mosaic.  size= or crop= with another algo, or "area" without size=, raises ValueError.
        algo "resample" with size=, crop= (as "area") and filter="cubic" (Catmull-Rom, the default) or "linear" covers the sizes
        from half to twice the crop (mcraw_demosaic_resample_batch): the "mhc" image of the whole frame behind a separable
        polyphase filter, in integers; with size= the crop's own size it is "mhc" cut to the crop, bit for bit.  The crop marks
        the sample positions: taps that leave it read the frame's real pixels (a stabilisation window; align_window gives
        one), and reflect at the frame's edges.  filter= with another algo raises ValueError.
        algo "warp" with size=(Ho, Wo), affine= and filter= (as "resample") samples the "mhc" image along one affine map per frame
        (mcraw_demosaic_warp_batch): the stabilisation warp, translation to 1/256 sample, roll up to about 14 degrees, zoom 0.75 ..
        1.25, in integers; with the identity and a translation of whole samples it is "mhc" cut there, bit for bit.  affine: an
        int32 array or tensor (6,) or (N, 6), {ayy, ayx, ty, axy, axx, tx} as the library takes them (stabilize() makes them), or
        a float array or tensor (2, 3) or (N, 2, 3), [[ayy, ayx, ty], [axy, axx, tx]] in samples, quantised by quantize_affine().
        The maps are host memory: a tensor on the device is brought to the host, which synchronises.  The four corners of the
        output must read inside the frame.  affine= with another algo, "warp" without size= or affine=, or crop= with "warp"
        raises ValueError.
        algo "ha" is the edge-directed demosaic (MCRAW_RGB_HA: Hamilton-Adams adaptive colour-plane interpolation in integers),
        (N, 3, H, W) as "mhc" and with every argument of "mhc": green follows the axis with the smaller gradient, R and B their
        differences against green, which keeps fine detail and high-contrast edges free of the zipper and false colour of the
        fixed 5x5 filter; on noisy input the direction follows the noise, so denoise= belongs in front of it.  "resample" and
        "warp" keep sampling the "mhc" image.
        algo "mesh" with size=(Ho, Wo), mesh= and filter= (as "warp") samples the "mhc" image along a mesh of source positions
        (mcraw_demosaic_mesh_batch): what is not affine -- lens distortion (distortion_mesh), the local motion that align_cells
        measures (stabilize_mesh), or any map (affine_mesh gives "warp"'s).  mesh: int32 (My, Mx, 2), (1, My, Mx, 2) or
        (N, My, Mx, 2) with (My, Mx) = mesh_grid(Ho, Wo), node (a, b) the position (Y, X) of output pixel (32 a, 32 b) in 1/256
        sample; positions in between are bilinear, and one that leaves the frame reads the frame's edge.  A contiguous CUDA tensor
        is used in place and nothing synchronises; a numpy array or CPU tensor is checked by mesh_check() first (ValueError with
        its message; check=False takes it as it is) and uploaded on the current stream.  mesh= with another algo, "mesh" without
        size= or mesh=, crop= or affine= with "mesh", or a wrong shape or dtype raises ValueError."""
        import torch
        code = _float_code(dtype)
        tdtype = {FLOAT_F32: torch.float32, FLOAT_F16: torch.float16, FLOAT_BF16: torch.bfloat16}[code]
        front = self._demosaic_front("demosaic", mosaic, algo, cfa, black, defects, denoise, shading, size, crop, filter, affine,
                                     highlights, white, gain, mesh, check)
        ho, wo = front.ho, front.wo
        out = self._demosaic_out("demosaic", front, out, (3, ho, wo), tdtype)
        if front.n == 0:
            return out
        return self._demosaic_call("mcraw_demosaic_batch", "demosaic", front, algo, code, FLOAT_CLIP if clip else 0, white, black,
                                   gain, matrix, out)

    def _demosaic_front(self, fn, mosaic, algo, cfa, black, defects, denoise, shading, size=None, crop=None, filter=None, affine=None,
                        highlights=None, white=None, gain=None, mesh=None, check=True):
        """What demosaic / demosaic_display / demosaic_yuv (`fn`) do alike in front of their output: the algo and cfa checks,
        the mosaic argument, the optional stages -- defects, then denoise, then highlights, then shading, each into a scratch tensor (the
        caller's mosaic stays as it is), none for an empty batch -- and the output size (`size` for the scaled algos).  Returns a
        _Front."""
        import torch
        if algo not in _RGB_ALGOS:
            raise ValueError("algo must be 'mhc', 'ha', 'bin2', 'area', 'resample', 'warp' or 'mesh', not %r" % (algo,))
        scaled = algo in _SCALED
        warp = algo == "warp"
        meshed = algo == "mesh"
        if mesh is not None and not meshed:
            raise ValueError("%s: mesh= belongs to algo='mesh', not %r" % (fn, algo))
        if meshed and (crop is not None or affine is not None):
            raise ValueError("%s: crop= and affine= do not go with algo='mesh' (the nodes say where every pixel reads)" % fn)
        if meshed and (size is None or mesh is None):
            raise ValueError("%s: algo='mesh' needs size=(Ho, Wo) and mesh=" % fn)
        if affine is not None and not warp:
            raise ValueError("%s: affine= belongs to algo='warp', not %r" % (fn, algo))
        if warp and crop is not None:
            raise ValueError("%s: crop= does not go with algo='warp' (the maps say where every pixel reads)" % fn)
        if warp and (size is None or affine is None):
            raise ValueError("%s: algo='warp' needs size=(Ho, Wo) and affine=" % fn)
        if not scaled and not warp and not meshed and (size is not None or crop is not None):
            raise ValueError("%s: size= and crop= belong to algo='area' and 'resample', not %r" % (fn, algo))
        if scaled and size is None:
            raise ValueError("%s: algo=%r needs size=(Ho, Wo)" % (fn, algo))
        if filter is not None and algo not in ("resample", "warp", "mesh"):
            raise ValueError("%s: filter= belongs to algo='resample', not %r" % (fn, algo))
        filt = None
        if algo in ("resample", "warp", "mesh"):
            filt = _FILTERS.get("cubic" if filter is None else filter)
            if filt is None:
                raise ValueError("%s: filter must be 'cubic' or 'linear', not %r" % (fn, filter))
        key = str(cfa).strip().lower()
        if key not in _CFA_CODES:
            raise ValueError("unknown cfa %r (rggb, bggr, grbg or gbrg)" % (cfa,))
        dev = self._torch_device(torch)
        mos, single = self._mosaic_arg(torch, dev, fn, mosaic)[:2]
        mos = self._pre_stages(fn, mos, black, defects, denoise, highlights, white, key, gain)
        if shading is not None and mos.numel():  # into a scratch tensor: the caller's mosaic stays as it is
            mos = self.shade(mos, shading, black=black)
        n, h, w = (int(v) for v in mos.shape)
        src = self._strided(fn, "the mosaic", mos, h, w) if n else None
        area = None
        if scaled:
            try:
                ho, wo = (int(v) for v in size)
                area = (0, 0, h // 2 * 2, w // 2 * 2) if crop is None else tuple(int(v) for v in crop)
            except (TypeError, ValueError):
                raise ValueError("%s: size must be (Ho, Wo) and crop (y0, x0, h, w)" % fn) from None
            if len(area) != 4 or min(area) < 0 or ho < 1 or wo < 1 or max(area + (ho, wo)) > 65536:
                raise ValueError("%s: size must be (Ho, Wo) and crop (y0, x0, h, w), all 0 .. 65536, not %r and %r" % (fn, size, crop))
        elif warp or meshed:
            try:
                ho, wo = (int(v) for v in size)
            except (TypeError, ValueError):
                raise ValueError("%s: size must be (Ho, Wo)" % fn) from None
            if ho < 1 or wo < 1 or max(ho, wo) > 65536:
                raise ValueError("%s: size must be (Ho, Wo), both 1 .. 65536, not %r" % (fn, size))
            if warp:
                maps = _affine_maps(fn, affine, n)
            else:
                nodes = self._mesh_tensor(torch, dev, fn, mesh, n, h, w, (ho, wo), check)
        else:
            ho, wo = (h, w) if algo in ("mhc", "ha") else (h // 2, w // 2)
        return _Front(mos, single, n, h, w, src, ho, wo, key, area, filt, maps if warp else None, nodes if meshed else None)

    def _mesh_tensor(self, torch, dev, fn, mesh, n, h, w, size, check):
        """mesh= of the demosaic methods as the contiguous int32 device tensor (nmesh, My, Mx, 2), nmesh 1 or n.  A tensor on the
        device is used in place and nothing synchronises; a host array or CPU tensor goes through mcraw_mesh_check first (check)
        and is uploaded on the current stream."""
        import numpy as np
        grid = mesh_grid(*size)
        def shape_ok(shape):
            shape = tuple(int(v) for v in shape)
            return shape == grid + (2,) or (len(shape) == 4 and shape[1:] == grid + (2,) and (shape[0] in (1, n) or not n))
        if isinstance(mesh, torch.Tensor) and mesh.device.type != "cpu":
            if mesh.dtype != torch.int32 or mesh.device != dev or not mesh.is_contiguous() or not shape_ok(mesh.shape):
                raise ValueError("%s: a mesh tensor must be contiguous int32 %r, (1, ...) or (%d, ...) on %s, not %s %r"
                                 % (fn, grid + (2,), n, dev, mesh.dtype, tuple(mesh.shape)))
            return mesh.reshape((-1,) + grid + (2,))
        if isinstance(mesh, torch.Tensor):
            mesh = mesh.detach().numpy()
        a = np.asarray(mesh)
        if a.dtype != np.int32 or not shape_ok(a.shape):
            raise ValueError("%s: mesh must be int32 %r, (1, ...) or (%d, ...), not %s %r" % (fn, grid + (2,), n, a.dtype, a.shape))
        a = np.ascontiguousarray(a.reshape((-1,) + grid + (2,)))
        if check and n:  # (an empty batch is a no-op whatever its frames' geometry)
            try:
                mesh_check(a, h, w, size)
            except ValueError as e:
                raise ValueError("%s: mesh: %s" % (fn, e)) from None
        return torch.from_numpy(a).to(dev, non_blocking=False)

    def _pre_stages(self, fn, mos, black, defects, denoise, highlights=None, white=None, cfa=None, gain=None):
        """defects=, denoise= and highlights= of the demosaic / decode methods, in that order, each into a scratch tensor; an
        empty batch passes through."""
        if defects is not None and mos.numel():  # in front of the gains
            mos = self._fix_defects(mos, defects, black, fn)
        if denoise is not None and mos.numel():  # on the sensor's values: behind the defects, in front of the gains
            mos = self._denoise_stage(mos, denoise, fn)
        if highlights is not None and mos.numel():  # behind the denoiser, in front of the gains, which move the clip level by position
            mos = self._highlights_stage(mos, highlights, fn, white, black, cfa, gain)
        return mos

    def _demosaic_out(self, fn, front, out, frame_shape, tdtype):
        """`out` of a demosaic method, checked or made: frame_shape per frame, without N for an (H, W) mosaic."""
        import torch
        want = tuple(frame_shape) if front.single else (front.n,) + tuple(frame_shape)
        return self._out_arg(torch, front.mos.device, fn, out, want, tdtype, contiguous=True)

    def _demosaic_call(self, symbol, fn, front, algo, dtype_code, flags, white, black, gain, matrix, out, stage=None, extra=()):
        """The tail of the three demosaics: colours, params and the library's `symbol` (stage: its display / YUV struct, None
        for the float entry; extra: further tensors that take part).  Returns out."""
        import torch
        mos, n, h, w, src = front.mos, front.n, front.h, front.w, front.src
        cols, nc = _rgb_colors(gain, matrix, n, fn)
        prm = _rgb_params(algo, dtype_code, flags, front.key, white, black)
        if algo == "warp":  # one entry point for the three families; the maps are host memory, read before the call returns
            a = Warp()
            a.out_h, a.out_w, a.filter, a.reserved = front.ho, front.wo, front.filt, 0
            d = C.byref(stage) if isinstance(stage, Display) else None
            y = C.byref(stage) if isinstance(stage, Yuv) else None
            maps = front.maps
            self._call(torch, mos.device, "mcraw_demosaic_warp_batch", (mos, out) + tuple(extra), C.byref(prm), C.byref(a), d, y, cols, nc,
                       maps.ctypes.data_as(C.POINTER(C.c_int32)), int(maps.shape[0]), *src, w, h, n, C.c_void_p(out.data_ptr()),
                       out.numel() * out.element_size())
            return out
        if algo == "mesh":  # one entry point for the three families; the nodes are device memory, read by the queued kernel
            a = Mesh()
            a.out_h, a.out_w, a.filter, a.reserved = front.ho, front.wo, front.filt, 0
            d = C.byref(stage) if isinstance(stage, Display) else None
            y = C.byref(stage) if isinstance(stage, Yuv) else None
            nodes = front.mesh
            self._call(torch, mos.device, "mcraw_demosaic_mesh_batch", (mos, out, nodes) + tuple(extra), C.byref(prm), C.byref(a), d, y, cols,
                       nc, C.c_void_p(nodes.data_ptr()), nodes.numel() * 4, int(nodes.shape[0]), *src, w, h, n,
                       C.c_void_p(out.data_ptr()), out.numel() * out.element_size())
            return out
        if algo in _SCALED:  # one entry point for the three families; its scratch lives as long as the call's other tensors
            struct, work_symbol, batch_symbol, rule = _SCALED[algo]
            a = struct()
            a.y0, a.x0, a.ch, a.cw = front.area
            a.out_h, a.out_w = front.ho, front.wo
            if front.filt is not None:
                a.filter = front.filt
            need = int(getattr(self._lib, work_symbol)(C.byref(a)))
            if need == 0:
                raise ValueError("%s: crop %r onto size %r: %s" % (fn, front.area, (front.ho, front.wo), rule))
            work = torch.empty((need,), dtype=torch.uint8, device=mos.device)
            d = C.byref(stage) if isinstance(stage, Display) else None
            y = C.byref(stage) if isinstance(stage, Yuv) else None
            self._call(torch, mos.device, batch_symbol, (mos, out, work) + tuple(extra), C.byref(prm), C.byref(a), d, y, cols, nc, *src,
                       w, h, n, C.c_void_p(work.data_ptr()), need, C.c_void_p(out.data_ptr()), out.numel() * out.element_size())
            return out
        structs = (C.byref(prm),) if stage is None else (C.byref(prm), C.byref(stage))
        self._call(torch, mos.device, symbol, (mos, out) + tuple(extra), *structs, cols, nc, *src, w, h, n,
                   C.c_void_p(out.data_ptr()), out.numel() * out.element_size())
        return out

    def _decode_scratch(self, inputs, width, height, type, check, fn):
        """The plain uint16 mosaics of frames resident in HBM, decoded into a scratch tensor on the current stream (for
        decode_rgb / decode_display; the stage is restored afterwards)."""
        import torch
        width, height, n = int(width), int(height), len(inputs)
        dev = self._torch_device(torch)
        scratch = torch.empty((n, height, width), dtype=torch.uint16, device=dev)
        descs = []
        for i, x in enumerate(inputs):
            if isinstance(x, torch.Tensor):
                if x.dtype != torch.uint8 or x.device != dev or not x.is_contiguous():
                    raise ValueError("%s: inputs must be contiguous uint8 tensors on %s" % (fn, dev))
                ptr, ln = x.data_ptr(), x.numel()
            else:
                ptr, ln = int(x[0]), int(x[1])
            descs.append((ptr, ln, width, height, int(type), scratch.data_ptr() + i * width * height * 2, width * height))
        if n:
            cur, run = self._run_stream(torch, dev)
            prev = self._stage
            self.set_post()
            try:
                res = self.decode_batch(self.make_frames(descs), mem=MEM_DEVICE, stream=C.c_void_p(run.cuda_stream), want_status=check)
            finally:
                self._restore_stage(prev)
                if run is not cur:
                    scratch.record_stream(run)
                    cur.wait_stream(run)
            if check:
                bad = [(i, st) for i, st in enumerate(res[1]) if st != 0]
                if bad:
                    raise McrawError("%s: %d of %d frames failed: %s" % (
                        fn, len(bad), n, ", ".join("frame %d status 0x%x" % b for b in bad[:16])))
        return scratch

    def _decode_front(self, fn, inputs, width, height, type, check, black, defects, denoise, shading, highlights=None, white=None,
                      cfa=None, gain=None):
        """The scratch mosaics of decode_rgb / decode_display / decode_yuv (`fn`), ready for the demosaic: decoded, then
        defects=, denoise= and highlights= (each into a further scratch tensor), then shading= in place."""
        scratch = self._pre_stages(fn, self._decode_scratch(inputs, width, height, type, check, fn), black, defects, denoise, highlights,
                                   white, cfa, gain)
        if shading is not None:
            self.shade(scratch, shading, black=black, out=scratch)
        return scratch

    def decode_rgb(self, inputs, width, height, type, *, algo="mhc", dtype, white, black=(0, 0, 0, 0), cfa="rggb",
                   gain=None, matrix=None, clip=False, out=None, check=True, shading=None, defects=None, denoise=None, size=None,
                   crop=None, filter=None, affine=None, highlights=None, mesh=None):
        """Decode frames of one geometry that are resident in HBM and demosaic them (demosaic()): (N, 3, H, W) for "mhc",
        (N, 3, H/2, W/2) for "bin2", (N, 3, Ho, Wo) for "area" with size=(Ho, Wo) and crop=.  inputs: uint8 CUDA tensors, or (device pointer, length) pairs.  The plain uint16
        mosaics go to a scratch tensor of torch's caching allocator; both steps are queued on torch.cuda.current_stream().
        check=True synchronises after the decode and raises McrawError naming the frames that failed; check=False returns
        at once.  The stage the context had before the call is restored afterwards.  shading: a lens-shading gain map
        (shade()), applied to the scratch mosaics in place before the demosaic.  defects: a dict of fix_pixels()' keyword
        arguments (black defaults to this call's), applied in front of shading= into a second scratch tensor.  denoise: a
        dict of denoise()'s keyword arguments, applied behind defects= and in front of shading=.  highlights: a dict of
        highlights()' keyword arguments, as demosaic() fills it in, applied behind denoise= and in front of shading=."""
        scratch = self._decode_front("decode_rgb", inputs, width, height, type, check, black, defects, denoise, shading, highlights,
                                     white, cfa, gain)
        return self.demosaic(scratch, algo=algo, dtype=dtype, white=white, black=black, cfa=cfa, gain=gain, matrix=matrix,
                             clip=clip, out=out, check=check, size=size, crop=crop, filter=filter, affine=affine, mesh=mesh)

    def _display_lut(self, torch, dev, fn, transfer, lut_size, bits):
        """(device LUT tensor, caller-owned?) for demosaic_display / demosaic_yuv (`fn`): a ready 1-D uint16 LUT (CUDA tensor on
        `dev`, or a host array, uploaded), or the built-in curve of transfer_lut, built once per (curve, size, bits, device)."""
        import numpy as np
        if isinstance(transfer, torch.Tensor):
            if transfer.device != dev or transfer.dim() != 1 or transfer.dtype not in (torch.uint16, torch.int16) \
                    or not transfer.is_contiguous():
                raise ValueError("%s: a LUT tensor must be a contiguous 1-D uint16 tensor on %s" % (fn, dev))
            lut, own = transfer.view(torch.uint16), True
        elif isinstance(transfer, np.ndarray):
            if transfer.ndim != 1 or transfer.dtype != np.uint16:
                raise ValueError("%s: a LUT array must be 1-D uint16" % fn)
            lut, own = torch.from_numpy(np.ascontiguousarray(transfer).view(np.int16)).to(dev).view(torch.uint16), True
        else:
            key = (transfer if isinstance(transfer, str) else float(transfer) if not callable(transfer) else None,
                   int(lut_size), int(bits), str(dev))
            cache = self.__dict__.setdefault("_luts", {})
            lut = cache.get(key) if key[0] is not None else None
            if lut is None:
                host = transfer_lut(transfer, lut_size, bits)
                lut = torch.from_numpy(host.view(np.int16)).to(dev).view(torch.uint16)
                if key[0] is not None:
                    cache[key] = lut
            own = False
        L = int(lut.numel())
        if L < 256 or L > 65536 or L & (L - 1):
            raise ValueError("%s: the LUT length must be a power of two, 256 .. 65536, not %d" % (fn, L))
        return lut, own

    def demosaic_display(self, mosaic, *, algo="mhc", white, black=(0, 0, 0, 0), cfa="rggb", gain=None, matrix=None,
                         transfer="srgb", lut_size=4096, dtype=None, layout="hwc", bits=None, out=None, check=True, shading=None,
                         defects=None, denoise=None, size=None, crop=None, filter=None, affine=None, highlights=None, mesh=None):
        """uint16 mosaics resident on the context's device -> display-ready integer RGB: the demosaic and colours of
        demosaic(), then clamp to [0, 1], index a transfer-curve LUT of L entries at rint(c * (L - 1)) and store the entry
        (its low byte for uint8).  dtype: torch.uint8 (default) or torch.uint16; layout "hwc" gives (N, Ho, Wo, 3), "chw"
        (N, 3, Ho, Wo) (an (H, W) mosaic drops N).  transfer: "srgb", "bt709", "linear", a gamma g (x ** (1/g)), a callable
        on [0, 1] -- built by transfer_lut(transfer, lut_size, bits), bits 8 for uint8 and 16 for uint16 unless given --
        or a ready 1-D uint16 LUT (host array or CUDA tensor) whose length is a power of two, 256 .. 65536.  Queued on
        torch.cuda.current_stream(); nothing synchronises, and a caller's LUT is read when the kernels run (in stream
        order).  `check` is accepted for symmetry with decode_display.  shading, defects, denoise, highlights, and algo
        "area" with size= and crop=: as demosaic()."""
        import torch
        dtype = torch.uint8 if dtype is None else dtype
        dcode = {torch.uint8: DISP_U8, torch.uint16: DISP_U16, "u8": DISP_U8, "u16": DISP_U16}.get(dtype)
        if dcode is None:
            raise ValueError("demosaic_display: dtype must be torch.uint8 or torch.uint16, not %r" % (dtype,))
        if layout not in _DISP_LAYOUTS:
            raise ValueError("demosaic_display: layout must be 'hwc' or 'chw', not %r" % (layout,))
        front = self._demosaic_front("demosaic_display", mosaic, algo, cfa, black, defects, denoise, shading, size, crop, filter, affine,
                                     highlights, white, gain, mesh, check)
        ho, wo = front.ho, front.wo
        out = self._demosaic_out("demosaic_display", front, out, (ho, wo, 3) if layout == "hwc" else (3, ho, wo),
                                 torch.uint8 if dcode == DISP_U8 else torch.uint16)
        if front.n == 0:
            return out
        lut, own = self._display_lut(torch, out.device, "demosaic_display", transfer, lut_size,
                                     (8 if dcode == DISP_U8 else 16) if bits is None else bits)
        d = Display()
        d.dtype, d.layout, d.lut_log2, d.reserved = dcode, _DISP_LAYOUTS[layout], int(lut.numel()).bit_length() - 1, 0
        d.lut = lut.data_ptr()
        return self._demosaic_call("mcraw_demosaic_display_batch", "demosaic_display", front, algo, 0, 0, white, black, gain, matrix,
                                   out, d, (lut if own else None,))

    def decode_display(self, inputs, width, height, type, *, algo="mhc", white, black=(0, 0, 0, 0), cfa="rggb", gain=None,
                       matrix=None, transfer="srgb", lut_size=4096, dtype=None, layout="hwc", bits=None, out=None, check=True, shading=None,
                       defects=None, denoise=None, size=None, crop=None, filter=None, affine=None, highlights=None, mesh=None):
        """Decode frames of one geometry that are resident in HBM and turn them into display-ready RGB
        (demosaic_display()), as decode_rgb does: the plain uint16 mosaics go to a scratch tensor, both steps are queued on
        torch.cuda.current_stream(), check=True synchronises after the decode and raises McrawError naming the frames that
        failed, and the context's stage is restored afterwards.  shading, defects, denoise, highlights: as decode_rgb()."""
        scratch = self._decode_front("decode_display", inputs, width, height, type, check, black, defects, denoise, shading, highlights,
                                     white, cfa, gain)
        return self.demosaic_display(scratch, algo=algo, white=white, black=black, cfa=cfa, gain=gain, matrix=matrix,
                                     transfer=transfer, lut_size=lut_size, dtype=dtype, layout=layout, bits=bits, out=out,
                                     check=check, size=size, crop=crop, filter=filter, affine=affine, mesh=mesh)

    def demosaic_yuv(self, mosaic, *, algo="mhc", white, black=(0, 0, 0, 0), cfa="rggb", gain=None, matrix=None, fmt="nv12",
                     standard="bt709", range="limited", transfer="bt709", lut_size=4096, in_bits=None, out=None, check=True, shading=None,
                     defects=None, denoise=None, size=None, crop=None, filter=None, affine=None, highlights=None, mesh=None):
        """uint16 mosaics resident on the context's device -> video-ready Y'CbCr 4:2:0: the demosaic, colours, clamp and
        transfer-curve LUT of demosaic_display(), then the integer matrix of yuv_matrix(standard, range) and a 2x2 box
        average for the chroma (sited at the block's centre).  fmt "nv12": torch.uint8; "p010": torch.uint16 holding
        10-bit codes << 6.  Result (N, Ho * 3 // 2, Wo) (an (H, W) mosaic drops N): per frame the Y plane (Ho rows), then
        Ho / 2 rows of interleaved (Cb, Cr) -- the bytes ffmpeg reads as -f rawvideo -pix_fmt nv12 / p010le; yuv_planes()
        gives the two as views.  Ho and Wo must be even (bin2: H and W multiples of 4).  transfer: as demosaic_display; a
        built-in curve is transfer_lut(transfer, lut_size, in_bits), in_bits defaulting to 12 (nv12) or 16 (p010); a ready
        LUT may hold entries of any in_bits 8 .. 16 (higher bits are masked off).  Queued on torch.cuda.current_stream();
        nothing synchronises.  `check` is accepted for symmetry with decode_yuv.  shading, defects, denoise, highlights, and algo
        "area" with size= (both even) and crop=: as demosaic()."""
        import torch
        if fmt not in _YUV_FORMATS:
            raise ValueError("demosaic_yuv: fmt must be 'nv12' or 'p010', not %r" % (fmt,))
        fcode, bits, default_in = _YUV_FORMATS[fmt]
        in_bits = default_in if in_bits is None else in_bits
        cy, cb, cr, sh, y_off, c_off = yuv_matrix(standard, range, bits, in_bits)
        front = self._demosaic_front("demosaic_yuv", mosaic, algo, cfa, black, defects, denoise, shading, size, crop, filter, affine,
                                     highlights, white, gain, mesh, check)
        ho, wo = front.ho, front.wo
        out = self._demosaic_out("demosaic_yuv", front, out, (ho * 3 // 2, wo), torch.uint8 if fcode == YUV_NV12 else torch.uint16)
        if front.n == 0:
            return out
        lut, own = self._display_lut(torch, out.device, "demosaic_yuv", transfer, lut_size, in_bits)
        y = Yuv()
        y.format, y.lut_log2, y.in_bits, y.sh, y.y_off, y.c_off = fcode, int(lut.numel()).bit_length() - 1, in_bits, sh, y_off, c_off
        for i in (0, 1, 2):
            y.cy[i], y.cb[i], y.cr[i] = cy[i], cb[i], cr[i]
        y.reserved = 0
        y.lut = lut.data_ptr()
        return self._demosaic_call("mcraw_demosaic_yuv_batch", "demosaic_yuv", front, algo, 0, 0, white, black, gain, matrix, out, y,
                                   (lut if own else None,))

    def decode_yuv(self, inputs, width, height, type, *, algo="mhc", white, black=(0, 0, 0, 0), cfa="rggb", gain=None,
                   matrix=None, fmt="nv12", standard="bt709", range="limited", transfer="bt709", lut_size=4096, in_bits=None,
                   out=None, check=True, shading=None, defects=None, denoise=None, size=None, crop=None, filter=None, affine=None, highlights=None, mesh=None):
        """Decode frames of one geometry that are resident in HBM and turn them into NV12 / P010 (demosaic_yuv()), as
        decode_display does: the plain uint16 mosaics go to a scratch tensor, both steps are queued on
        torch.cuda.current_stream(), check=True synchronises after the decode and raises McrawError naming the frames that
        failed, and the context's stage is restored afterwards.  shading, defects, denoise, highlights: as decode_rgb()."""
        scratch = self._decode_front("decode_yuv", inputs, width, height, type, check, black, defects, denoise, shading, highlights,
                                     white, cfa, gain)
        return self.demosaic_yuv(scratch, algo=algo, white=white, black=black, cfa=cfa, gain=gain, matrix=matrix, fmt=fmt,
                                 standard=standard, range=range, transfer=transfer, lut_size=lut_size, in_bits=in_bits, out=out,
                                 check=check, size=size, crop=crop, filter=filter, affine=affine, mesh=mesh)

    def profile(self, enable=True, only=None, every=1):
        """Bracket kernel launches with events: all kernels, or just the names in `only`; every `every`-th launch."""
        self._lib.mcraw_ctx_profile_every(self._h, max(1, int(every)))
        if only:
            mode = 0
            for name in only:
                mode |= 2 << _kernel_id(name)
        else:
            mode = 1 if enable else 0
        self._lib.mcraw_ctx_profile(self._h, mode)

    def kernel_ms(self, name, reset=False):
        ms = C.c_double()
        n = C.c_int()
        kid = _kernel_id(name)
        rc = self._lib.mcraw_ctx_kernel_ms(self._h, kid, C.byref(ms), C.byref(n), 1 if reset else 0)
        if rc != 0:
            raise McrawError("mcraw_ctx_kernel_ms failed (%d)" % rc)
        return ms.value, n.value
