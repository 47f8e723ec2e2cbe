"""What the GPU tests of the demosaic entry points (test_gpu_rgb / _display / _yuv / _area / _resample .py) build alike:
constants, tensors to and from numpy, random inputs, the C structs, encoded frames with the oracle's decode, and the raw C calls."""
import ctypes as C

import numpy as np
import torch

import _libs as L
import _rgb_ref as R
import _yuv_ref as Y
import motioncam_decoder_amd as M

DEV = torch.device("cuda:0")
CFAS = ("rggb", "bggr", "grbg", "gbrg")
SENT = 0xA5
GUARD = 4096
SRGBISH = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)


def to_np(t):
    """uint8 / uint16 tensor -> numpy (torch has few CUDA kernels for uint16: go through int16)."""
    a = t.detach()
    if a.dtype == torch.uint16:
        return a.view(torch.int16).cpu().numpy().view(np.uint16)
    return a.cpu().numpy()


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def mosaic(rng, h, w, nbits):
    return rng.integers(0, 1 << nbits, size=(h, w), dtype=np.uint16)


def rand_lut(rng, size):
    return rng.integers(0, 1 << 16, size=size, dtype=np.uint16)


def rgb_params(algo="mhc", white=4095.0, black=(0, 0, 0, 0), cfa="rggb", dtype=0, flags=0):
    p = M.RgbParams()
    p.algo = {"mhc": 1, "bin2": 2}[algo]
    p.dtype, p.flags, p.cfa = dtype, flags, R.CFA_CODE[cfa]
    for i in range(4):
        p.black[i] = black[i]
    p.white = white
    return p


def rgb_color(gain=(1, 1, 1), m=None):
    c = M.RgbColor()
    m = np.eye(3) if m is None else np.asarray(m)
    for i in range(3):
        c.gain[i] = float(gain[i])
    for i in range(9):
        c.m[i] = float(m.ravel()[i])
    return c


def frames(rng, shapes, typ):
    items = []
    for (w, h) in shapes:
        img = L.natural_image_np(w, h, 12, 12.0, int(rng.integers(1 << 30)))
        buf = L.encode7(img) if typ == 7 else L.encode6(img)
        ret, want = (L.oracle_decode7 if typ == 7 else L.oracle_decode6)(buf, w, h)
        assert ret == w * h
        items.append((buf, want))
    return items


def raw_call(ctx, symbol, prm, stage, cols, ncol, in_ptr, pitch, fstride, w, h, n, out_ptr, out_bytes, stream=None, staged=True):
    """The C entry point `symbol` as it is: prm and stage may be None (a NULL pointer); staged=False: the float entry, which
    takes no stage struct."""
    arr = (M.RgbColor * max(ncol, 1))()
    for i in range(min(ncol, len(cols))):
        arr[i] = cols[i]
    structs = [C.byref(prm) if prm is not None else None]
    if staged:
        structs.append(C.byref(stage) if stage is not None else None)
    return getattr(M.load(), symbol)(ctx._h, *structs, arr, ncol, C.c_void_p(in_ptr), pitch, fstride, w, h, n, C.c_void_p(out_ptr),
                                     out_bytes, C.c_void_p(stream))


# ---- the scaled entry points (test_gpu_area / _resample .py)

FLOATS = (("f32", torch.int32), ("f16", torch.int16), ("bf16", torch.int16))
TD = {"u8": torch.uint8, "u16": torch.uint16, "nv12": torch.uint8, "p010": torch.uint16}
IN_BITS = 11


def bits(t, view):
    return t.contiguous().view(view).cpu().numpy().view(np.uint32 if view == torch.int32 else np.uint16)


def as_int(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def display(lut_ptr, dtype="u8", layout="hwc", log2=12):
    d = M.Display()
    d.dtype, d.layout, d.lut_log2, d.reserved, d.lut = M.DISP_U8 if dtype == "u8" else M.DISP_U16, M._DISP_LAYOUTS[layout], log2, 0, lut_ptr
    return d


def yuv(lut_ptr, fmt="nv12", log2=12, in_bits=IN_BITS):
    cy, cb, cr, sh, y_off, c_off = M.yuv_matrix("bt709", "limited", Y.BITS[fmt], in_bits)
    y = M.Yuv()
    y.format, y.lut_log2, y.in_bits, y.sh, y.y_off, y.c_off = (1 if fmt == "nv12" else 2), log2, in_bits, sh, y_off, c_off
    for i in range(3):
        y.cy[i], y.cb[i], y.cr[i] = cy[i], cb[i], cr[i]
    y.reserved, y.lut = 0, lut_ptr
    return y


def colours(gain, matrix, i):
    g = np.asarray(gain, dtype=np.float32)
    m = np.asarray(matrix, dtype=np.float32)
    return (g[i] if g.ndim == 2 else g), (m[i] if m.ndim == 3 else m)


def raw_scaled_call(symbol, ctx, prm, win, d, y, cols, ncol, in_ptr, pitch, fstride, w, h, n, work_ptr, work_bytes, out_ptr, out_bytes,
                    stream=None):
    """The C entry point `symbol` of a scaled algo as it is: prm, win (its window struct), d and y may be None (NULL pointers)."""
    arr = (M.RgbColor * max(ncol, 1))()
    for i in range(min(ncol, len(cols))):
        arr[i] = cols[i]
    ref = [C.byref(s) if s is not None else None for s in (prm, win, d, y)]
    return getattr(M.load(), symbol)(ctx._h, *ref, arr, ncol, C.c_void_p(in_ptr), pitch, fstride, w, h, n, C.c_void_p(work_ptr),
                                     work_bytes, C.c_void_p(out_ptr), out_bytes, C.c_void_p(stream))


def work_bytes(symbol, win):
    """The scratch that the window struct `win` needs, from the library's `symbol`."""
    need = int(getattr(M.load(), symbol)(C.byref(win)))
    assert need > 0
    return need
