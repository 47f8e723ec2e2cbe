"""numpy reference of the YUV stage (mcraw_demosaic_yuv_batch, include/mcraw_hip.h), bit-exact.

On top of _rgb_ref.rgb_values (the f32 outputs o) and _display_ref.lut_index: P_c = lut[i_c] & (2^in_bits - 1), then in
integers (int64 here, with an assertion that every sum stays inside int32; >> is an arithmetic shift)
    Y  = clamp(((cy . P + 2^(sh - 1)) >> sh) + y_off, 0, top)            per pixel
    S  = sum of P over each 2x2 block of output pixels
    Cb = clamp(((cb . S + 2^(sh + 1)) >> (sh + 2)) + c_off, 0, top)      per block; Cr likewise
fmt "nv12": top = 255, uint8; "p010": top = 1023, uint16 holding code << 6.  A frame is (ho * 3 // 2, wo): the Y plane,
then ho / 2 rows of wo / 2 interleaved (Cb, Cr) pairs."""
import numpy as np

from _display_ref import lut_index
from _rgb_ref import rgb_values

BITS = {"nv12": 8, "p010": 10}
DTYPE = {"nv12": np.uint8, "p010": np.uint16}
I32 = 1 << 31


def rule_ok(rows, sh, in_bits):
    """The overflow rule: 4 * (2^in_bits - 1) * (|c0| + |c1| + |c2|) + 2^(sh + 1) < 2^31 for every row."""
    return all(4 * ((1 << in_bits) - 1) * sum(abs(int(c)) for c in r) + (1 << (sh + 1)) < I32 for r in rows)


def _dot(c, v, rnd):
    s = int(c[0]) * v[0] + int(c[1]) * v[1] + int(c[2]) * v[2]
    for part in (int(c[0]) * v[0], int(c[0]) * v[0] + int(c[1]) * v[1], s, s + rnd):
        assert part.min() >= -I32 and part.max() < I32, "an int32 sum would wrap"
    return s + rnd


def yuv_codes(P, cy, cb, cr, sh, y_off, c_off, bits):
    """P (3, h, w) integers -> (Y (h, w), Cb (h/2, w/2), Cr (h/2, w/2)) codes, int64."""
    P = np.asarray(P).astype(np.int64)
    top = (1 << bits) - 1
    Y = np.clip((_dot(cy, P, 1 << (sh - 1)) >> sh) + y_off, 0, top)
    S = P[:, 0::2, 0::2] + P[:, 0::2, 1::2] + P[:, 1::2, 0::2] + P[:, 1::2, 1::2]
    Cb = np.clip((_dot(cb, S, 1 << (sh + 1)) >> (sh + 2)) + c_off, 0, top)
    Cr = np.clip((_dot(cr, S, 1 << (sh + 1)) >> (sh + 2)) + c_off, 0, top)
    return Y, Cb, Cr


def pack(Y, Cb, Cr, fmt):
    """The frame as stored: (h * 3 // 2, w), the Y rows then the interleaved (Cb, Cr) rows; P010 holds code << 6."""
    h, w = Y.shape
    out = np.empty((h * 3 // 2, w), dtype=np.int64)
    out[:h] = Y
    out[h:, 0::2] = Cb
    out[h:, 1::2] = Cr
    if fmt == "p010":
        out <<= 6
    return out.astype(DTYPE[fmt])


def yuv_from_o(o, lut, fmt, coef, in_bits):
    """The stage behind the colour stage: o (3, ho, wo) f32 -> the stored frame.  coef = (cy, cb, cr, sh, y_off, c_off)."""
    lut = np.asarray(lut, dtype=np.uint16)
    P = lut[lut_index(o, len(lut))].astype(np.int64) & ((1 << in_bits) - 1)
    cy, cb, cr, sh, y_off, c_off = coef
    return pack(*yuv_codes(P, cy, cb, cr, sh, y_off, c_off, BITS[fmt]), fmt)


def yuv_ref(img, algo, white, lut, fmt, coef, in_bits, black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1), matrix=None):
    """The output of one frame: uint8 (nv12) or uint16 (p010), (ho * 3 // 2, wo)."""
    o = rgb_values(img, algo, white, black, cfa, gain, matrix, clip=False)
    return yuv_from_o(o, lut, fmt, coef, in_bits)
