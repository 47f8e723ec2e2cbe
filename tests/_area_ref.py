"""numpy statement of the area downscale (mcraw_demosaic_area_batch, include/mcraw_hip.h), bit-exact.

Per axis, Q quads of the crop onto O output pixels:
    c(k, q) = clamp(floor((256 * (q * O - k * Q) + (Q >> 1)) / Q), 0, 256),   w(k, q) = c(k, q + 1) - c(k, q), q from floor(k Q / O)
e: _rgb_ref.bin2_estimates of the crop;  h = sum_q wx e;  t = (h + 8) >> 4;  v = sum_q wy t;  E = (v + 128) >> 8, in units of
1/32.  Behind E the colour stage, the LUT and the Y'CbCr matrix are _rgb_ref's, _display_ref's and _yuv_ref's, with
k[c] = (gain[c] * inv) * (1/32)."""
import numpy as np

import _display_ref as D
import _rgb_ref as R
import _yuv_ref as Y
from _float_ref import bf16_bits

TAPS = 17
I32 = 1 << 31


def coef(k, q, Q, O):
    """c(k, q) on integer arrays (int64; Python's // is the floor division)."""
    k, q = np.asarray(k, dtype=np.int64), np.asarray(q, dtype=np.int64)
    return np.clip((256 * (q * O - k * Q) + (Q >> 1)) // Q, 0, 256)


def weights(Q, O):
    """(q0 (O,), w (O, 17)) int64: the first quad under every output pixel and the weights of the 17 quads from it on.  Asserts
    that no 18th quad carries weight."""
    k = np.arange(O, dtype=np.int64)
    q0 = k * Q // O
    c = coef(k[:, None], q0[:, None] + np.arange(TAPS + 1)[None, :], Q, O)
    assert (c[:, 0] == 0).all() and (c[:, -1] == 256).all(), "more than 17 taps"
    return q0, c[:, 1:] - c[:, :-1]


def reduce_axis(e, O, axis):
    """sum_q w(k, q) e[.., q, ..] along `axis` of the integer array e: the 17 taps of every output index, gathered."""
    e = np.moveaxis(np.asarray(e).astype(np.int64), axis, -1)
    Q = e.shape[-1]
    q0, w = weights(Q, O)
    last = np.where(w > 0, np.arange(TAPS)[None, :], -1).max(axis=1)
    assert (q0 + last < Q).all(), "a tap behind the crop"
    pad = np.concatenate([e, np.zeros(e.shape[:-1] + (TAPS,), dtype=np.int64)], axis=-1)
    out = np.zeros(e.shape[:-1] + (O,), dtype=np.int64)
    for t in range(TAPS):
        out += pad[..., q0 + t] * w[:, t]
    return np.moveaxis(out, -1, axis)


def area_from_e(e, size):
    """e (3, Qh, Qw) integers, BIN2's estimates -> E (3, Ho, Wo) int64, with the contract's int32 bounds asserted."""
    ho, wo = size
    h = reduce_axis(e, wo, 2)  # (3, Qh, Wo)
    assert np.abs(h).max() <= 256 * 131070
    t = (h + 8) >> 4
    v = reduce_axis(t, ho, 1)
    assert np.abs(v).max() < 1 << 30
    E = (v + 128) >> 8
    assert np.abs(E).max() < 1 << 22
    return E


def area_estimates(img, crop, size, black=(0, 0, 0, 0), cfa="rggb"):
    """E (3, Ho, Wo) int64 in units of 1/32.  crop (y0, x0, h, w), all even; size (Ho, Wo)."""
    y0, x0, h, w = crop
    assert not (y0 | x0 | h | w) & 1
    sub = np.asarray(img)[y0:y0 + h, x0:x0 + w]
    assert sub.shape == (h, w)
    return area_from_e(R.bin2_estimates(sub, black, cfa), size)


def values(E, white, black=(0, 0, 0, 0), gain=(1, 1, 1), matrix=None, clip=False):
    """The f32 outputs o (3, Ho, Wo): _rgb_ref.rgb_values' colour stage on E with k = (gain * inv) * (1/32)."""
    k = R.scales("bin2", white, black, gain) * np.float32(0.0625)  # (g * inv) * 0.5 * 0.0625: powers of two, exact
    m = np.eye(3, dtype=np.float32) if matrix is None else np.asarray(matrix, dtype=np.float32).reshape(3, 3)
    v = [E[c].astype(np.float32) * k[c] for c in range(3)]
    o = np.stack([(m[i, 0] * v[0] + m[i, 1] * v[1]) + m[i, 2] * v[2] for i in range(3)]).astype(np.float32)
    if clip:
        o = np.minimum(np.maximum(o, np.float32(0.0)), np.float32(1.0))
    return o


def float_bits(o, dtype):
    """o as the stored bit patterns: uint32 for f32, uint16 for f16 / bf16."""
    if dtype == "f32":
        return np.ascontiguousarray(o).view(np.uint32)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return o.astype(np.float16).view(np.uint16)
    return bf16_bits(o)


def area_ref(img, crop, size, dtype, white, black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1), matrix=None, clip=False):
    return float_bits(values(area_estimates(img, crop, size, black, cfa), white, black, gain, matrix, clip), dtype)


def display_from_o(o, lut, dtype="u8", layout="hwc"):
    q = D.apply_lut(o, lut, dtype)
    return np.ascontiguousarray(q.transpose(1, 2, 0)) if layout == "hwc" else q


def area_display_ref(img, crop, size, white, lut, dtype="u8", layout="hwc", black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1),
                     matrix=None):
    return display_from_o(values(area_estimates(img, crop, size, black, cfa), white, black, gain, matrix), lut, dtype, layout)


def area_yuv_ref(img, crop, size, white, lut, fmt, coef, in_bits, black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1), matrix=None):
    return Y.yuv_from_o(values(area_estimates(img, crop, size, black, cfa), white, black, gain, matrix), lut, fmt, coef, in_bits)


def fit_crop(height, width, ho, wo):
    """The contract of motioncam_decoder_amd.fit_crop, restated."""
    if width * ho <= height * wo:
        w, h = width // 2 * 2, width * ho // wo // 2 * 2
    else:
        h, w = height // 2 * 2, height * wo // ho // 2 * 2
    return ((height - h) // 4 * 2, (width - w) // 4 * 2, h, w)
