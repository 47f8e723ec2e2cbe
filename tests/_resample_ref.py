"""numpy statement of the resampling demosaic (mcraw_demosaic_resample_batch, include/mcraw_hip.h), bit-exact.

e: _rgb_ref.mhc_estimates of the WHOLE frame (1/16 DN), reflected 101-style beyond its edges.  Per axis, C crop samples onto O
pixels (j counts from the crop's origin):
    D = 2 max(C, O);  n(k, j) = 2 O j - ((2 k + 1) C - O);  a = (1024 |n| + D // 2) // D
    linear f = max(0, 1024 - a);  cubic f = Catmull-Rom times 2 * 1024^3 (kernel_f below)
    w = (4096 f + F // 2) // F, F = sum f; the residual 4096 - sum w goes to the tap of smallest |n| (half each to two such taps)
    t = (sum_j wx e + 2048) >> 12 along x, then E = (sum_j wy t + 2048) >> 12 along y
Behind E the colour stage, the LUT and the Y'CbCr matrix are _rgb_ref's, _display_ref's and _yuv_ref's, with MHC's k[c]."""
import numpy as np

import _area_ref as A
import _rgb_ref as R
import _yuv_ref as Y

TAPS = {"linear": 5, "cubic": 9}
FILTER_CODE = {"linear": 0, "cubic": 1}
CAND = 12   # candidates jc - 5 .. jc + 6 round jc = floor(u)
REACH = 4   # taps leave the crop by at most this many samples


def kernel_f(a, filt):
    """The raw kernel value at distance a / 1024 of the stretched unit (int64 arrays)."""
    a = np.asarray(a, dtype=np.int64)
    if filt == "linear":
        return np.maximum(0, 1024 - a)
    near = 3 * a ** 3 - 5 * 1024 * a ** 2 + 2 * 1024 ** 3
    far = -a ** 3 + 5 * 1024 * a ** 2 - 8 * 1024 ** 2 * a + 4 * 1024 ** 3
    return np.where(a <= 1024, near, np.where(a < 2048, far, 0))


def weights(C, O, filt):
    """(j0 (O,), nt (O,), w (O, 9)) int64: the first sample that carries weight (relative to the crop), the taps from it to the
    last that does, and their weights (0 behind nt)."""
    assert 2 * O >= C and O <= 2 * C and filt in TAPS
    k = np.arange(O, dtype=np.int64)
    D = 2 * max(C, O)
    jc = ((2 * k + 1) * C - O) // (2 * O)
    j = jc[:, None] - 5 + np.arange(CAND, dtype=np.int64)[None, :]
    n = 2 * O * j - ((2 * k[:, None] + 1) * C - O)
    f = kernel_f((1024 * np.abs(n) + D // 2) // D, filt)
    assert (f[:, 0] == 0).all() and (f[:, -1] == 0).all(), "a tap beyond the candidates"
    F = f.sum(axis=1, keepdims=True)
    w = (4096 * f + F // 2) // F
    res = 4096 - w.sum(axis=1)
    near = np.where(f != 0, np.abs(n), np.iinfo(np.int64).max)
    near = near == near.min(axis=1, keepdims=True)
    cnt = near.sum(axis=1)
    assert ((cnt == 1) | (cnt == 2)).all() and (res[cnt == 2] % 2 == 0).all()
    rows = np.arange(O)
    half = np.where(cnt == 2, res // 2, 0)
    w[rows, near.argmax(axis=1)] += res - half
    w[rows, CAND - 1 - near[:, ::-1].argmax(axis=1)] += half
    nz = f != 0
    first = nz.argmax(axis=1)
    last = CAND - 1 - nz[:, ::-1].argmax(axis=1)
    nt = last - first + 1
    assert nt.max() <= TAPS[filt]
    idx = first[:, None] + np.arange(9)[None, :]
    out = np.where(np.arange(9)[None, :] < nt[:, None], np.take_along_axis(w, np.minimum(idx, CAND - 1), axis=1), 0)
    return jc - 5 + first, nt, out


def filter_axis(e, origin, C, O, filt, axis):
    """(sum_j w(k, j) e[origin + j] + 2048) >> 12 along `axis` of the integer array e, which is the frame padded by REACH on
    that axis (so frame index i sits at i + REACH)."""
    e = np.moveaxis(np.asarray(e).astype(np.int64), axis, -1)
    j0, nt, w = weights(C, O, filt)
    out = np.zeros(e.shape[:-1] + (O,), dtype=np.int64)
    for t in range(9):
        idx = origin + REACH + j0 + t
        live = t < nt
        assert (idx[live] >= 0).all() and (idx[live] < e.shape[-1]).all(), "a tap more than REACH beyond the crop"
        out += e[..., np.where(live, idx, 0)] * w[:, t]
    return np.moveaxis((out + 2048) >> 12, -1, axis)


def resample_from_e(e, crop, size, filt="cubic"):
    """e (3, H, W) integers, MHC's estimates of the whole frame -> E (3, Ho, Wo) int64, with the contract's bounds asserted."""
    y0, x0, h, w = crop
    assert not (y0 | x0 | h | w) & 1 and y0 + h <= e.shape[1] and x0 + w <= e.shape[2] and min(e.shape[1:]) >= 8
    ho, wo = size
    assert np.abs(e).max() < 1 << 22
    P = np.pad(np.asarray(e, dtype=np.int64), ((0, 0), (REACH, REACH), (REACH, REACH)), mode="reflect")
    t = filter_axis(P, x0, w, wo, filt, 2)   # (3, H + 2 REACH, Wo)
    assert np.abs(t).max() < 1 << 23
    E = filter_axis(t, y0, h, ho, filt, 1)
    assert np.abs(E).max() < 1 << 24
    return E


def resample_estimates(img, crop, size, filt="cubic", black=(0, 0, 0, 0), cfa="rggb"):
    """E (3, Ho, Wo) int64 in units of 1/16.  crop (y0, x0, h, w), all even; size (Ho, Wo)."""
    return resample_from_e(R.mhc_estimates(np.asarray(img), black, cfa), crop, size, filt)


def values(E, white, black=(0, 0, 0, 0), gain=(1, 1, 1), matrix=None, clip=False):
    """The f32 outputs o (3, Ho, Wo): _rgb_ref.rgb_values' colour stage on E with MHC's k = (gain * inv) * (1/16)."""
    k = R.scales("mhc", white, black, gain)
    m = np.eye(3, dtype=np.float32) if matrix is None else np.asarray(matrix, dtype=np.float32).reshape(3, 3)
    v = [E[c].astype(np.float32) * k[c] for c in range(3)]
    o = np.stack([(m[i, 0] * v[0] + m[i, 1] * v[1]) + m[i, 2] * v[2] for i in range(3)]).astype(np.float32)
    if clip:
        o = np.minimum(np.maximum(o, np.float32(0.0)), np.float32(1.0))
    return o


float_bits = A.float_bits
display_from_o = A.display_from_o
yuv_from_o = Y.yuv_from_o


def resample_ref(img, crop, size, dtype, white, filt="cubic", black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1), matrix=None, clip=False):
    return float_bits(values(resample_estimates(img, crop, size, filt, black, cfa), white, black, gain, matrix, clip), dtype)


def resample_display_ref(img, crop, size, white, lut, dtype="u8", layout="hwc", filt="cubic", black=(0, 0, 0, 0), cfa="rggb",
                         gain=(1, 1, 1), matrix=None):
    return display_from_o(values(resample_estimates(img, crop, size, filt, black, cfa), white, black, gain, matrix), lut, dtype, layout)


def resample_yuv_ref(img, crop, size, white, lut, fmt, coef, in_bits, filt="cubic", black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1),
                     matrix=None):
    return yuv_from_o(values(resample_estimates(img, crop, size, filt, black, cfa), white, black, gain, matrix), lut, fmt, coef, in_bits)
