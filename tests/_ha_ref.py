"""numpy statement of the edge-directed demosaic (MCRAW_RGB_HA, include/mcraw_hip.h), bit-exact: Hamilton-Adams adaptive
colour-plane interpolation in integers.

d = sample - black[p], reflected 101-style by 3 samples.  The green plane g, in 1/8 DN, on the frame and a ring of one pixel
(computed from the reflected d): 8 d at a green site; at an R or B site the horizontal or the vertical estimate, whichever has
the smaller gradient, or their mean.  The estimates E_c, in 1/32 DN: E_G = 4 g, the native channel 32 d, R and B from the colour
differences against g along the axis that carries the colour (green sites) or along the flatter diagonal (R at B, B at R).
From E_c on the float, display and YUV stages are MHC's (_rgb_ref, _display_ref, _yuv_ref) with the scale 1/32."""
import numpy as np

import _rgb_ref as R
from _float_ref import bf16_bits

REACH = 3  # samples that a read may leave the frame by
SCALE = 0.03125


def _roles(h, w, cfa, y0=0, x0=0):
    """RGGB role of every position of rows y0 .. y0 + h - 1 and columns x0 .. x0 + w - 1 (negative coordinates keep the parity)."""
    return (((np.arange(y0, y0 + h)[:, None] & 1) * 2 + (np.arange(x0, x0 + w)[None, :] & 1)) ^ R.SHIFT[cfa])


def _pick(a, Da, b, Db):
    """2 a where Da < Db, 2 b where Db < Da, a + b where they are equal; and which it was (0, 1, 2)."""
    way = np.where(Da < Db, 0, np.where(Db < Da, 1, 2))
    return np.where(way == 0, 2 * a, np.where(way == 1, 2 * b, a + b)), way


def green_plane(img, black=(0, 0, 0, 0), cfa="rggb"):
    """(g, way, P): g (h + 2, w + 2) int64 in 1/8 DN, the frame and its ring of one; way (h + 2, w + 2): the outcome of the choice
    at the R / B sites (0 horizontal, 1 vertical, 2 tie), -1 at the green sites; P: d padded by REACH."""
    d = R._d(img, black)
    h, w = d.shape
    P = np.pad(d, REACH, mode="reflect")

    def at(dy, dx):  # d at (y + dy, x + dx) for y = -1 .. h, x = -1 .. w
        return P[REACH - 1 + dy:REACH + 1 + dy + h, REACH - 1 + dx:REACH + 1 + dx + w]

    C = at(0, 0)
    ch = 2 * C - at(0, -2) - at(0, 2)
    cv = 2 * C - at(-2, 0) - at(2, 0)
    gh = 2 * (at(0, -1) + at(0, 1)) + ch
    gv = 2 * (at(-1, 0) + at(1, 0)) + cv
    DH = np.abs(at(0, -1) - at(0, 1)) + np.abs(ch)
    DV = np.abs(at(-1, 0) - at(1, 0)) + np.abs(cv)
    grb, way = _pick(gh, DH, gv, DV)
    role = _roles(h + 2, w + 2, cfa, -1, -1)
    rb = (role == 0) | (role == 3)
    return np.where(rb, grb, 8 * C), np.where(rb, way, -1), P


def ha_detail(img, black=(0, 0, 0, 0), cfa="rggb"):
    """(E, gway, dway): E (3, h, w) int64 in 1/32 DN; gway (h, w): the green choice at the R / B sites of the frame (0, 1, 2; -1 at
    green sites); dway (h, w): the diagonal choice there (0: nw-se, 1: ne-sw, 2: tie; -1 at green sites)."""
    g, gway, P = green_plane(img, black, cfa)
    h, w = np.asarray(img).shape

    def dat(dy, dx):
        return P[REACH + dy:REACH + dy + h, REACH + dx:REACH + dx + w]

    def gat(dy, dx):
        return g[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    G = gat(0, 0)

    def pair(a, b):
        c = 2 * G - gat(*a) - gat(*b)
        return 8 * (dat(*a) + dat(*b)) + c, 8 * np.abs(dat(*a) - dat(*b)) + np.abs(c)

    horiz = 2 * pair((0, -1), (0, 1))[0]
    vert = 2 * pair((-1, 0), (1, 0))[0]
    nN, DN = pair((-1, -1), (1, 1))
    nP, DP = pair((-1, 1), (1, -1))
    diag, dway = _pick(nN, DN, nP, DP)
    native = 32 * dat(0, 0)
    role = _roles(h, w, cfa)
    E = np.empty((3, h, w), dtype=np.int64)
    pick = {0: (native, 4 * G, diag), 3: (diag, 4 * G, native), 1: (horiz, native, vert), 2: (vert, native, horiz)}
    for r, chans in pick.items():
        m = role == r
        for c in range(3):
            E[c][m] = chans[c][m]
    rb = (role == 0) | (role == 3)
    return E, gway[1:-1, 1:-1], np.where(rb, dway, -1)


def ha_estimates(img, black=(0, 0, 0, 0), cfa="rggb"):
    """E (3, h, w) int64, in units of 1/32."""
    return ha_detail(img, black, cfa)[0]


def ways(img, black=(0, 0, 0, 0), cfa="rggb"):
    """How often each outcome of the green choice and of the diagonal choice occurs at the frame's R / B sites: two lists of three."""
    _, gw, dw = ha_detail(img, black, cfa)
    return [int((gw == k).sum()) for k in range(3)], [int((dw == k).sum()) for k in range(3)]


def scales(white, black, gain):
    """k[c] (f32): inv = 1 / (white - 0.25 * sum(black)), k = (gain * inv) * (1/32)."""
    inv = np.float32(1.0) / (np.float32(white) - np.float32(0.25) * np.float32(int(sum(int(b) for b in black))))
    return np.array([(np.float32(g) * inv) * np.float32(SCALE) for g in np.asarray(gain, dtype=np.float32)], dtype=np.float32)


def values_from_e(E, white, black=(0, 0, 0, 0), gain=(1, 1, 1), matrix=None, clip=False):
    """MHC's colour stage on E: the f32 outputs o (3, h, w) before the dtype conversion."""
    k = scales(white, black, gain)
    m = np.eye(3, dtype=np.float32) if matrix is None else np.asarray(matrix, dtype=np.float32).reshape(3, 3)
    v = [E[c].astype(np.float32) * k[c] for c in range(3)]
    o = np.stack([(m[i, 0] * v[0] + m[i, 1] * v[1]) + m[i, 2] * v[2] for i in range(3)]).astype(np.float32)
    if clip:
        o = np.minimum(np.maximum(o, np.float32(0.0)), np.float32(1.0))
    return o


def rgb_values(img, white, black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1), matrix=None, clip=False):
    return values_from_e(ha_estimates(img, black, cfa), white, black, gain, matrix, clip)


def ref_bits(img, dtype, white, **kw):
    """The float family's output as bit patterns (uint32 for f32, uint16 otherwise), (3, h, w)."""
    o = rgb_values(img, white, **kw)
    if dtype == "f32":
        return np.ascontiguousarray(o).view(np.uint32)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(o.astype(np.float16)).view(np.uint16)
    return bf16_bits(o).view(np.uint16)


def display_ref(img, white, lut, dtype="u8", layout="hwc", **kw):
    """The display family's output of one frame: (h, w, 3) for "hwc", (3, h, w) for "chw"."""
    from _display_ref import apply_lut
    q = apply_lut(rgb_values(img, white, **kw), lut, dtype)
    return np.ascontiguousarray(q.transpose(1, 2, 0)) if layout == "hwc" else q


def yuv_ref(img, white, lut, fmt, coef, in_bits, **kw):
    """The YUV family's output of one frame: (h * 3 // 2, w)."""
    from _yuv_ref import yuv_from_o
    return yuv_from_o(rgb_values(img, white, **kw), lut, fmt, coef, in_bits)
