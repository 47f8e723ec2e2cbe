"""numpy reference of the demosaic to linear RGB (mcraw_demosaic_batch, include/mcraw_hip.h), bit-exact.

Integer stage in int64: d = sample - black[p] (p = (y & 1) * 2 + (x & 1)), reflected 101-style at the frame edges for MHC;
estimates E_c in units of 1/16 (MHC, Malvar-He-Cutler 5x5) or 1/2 (BIN2, one output per 2x2 quad).  Float stage in f32, in
the library's order: k[c] = (gain[c] * inv) * scale, v_c = (float)E_c * k[c], o_i = (m[3i] v_0 + m[3i+1] v_1) + m[3i+2] v_2,
clip to [0, 1], then f32 / f16 (RNE) / bf16 (RNE, _float_ref.bf16_bits)."""
import numpy as np

from _float_ref import bf16_bits

# role of CFA position p in RGGB terms (0 R, 1 G on the R row, 2 G on the B row, 3 B) is p ^ SHIFT[cfa]
SHIFT = {"rggb": 0, "grbg": 1, "gbrg": 2, "bggr": 3}
CFA_CODE = {"rggb": 0, "bggr": 1, "grbg": 2, "gbrg": 3}


def _d(img, black):
    img = np.asarray(img)
    h, w = img.shape
    blk = np.asarray(black, dtype=np.int64)
    p = (np.arange(h)[:, None] & 1) * 2 + (np.arange(w)[None, :] & 1)
    return img.astype(np.int64) - blk[p]


def mhc_estimates(img, black=(0, 0, 0, 0), cfa="rggb"):
    """E (3, h, w) int64, in units of 1/16."""
    d = _d(img, black)
    h, w = d.shape
    P = np.pad(d, 2, mode="reflect")  # -k -> k, h-1+k -> h-1-k: keeps the CFA parity

    def at(dy, dx):
        return P[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]

    C = at(0, 0)
    ax1 = at(-1, 0) + at(1, 0) + at(0, -1) + at(0, 1)
    ax2v, ax2h = at(-2, 0) + at(2, 0), at(0, -2) + at(0, 2)
    diag = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
    native = 16 * C
    g_at_rb = 8 * C + 4 * ax1 - 2 * (ax2v + ax2h)
    horiz = 10 * C + 8 * (at(0, -1) + at(0, 1)) - 2 * ax2h - 2 * diag + ax2v  # wanted colour left / right of C
    vert = 10 * C + 8 * (at(-1, 0) + at(1, 0)) - 2 * ax2v - 2 * diag + ax2h   # ... above / below
    rb_at_br = 12 * C + 4 * diag - 3 * (ax2v + ax2h)
    role = ((np.arange(h)[:, None] & 1) * 2 + (np.arange(w)[None, :] & 1)) ^ SHIFT[cfa]
    E = np.empty((3, h, w), dtype=np.int64)
    pick = {0: (native, g_at_rb, rb_at_br), 3: (rb_at_br, g_at_rb, native),
            1: (horiz, native, vert), 2: (vert, native, horiz)}
    for r, chans in pick.items():
        m = role == r
        for c in range(3):
            E[c][m] = chans[c][m]
    return E


def bin2_estimates(img, black=(0, 0, 0, 0), cfa="rggb"):
    """E (3, h/2, w/2) int64, in units of 1/2."""
    d = _d(img, black)
    q = [d[(p >> 1)::2, (p & 1)::2] for p in range(4)]
    s = SHIFT[cfa]
    return np.stack([2 * q[0 ^ s], q[1 ^ s] + q[2 ^ s], 2 * q[3 ^ s]])


def estimates(img, algo, black=(0, 0, 0, 0), cfa="rggb"):
    return mhc_estimates(img, black, cfa) if algo == "mhc" else bin2_estimates(img, black, cfa)


def scales(algo, white, black, gain):
    """k[c] (f32): inv = 1 / (white - 0.25 * sum(black)), k = (gain * inv) * (1/16 or 1/2)."""
    inv = np.float32(1.0) / (np.float32(white) - np.float32(0.25) * np.float32(int(sum(int(b) for b in black))))
    sc = np.float32(0.0625 if algo == "mhc" else 0.5)
    return np.array([(np.float32(g) * inv) * sc for g in np.asarray(gain, dtype=np.float32)], dtype=np.float32)


def rgb_values(img, algo, white, black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1), matrix=None, clip=False):
    """The f32 outputs o (3, ho, wo) before the dtype conversion."""
    E = estimates(img, algo, black, cfa)
    k = scales(algo, white, black, gain)
    m = np.eye(3, dtype=np.float32) if matrix is None else np.asarray(matrix, dtype=np.float32).reshape(3, 3)
    v = [E[c].astype(np.float32) * k[c] for c in range(3)]
    o = np.stack([(m[i, 0] * v[0] + m[i, 1] * v[1]) + m[i, 2] * v[2] for i in range(3)]).astype(np.float32)
    if clip:
        o = np.minimum(np.maximum(o, np.float32(0.0)), np.float32(1.0))
    return o


def rgb_ref(img, algo, dtype, white, black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1), matrix=None, clip=False):
    """(3, ho, wo): float32 / float16 arrays, bf16 as uint16 bit patterns."""
    o = rgb_values(img, algo, white, black, cfa, gain, matrix, clip)
    if dtype == "f32":
        return o
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return o.astype(np.float16)
    return bf16_bits(o)


def ref_bits(img, algo, dtype, white, **kw):
    """The output's bit patterns as an unsigned integer array (uint32 for f32, uint16 otherwise)."""
    o = np.ascontiguousarray(rgb_ref(img, algo, dtype, white, **kw))
    return o.view(np.uint32) if dtype == "f32" else o.view(np.uint16)
