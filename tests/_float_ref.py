"""numpy reference of the normalised float output (mcraw_ctx_set_float_out, include/mcraw_hip.h), bit-exact:
inv[p] = 1.0f / (white - (float)black[p]); v = (float)(sample - black[p]) * inv[p]; clip to [0, 1]; f32 / f16 (RNE) / bf16 (RNE)."""
import numpy as np

CFA = {"rggb": [0, 1, 2, 3], "bggr": [3, 2, 1, 0], "grbg": [1, 0, 3, 2], "gbrg": [2, 3, 0, 1]}


def bf16_bits(v):
    """float32 array -> bfloat16 bit patterns (uint16), rounded to nearest even (finite inputs)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def float_values(img, white, black=(0, 0, 0, 0), clip=False):
    """The f32 values v of a uint16 mosaic (h, w)."""
    img = np.asarray(img, dtype=np.uint16)
    h, w = img.shape
    blk = np.asarray(black, dtype=np.int64)
    p = (np.arange(h)[:, None] & 1) * 2 + (np.arange(w)[None, :] & 1)
    inv = np.float32(1.0) / (np.float32(white) - blk.astype(np.float32))
    d = (img.astype(np.int64) - blk[p]).astype(np.float32)
    v = (d * inv.astype(np.float32)[p]).astype(np.float32)
    if clip:
        v = np.minimum(np.maximum(v, np.float32(0.0)), np.float32(1.0))
    return v


def float_ref(img, dtype, white, layout="planes", black=(0, 0, 0, 0), clip=False, plane=None):
    """The output bytes' values: float32 / float16 arrays, bf16 as uint16 bit patterns.  planes: (4, h/2, w/2)."""
    v = float_values(img, white, black, clip)
    if dtype == "f32":
        o = v
    elif dtype == "f16":
        with np.errstate(over="ignore"):  # (overflow to inf is the contract)
            o = v.astype(np.float16)
    else:
        o = bf16_bits(v)
    if layout == "mosaic":
        return o
    h, w = o.shape
    plane = [0, 1, 2, 3] if plane is None else list(plane)
    res = np.zeros((4, h // 2, w // 2), dtype=o.dtype)
    for p in range(4):
        res[plane[p]] = o[(p >> 1)::2, (p & 1)::2]
    return res


def ref_bytes(img, dtype, white, layout="planes", black=(0, 0, 0, 0), clip=False, plane=None):
    return np.ascontiguousarray(float_ref(img, dtype, white, layout, black, clip, plane)).view(np.uint8).ravel()
