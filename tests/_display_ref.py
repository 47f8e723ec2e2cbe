"""numpy reference of the display stage (mcraw_demosaic_display_batch, include/mcraw_hip.h), bit-exact.

On top of _rgb_ref.rgb_values (the f32 outputs o, no clip): c = o > 0 ? min(o, 1) : 0 (NaN -> 0), i = rint(c * (L - 1))
with the product rounded to float32 and rint half-to-even, out = lut[i] (its low byte for uint8).  Layout "chw" gives
(3, ho, wo), "hwc" (ho, wo, 3)."""
import numpy as np

from _rgb_ref import rgb_values


def lut_index(o, L):
    """Indices (uint32) of the f32 outputs o into a LUT of L entries."""
    o = np.asarray(o, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(o > np.float32(0.0), np.minimum(o, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    prod = (c * np.float32(L - 1)).astype(np.float32)
    return np.rint(prod).astype(np.uint32)


def apply_lut(o, lut, dtype="u8"):
    lut = np.asarray(lut, dtype=np.uint16)
    q = lut[lut_index(o, len(lut))]
    return (q & 0xFF).astype(np.uint8) if dtype == "u8" else q


def display_ref(img, algo, white, lut, dtype="u8", layout="hwc", black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1),
                matrix=None):
    """The output of one frame: uint8 / uint16, (ho, wo, 3) for "hwc" or (3, ho, wo) for "chw"."""
    o = rgb_values(img, algo, white, black, cfa, gain, matrix, clip=False)
    q = apply_lut(o, lut, dtype)
    return np.ascontiguousarray(q.transpose(1, 2, 0)) if layout == "hwc" else q
