"""Normalised float output (mcraw_ctx_set_float_out) without a GPU: the ABI's symbols, the numpy reference of the value
contract on hand-computed cases, cfa_planes, and the setters' refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _float_ref as R
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float_out_symbols_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    for name in ("mcraw_ctx_set_float_out", "mcraw_pool_set_float_out"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in M.ABI_SYMBOLS
        assert hasattr(M.load(), name)
    for macro, v in (("MCRAW_FLOAT_F32", 1), ("MCRAW_FLOAT_F16", 2), ("MCRAW_FLOAT_BF16", 3), ("MCRAW_LAYOUT_MOSAIC", 0),
                     ("MCRAW_LAYOUT_PLANES", 1), ("MCRAW_FLOAT_CLIP", 1)):
        assert re.search(r"#define %s\s+%du?\b" % (macro, v), hdr), macro


def test_float_out_struct_layout():
    assert C.sizeof(M.FloatOut) == 28
    assert M.FloatOut.white.offset == 20 and M.FloatOut.plane.offset == 24 and M.FloatOut.black.offset == 12


def _one(sample, white, black=0, dtype="f32", clip=False):
    img = np.full((2, 2), sample, dtype=np.uint16)
    return R.float_ref(img, dtype, white, "mosaic", (black,) * 4, clip)[0, 0]


def test_reference_f16_round_to_nearest_even():
    # white 2048: v = sample / 2048 exactly; 2049 / 2048 = 1 + 2^-11 is the tie between 1 and 1 + 2^-10
    assert _one(2049, 2048, dtype="f16").view(np.uint16) == 0x3C00
    assert _one(2051, 2048, dtype="f16").view(np.uint16) == 0x3C02  # 1 + 3 * 2^-11: tie, to the even 1 + 2^-9
    assert _one(2050, 2048, dtype="f16").view(np.uint16) == 0x3C01


def test_reference_bf16_round_to_nearest_even():
    assert _one(257, 256, dtype="bf16") == 0x3F80  # 1 + 2^-8: tie between 1 and 1 + 2^-7
    assert _one(259, 256, dtype="bf16") == 0x3F82  # 1 + 3 * 2^-8: tie, to the even 1 + 2^-6
    assert _one(258, 256, dtype="bf16") == 0x3F81
    assert R.bf16_bits(np.array([1.0, -2.0, 0.0], np.float32)).tolist() == [0x3F80, 0xC000, 0x0000]


def test_reference_f16_overflow_to_inf():
    assert _one(65504, 1, dtype="f16").view(np.uint16) == 0x7BFF
    assert _one(65519, 1, dtype="f16").view(np.uint16) == 0x7BFF
    assert _one(65520, 1, dtype="f16").view(np.uint16) == 0x7C00
    assert np.isinf(_one(65535, 1, dtype="f16"))


def test_reference_negatives_kept_without_clip():
    inv = np.float32(1.0) / np.float32(1000.0)
    assert _one(50, 1100, black=100) == np.float32(-50.0) * inv < 0
    assert _one(50, 1100, black=100, clip=True) == 0.0
    assert _one(5000, 1100, black=100) > 1.0 and _one(5000, 1100, black=100, clip=True) == 1.0
    # one rounding, in the multiply: (s - b) * inv, not s * inv - b * inv
    s, b, w = 4000, 64, 4095.0
    inv = np.float32(1.0) / (np.float32(w) - np.float32(b))
    assert _one(s, w, black=b) == np.float32(s - b) * inv


def test_reference_planes_layout():
    img = np.arange(4 * 6, dtype=np.uint16).reshape(4, 6)
    pl = R.float_ref(img, "f32", 1.0, "planes", plane=M.cfa_planes("gbrg"))
    assert pl.shape == (4, 2, 3)
    # gbrg: position 0 (even row, even col) is G on the B row -> plane 2; position 1 is B -> plane 3; 2 is R -> 0; 3 -> 1
    assert np.array_equal(pl[2], img[0::2, 0::2]) and np.array_equal(pl[3], img[0::2, 1::2])
    assert np.array_equal(pl[0], img[1::2, 0::2]) and np.array_equal(pl[1], img[1::2, 1::2])


@pytest.mark.parametrize("arr,want", [("rggb", [0, 1, 2, 3]), ("bggr", [3, 2, 1, 0]), ("grbg", [1, 0, 3, 2]), ("gbrg", [2, 3, 0, 1]),
                                      ("RGGB", [0, 1, 2, 3])])
def test_cfa_planes(arr, want):
    assert M.cfa_planes(arr) == want


def test_cfa_planes_puts_r_g_g_b_in_order():
    colour = {"r": 0, "b": 3}
    for arr in ("rggb", "bggr", "grbg", "gbrg"):
        pl = M.cfa_planes(arr)
        r_row = arr.index("r") >> 1
        for p, ch in enumerate(arr):
            want = colour.get(ch, 1 if (p >> 1) == r_row else 2)
            assert pl[p] == want, (arr, p)
    with pytest.raises(ValueError):
        M.cfa_planes("rgbw")


def test_float_out_arguments():
    f = M.float_out("bf16", 1023, layout="mosaic", black=(1, 2, 3, 4), clip=True)
    assert (f.dtype, f.layout, f.flags, list(f.black), f.white) == (M.FLOAT_BF16, M.LAYOUT_MOSAIC, M.FLOAT_CLIP, [1, 2, 3, 4], 1023.0)
    assert M.float_out("f32", 1).dtype == M.FLOAT_F32 and M.float_out("f16", 1).layout == M.LAYOUT_PLANES
    with pytest.raises(ValueError):
        M.float_out("f64", 1)
    with pytest.raises(ValueError):
        M.float_out("f16", 1, layout="rows")


def test_setters_reject_null_context_and_pool():
    lib = M.load()
    f = M.float_out("f16", 4095)
    assert lib.mcraw_ctx_set_float_out(None, C.byref(f)) < 0
    assert lib.mcraw_ctx_set_float_out(None, None) < 0
    assert lib.mcraw_pool_set_float_out(None, C.byref(f)) < 0
    assert lib.mcraw_pool_set_float_out(None, None) < 0


def test_no_cpu_fallback_without_device():
    import subprocess
    import sys
    code = ("import motioncam_decoder_amd as M\n"
            "try:\n    M.Context(0)\nexcept M.McrawError as e:\n    print('refused', e)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert "refused" in r.stdout, (r.stdout, r.stderr)
