"""CPU: the encoder's C ABI (include/mcraw_hip.h: mcraw_encode_bound7, mcraw_encode_batch, mcraw_encode7) is exported,
its size bound is the exact worst case and needs no device, the encode calls fail without a device (no CPU fallback),
and mcraw_export lists --transcode in its usage line."""
import ctypes
import os
import subprocess

import pytest

import _libs as L
import motioncam_decoder_amd as M
from motioncam_decoder_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORT = os.path.join(ROOT, "motioncam_decoder_amd", "lib", "mcraw_export")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return M.load()


def _bound(w, h):
    encw, ench = (w + 63) // 64 * 64, (h + 3) // 4 * 4
    nblk = encw * ench // 64
    return 16 + 128 * nblk + 2 * (4 + 130 * ((nblk + 63) // 64))


def test_encoder_symbols_exported(lib):
    for name in ("mcraw_encode_bound7", "mcraw_encode_batch", "mcraw_encode7"):
        assert name in M.ABI_SYMBOLS
        assert hasattr(lib, name), name
    assert hasattr(M, "EncFrame") and hasattr(M.Context, "encode_batch") and hasattr(M.Context, "make_enc_frames")
    assert ctypes.sizeof(M.EncFrame) == 40  # in, width, height, out, out_capacity, len_out (LP64)
    raw = open(M.lib_path(), "rb").read()
    for k in (b"k7e_payload", b"k7e_side"):
        assert k in raw, k


def test_bound_formula(lib):
    syn = L.synth()
    sizes = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 127, 128, 129, 200, 1000, 2160, 3024, 3840, 4032, 4320, 7680]
    for w in sizes:
        for h in sizes:
            b = M.encode_bound7(w, h)
            assert b == _bound(w, h), (w, h)
            assert b <= syn.mcraw_synth_bound7(w, h), (w, h)
    for w, h in ((0, 4), (4, 0), (-1, 5), (5, -3)):
        assert M.encode_bound7(w, h) == 0


def test_bound_is_reached_by_noise(lib):
    # a frame of full-range noise codes every block raw-16 and both side streams at their widest records
    import numpy as np
    img = np.random.default_rng(7).integers(0, 65536, size=(8, 128), dtype=np.uint16)
    img[0, 0], img[0, 2] = 0, 65535
    buf = L.encode7(img)
    assert len(buf) <= M.encode_bound7(128, 8)


def test_no_cpu_fallback_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import numpy as np
    img = np.zeros((4, 64), dtype=np.uint16)
    out = np.zeros(M.encode_bound7(64, 4), dtype=np.uint8)
    assert lib.mcraw_encode7(out.ctypes.data, out.size, img.ctypes.data, 64, 4) == 0
    frames = M.Context.make_enc_frames([(img.ctypes.data, 64, 4, out.ctypes.data, out.size)])
    written = (ctypes.c_size_t * 1)()
    status = (ctypes.c_int32 * 1)()
    assert lib.mcraw_encode_batch(None, frames, 1, M.MEM_HOST, None, written, status) < 0
    h = ctypes.c_void_p()
    assert lib.mcraw_ctx_create(0, ctypes.byref(h)) != 0  # no context without a device, hence no batch
    assert not out.any()


def test_export_usage_lists_transcode():
    build.build_hip()
    build.build_host()
    r = subprocess.run([EXPORT], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    usage = (r.stdout + r.stderr).strip().splitlines()[0]
    assert usage.startswith("Usage: mcraw_export") and "--transcode" in usage, usage
