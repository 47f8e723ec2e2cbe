"""Demosaic to planar linear RGB (mcraw_demosaic_batch, Context.demosaic / decode_rgb) on the GPU: every output bit pattern
equals the numpy reference (_rgb_ref), nothing outside the output is written, the input is left as it was, rejected
calls write nothing, and per-frame colours stay with their batch."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _libs as L
import _rgb_ref as R
import motioncam_decoder_amd as M
from _demosaic_gpu import CFAS, DEV, GUARD, SENT, SRGBISH, raw_call, rgb_params
from _demosaic_gpu import frames as _frames, mosaic as _mosaic, rgb_color as _color

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16", "bf16")
TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ES = {"f32": 4, "f16": 2, "bf16": 2}


def _bits(t, dtype):
    a = t.detach().cpu()
    if dtype == "bf16":
        return a.view(torch.int16).numpy().view(np.uint16)
    return a.numpy().view(np.uint32 if dtype == "f32" else np.uint16)


def _raw_call(ctx, prm, *args, **kw):
    return raw_call(ctx, "mcraw_demosaic_batch", prm, None, *args, staged=False, **kw)


def _params(algo="mhc", dtype="f16", white=4095.0, black=(0, 0, 0, 0), cfa="rggb", clip=False):
    return rgb_params(algo, white, black, cfa, {"f32": 1, "f16": 2, "bf16": 3}[dtype], 1 if clip else 0)


def _ref(img, algo, dtype, white, black, cfa, gain, matrix, clip):
    return R.ref_bits(img, algo, dtype, white, black=black, cfa=cfa, gain=gain, matrix=matrix, clip=clip)


@pytest.mark.parametrize("clip", (False, True))
@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("algo", ("mhc", "bin2"))
def test_demosaic_matches_reference(gpu_ctx, algo, dtype, cfa, clip):
    rng = np.random.default_rng(zlib.crc32(("%s%s%s%d" % (algo, dtype, cfa, clip)).encode()))
    for (w, h, nbits) in ((66, 18, 10), (64, 16, 12), (40, 12, 14), (24, 8, 16)):
        white = float((1 << nbits) - 1)
        black = tuple(int(b) for b in rng.integers(0, 1 << (nbits - 4), size=4))
        imgs = [_mosaic(rng, h, w, nbits) for _ in range(2)]
        gain = (1.8, 1.0, 1.3)
        t = torch.from_numpy(np.stack(imgs)).to(DEV)
        out = gpu_ctx.demosaic(t, algo=algo, dtype=TD[dtype], white=white, black=black, cfa=cfa, gain=gain, matrix=SRGBISH,
                               clip=clip)
        torch.cuda.synchronize()
        for i in range(2):
            want = _ref(imgs[i], algo, dtype, white, black, cfa, gain, SRGBISH, clip)
            assert np.array_equal(_bits(out[i], dtype), want), (w, h, nbits, i)


@pytest.mark.parametrize("w,h", [(4, 4), (6, 4), (64, 16), (66, 18), (1002, 750), (8, 1000), (3840, 2160)])
def test_demosaic_sizes(gpu_ctx, w, h):
    rng = np.random.default_rng(w * 7 + h)
    img = _mosaic(rng, h, w, 12)
    t = torch.from_numpy(img).to(DEV)
    for algo, dtype, cfa in (("mhc", "f16", "rggb"), ("mhc", "f32", "gbrg"), ("bin2", "bf16", "grbg")):
        out = gpu_ctx.demosaic(t, algo=algo, dtype=dtype, white=4095.0, black=(64, 65, 66, 67), cfa=cfa, gain=(2.0, 1.0, 1.5),
                               matrix=SRGBISH)
        torch.cuda.synchronize()
        ho, wo = (h, w) if algo == "mhc" else (h // 2, w // 2)
        assert tuple(out.shape) == (3, ho, wo)
        want = _ref(img, algo, dtype, 4095.0, (64, 65, 66, 67), cfa, (2.0, 1.0, 1.5), SRGBISH, False)
        assert np.array_equal(_bits(out, dtype), want), (algo, dtype, w, h)


@pytest.mark.parametrize("algo", ("mhc", "bin2"))
def test_strided_input_per_frame_colours_sentinels(gpu_ctx, algo):
    rng = np.random.default_rng(11)
    n, h, w, pitch, fstride = 3, 34, 70, 83, 34 * 83 + 29
    imgs = [_mosaic(rng, h, w, 14) for _ in range(n)]
    # (int16 storage: torch has few CUDA kernels for uint16, the library reads the bits)
    base = torch.from_numpy(rng.integers(0, 1 << 16, size=n * fstride + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    v16 = torch.as_strided(base, (n, h, w), (fstride, pitch, 1), 5)  # 5: odd element offset, not 16-byte aligned
    for i in range(n):
        v16[i].copy_(torch.from_numpy(imgs[i].view(np.int16)).to(DEV))
    view = v16.view(torch.uint16)
    before = base.clone()
    gains = np.array([[2.0, 1.0, 1.5], [1.2, 1.0, 2.2], [1.0, 1.0, 1.0]], np.float32)
    mats = np.stack([SRGBISH, np.eye(3, dtype=np.float32), SRGBISH[::-1].copy()])
    for dtype in DTYPES:
        ho, wo = (h, w) if algo == "mhc" else (h // 2, w // 2)
        nbytes = n * 3 * ho * wo * ES[dtype]
        for misalign in (0, ES[dtype]):  # element-aligned but (for the second) not 16-byte aligned
            buf = torch.full((GUARD + misalign + nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
            out = buf[GUARD + misalign: GUARD + misalign + nbytes].view(TD[dtype]).view(n, 3, ho, wo)
            for per in (True, False):
                gpu_ctx.demosaic(view, algo=algo, dtype=dtype, white=16383.0, black=(512, 500, 510, 520), cfa="bggr",
                                 gain=gains if per else gains[0], matrix=mats if per else mats[0], out=out)
                torch.cuda.synchronize()
                a = buf.cpu().numpy()
                assert (a[:GUARD + misalign] == SENT).all() and (a[GUARD + misalign + nbytes:] == SENT).all()
                for i in range(n):
                    k = i if per else 0
                    want = _ref(imgs[i], algo, dtype, 16383.0, (512, 500, 510, 520), "bggr", gains[k], mats[k], False)
                    assert np.array_equal(_bits(out[i], dtype), want), (dtype, misalign, per, i)
    assert torch.equal(base, before), "the input was written"


def test_rejections_write_nothing(gpu_ctx):
    w, h, n = 16, 8, 2
    img = torch.zeros((n, h, w), dtype=torch.int16, device=DEV).view(torch.uint16)
    nbytes = n * 3 * h * w * 2
    buf = torch.full((nbytes + 8,), SENT, dtype=torch.uint8, device=DEV)
    ip, op = img.data_ptr(), buf.data_ptr()
    ok = _color()
    nan = _color(gain=(float("nan"), 1, 1))
    infm = _color(m=[1, 0, 0, 0, float("inf"), 0, 0, 0, 1])
    cases = [
        (_params(), [ok], 1, ip, w, h * w, 15, h, n, op, nbytes),           # odd width
        (_params(), [ok], 1, ip, w, h * w, w, 7, n, op, nbytes),            # odd height
        (_params(), [ok], 1, ip, w, h * w, 2, h, n, op, nbytes),            # width below 4
        (_params(), [ok], 1, ip, w, h * w, w, 2, n, op, nbytes),            # height below 4
        (_params(), [ok], 1, ip, w - 2, h * w, w, h, n, op, nbytes),        # pitch < width
        (_params(), [ok], 1, ip, w, h * w - w, w, h, n, op, nbytes),        # frame stride too small
        (_params(algo="mhc"), [ok], 1, ip, w, h * w, w, h, n, op, nbytes - 1),  # out too small
        (_params(), [ok], 1, ip, w, h * w, w, h, n, op + 1, nbytes),        # out not element aligned
        (_params(), [ok, ok, ok], 3, ip, w, h * w, w, h, n, op, nbytes),    # ncolors not 1 or n
        (_params(), [ok], 0, ip, w, h * w, w, h, n, op, nbytes),
        (_params(), [nan], 1, ip, w, h * w, w, h, n, op, nbytes),           # non-finite gain
        (_params(), [ok, infm], 2, ip, w, h * w, w, h, n, op, nbytes),      # non-finite matrix entry
        (_params(white=float("inf")), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),
        (_params(white=100.0, black=(100, 100, 100, 100)), [ok], 1, ip, w, h * w, w, h, n, op, nbytes),
        (None, [ok], 1, ip, w, h * w, w, h, n, op, nbytes),
    ]
    for bad in ("algo", "dtype", "cfa", "flags"):
        p = _params()
        setattr(p, bad, {"algo": 3, "dtype": 4, "cfa": 4, "flags": 2}[bad])
        cases.append((p, [ok], 1, ip, w, h * w, w, h, n, op, nbytes))
    serial = gpu_ctx.last_serial()
    for i, c in enumerate(cases):
        rc = _raw_call(gpu_ctx, *c)
        assert rc < 0, i
        assert M.load().mcraw_last_error().decode().startswith("mcraw_demosaic_batch"), i
    assert _raw_call(gpu_ctx, _params(), [ok], 1, ip, w, h * w, w, h, 0, op, 0) == 0  # n == 0: a no-op
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert (buf.cpu().numpy() == SENT).all()
    assert gpu_ctx.last_serial() == serial
    # the good call next to them does write
    assert _raw_call(gpu_ctx, _params(), [ok], 1, ip, w, h * w, w, h, n, op, nbytes) == 0
    torch.cuda.synchronize()  # (the context's own stream: a device-wide wait)
    assert (buf.cpu().numpy()[:nbytes] == 0).all()


@pytest.mark.parametrize("two_streams", (False, True))
def test_queued_batches_keep_their_colours(gpu_ctx, two_streams):
    rng = np.random.default_rng(5)
    n, h, w = 4, 64, 256
    imgs = [_mosaic(rng, h, w, 12) for _ in range(n)]
    t = torch.from_numpy(np.stack(imgs)).to(DEV)
    s1 = torch.cuda.Stream(DEV)
    s2 = torch.cuda.Stream(DEV) if two_streams else s1
    sets = []
    for b in range(6):
        g = rng.uniform(0.5, 2.5, size=(n, 3)).astype(np.float32)
        m = (SRGBISH[None] * rng.uniform(0.5, 1.5, size=(n, 3, 3))).astype(np.float32)
        sets.append((g, m))
    outs = []
    torch.cuda.synchronize()
    for b, (g, m) in enumerate(sets):  # queued back to back, no host sync between them
        with torch.cuda.stream(s1 if b % 2 == 0 else s2):
            outs.append(gpu_ctx.demosaic(t, algo="mhc", dtype="f32", white=4095.0, gain=g, matrix=m))
    torch.cuda.synchronize()
    for (g, m), o in zip(sets, outs):
        for i in range(n):
            want = _ref(imgs[i], "mhc", "f32", 4095.0, (0, 0, 0, 0), "rggb", g[i], m[i], False)
            assert np.array_equal(_bits(o[i], "f32"), want)


@pytest.mark.parametrize("typ", (7, 6))
def test_decode_rgb_matches_reference_of_oracle(gpu_ctx, typ):
    rng = np.random.default_rng(typ)
    w, h = 512, 96
    items = _frames(rng, [(w, h)] * 3, typ)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    black, cfa, gain = (64, 64, 64, 64), "grbg", (1.9, 1.0, 1.4)
    for algo, dtype in (("mhc", "f16"), ("bin2", "f32"), ("mhc", "bf16")):
        out = gpu_ctx.decode_rgb(ins, w, h, typ, algo=algo, dtype=dtype, white=4095.0, black=black, cfa=cfa, gain=gain,
                                 matrix=SRGBISH, clip=True)
        torch.cuda.synchronize()
        for i, (_, want) in enumerate(items):
            assert np.array_equal(_bits(out[i], dtype), _ref(want, algo, dtype, 4095.0, black, cfa, gain, SRGBISH, True))


def test_decode_rgb_golden_vectors(gpu_ctx, golden):
    done = 0
    for name, g in sorted(golden.items()):
        w, h = g["w"], g["h"]
        if g["ret"] != w * h or w < 4 or h < 4 or w % 2 or h % 2:
            continue
        want = g["out"].reshape(h, w)
        t = torch.from_numpy(np.ascontiguousarray(g["buf"])).to(DEV)
        out = gpu_ctx.decode_rgb([t], w, h, g["type"], algo="mhc", dtype="f32", white=65535.0, gain=(1.5, 1.0, 1.2))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out[0], "f32"), _ref(want, "mhc", "f32", 65535.0, (0,) * 4, "rggb", (1.5, 1.0, 1.2), None,
                                                         False)), name
        done += 1
    assert done > 0


def test_decode_rgb_on_side_stream_and_unchecked(gpu_ctx):
    rng = np.random.default_rng(9)
    w, h = 256, 64
    items = _frames(rng, [(w, h)] * 2, 7)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = gpu_ctx.decode_rgb(ins, w, h, 7, algo="mhc", dtype="f32", white=4095.0, check=False)
        doubled = out * 2  # a torch op queued behind it on the same stream
    s.synchronize()
    for i, (_, want) in enumerate(items):
        ref = R.rgb_values(want, "mhc", 4095.0)
        assert np.array_equal(_bits(out[i], "f32"), ref.view(np.uint32))
        assert np.array_equal(doubled[i].cpu().numpy(), ref * np.float32(2))
    # the default (null) stream: the library runs on a side stream the current one waits for
    out2 = gpu_ctx.decode_rgb(ins, w, h, 7, algo="bin2", dtype="f16", white=4095.0, check=False)
    total = out2.float().sum()
    torch.cuda.synchronize()
    want = np.stack([R.rgb_ref(x, "bin2", "f16", 4095.0) for _, x in items])
    assert np.array_equal(out2.cpu().numpy().view(np.uint16), want.view(np.uint16))
    assert float(total) == float(torch.from_numpy(want).to(DEV).float().sum())


def test_decode_rgb_truncated_frame_raises(gpu_ctx):
    rng = np.random.default_rng(4)
    w, h = 256, 64
    items = _frames(rng, [(w, h)] * 3, 7)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    ins[1] = ins[1][: ins[1].numel() // 2].clone()
    with pytest.raises(M.McrawError, match="frame 1"):
        gpu_ctx.decode_rgb(ins, w, h, 7, dtype="f16", white=4095.0)


def test_stage_and_serial_left_alone(gpu_ctx):
    rng = np.random.default_rng(8)
    w, h = 128, 32
    items = _frames(rng, [(w, h)], 7)
    t = torch.from_numpy(items[0][0]).to(DEV)
    mos = torch.from_numpy(items[0][1]).to(DEV)
    gpu_ctx.set_float_out("f32", 4095.0, layout="mosaic", black=(64,) * 4)
    try:
        serial = gpu_ctx.last_serial()
        gpu_ctx.demosaic(mos, dtype="f16", white=4095.0)
        torch.cuda.synchronize()
        assert gpu_ctx.last_serial() == serial
        gpu_ctx.decode_rgb([t], w, h, 7, dtype="f16", white=4095.0)
        # the float stage still governs the next plain batch
        out = torch.full((w * h * 4,), SENT, dtype=torch.uint8, device=DEV)
        written, status = gpu_ctx.decode_batch(M.Context.make_frames([(t.data_ptr(), t.numel(), w, h, 7, out.data_ptr(), w * h * 2)]))
        assert status == [0]
        import _float_ref as FR
        want = FR.ref_bytes(items[0][1], "f32", 4095.0, "mosaic", (64,) * 4)
        assert np.array_equal(out.cpu().numpy(), want)
    finally:
        gpu_ctx.set_post()


def test_uhd_batch_profiled(gpu_ctx):
    rng = np.random.default_rng(16)
    n, h, w = 16, 2160, 3840
    distinct = [_mosaic(rng, h, w, 12) for _ in range(2)]
    t = torch.from_numpy(np.stack([distinct[i % 2] for i in range(n)])).to(DEV)
    gpu_ctx.profile(only=["krgb_mhc"])
    gpu_ctx.kernel_ms("krgb_mhc", reset=True)
    out = gpu_ctx.demosaic(t, algo="mhc", dtype="f16", white=4095.0, black=(64,) * 4, gain=(2.0, 1.0, 1.6), matrix=SRGBISH)
    torch.cuda.synchronize()
    ms, launches = gpu_ctx.kernel_ms("krgb_mhc", reset=True)
    gpu_ctx.profile(enable=False)
    assert launches == 1 and ms > 0
    for i in (0, 1, n - 1):
        want = _ref(distinct[i % 2], "mhc", "f16", 4095.0, (64,) * 4, "rggb", (2.0, 1.0, 1.6), SRGBISH, False)
        assert np.array_equal(_bits(out[i], "f16"), want), i
