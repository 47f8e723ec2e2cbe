"""Normalised float output (mcraw_ctx_set_float_out / decode_tensor) on the GPU: every output byte equals the numpy
reference (_float_ref) applied to the oracle's uint16 decode, and nothing outside the output is written."""
import ctypes as C

import numpy as np
import pytest
import torch

import _float_ref as R
import _libs as L
import motioncam_decoder_amd as M

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16", "bf16")
ES = {"f32": 4, "f16": 2, "bf16": 2}
SENT = 0xA5


def _items(shapes, seed, types=(7, 6)):
    rng = np.random.default_rng(seed)
    items = []
    for (w, h, nbits) in shapes:
        img = rng.integers(0, 1 << nbits, size=(h, w), dtype=np.uint16)
        img[: max(1, h // 3), : max(1, w // 2)] = 70  # a flat corner: empty blocks / 2-byte records
        for t in types:
            buf = L.encode7(img) if t == 7 else L.encode6(img)
            ret, want = (L.oracle_decode7 if t == 7 else L.oracle_decode6)(buf, w, h)
            assert ret == w * h
            items.append((t, w, h, buf, want))
    return items


def _need(w, h, dtype, layout):
    return (w // 2) * (h // 2) * 4 * ES[dtype] if layout == "planes" else w * h * ES[dtype]


def _run(ctx, items, dtype, layout, white, black=(0, 0, 0, 0), clip=False, plane=None, mem=M.MEM_DEVICE, misalign=0,
         cap16=None, pool=None, ticket=False):
    """Decode `items` with the float stage; returns [(status, written, output bytes)] and checks the sentinels."""
    dev = torch.device("cuda:0")
    (pool or ctx).set_float_out(dtype, white, layout=layout, black=black, clip=clip, plane=plane)
    try:
        keep, descs, outs = [], [], []
        for i, (typ, w, h, buf, want) in enumerate(items):
            need = _need(w, h, dtype, layout)
            cap = cap16 if cap16 is not None else need // 2
            total = need + misalign + 64
            if mem == M.MEM_DEVICE:
                pdev = torch.device("cuda", pool.devices()[i % pool.size]) if pool else dev
                t_in = torch.from_numpy(np.ascontiguousarray(buf)).to(pdev)
                t_out = torch.full((total,), SENT, dtype=torch.uint8, device=pdev)
                keep += [t_in, t_out]
                descs.append((t_in.data_ptr(), t_in.numel(), w, h, typ, t_out.data_ptr() + misalign, cap))
            else:
                a_in = np.ascontiguousarray(buf)
                t_out = np.full(total, SENT, dtype=np.uint8)
                keep.append(a_in)
                descs.append((a_in.ctypes.data, a_in.size, w, h, typ, t_out.ctypes.data + misalign, cap))
            outs.append(t_out)
        for d in range(torch.cuda.device_count() if pool else 1):
            torch.cuda.synchronize(d)
        frames = M.Context.make_frames(descs)
        if pool and mem == M.MEM_DEVICE:
            written, status = pool.decode_batch_device(frames)
        elif pool:
            written, status = pool.wait(pool.decode_batch_async(frames)) if ticket else pool.decode_batch(frames)
        elif ticket:
            written, status = ctx.wait(ctx.decode_batch_async(frames))
        else:
            written, status = ctx.decode_batch(frames, mem=mem)
        res = []
        for (typ, w, h, buf, want), o, wr, st in zip(items, outs, written, status):
            a = o.cpu().numpy() if isinstance(o, torch.Tensor) else o
            need = _need(w, h, dtype, layout)
            assert (a[:misalign] == SENT).all(), "wrote in front of the output"
            assert (a[misalign + need:] == SENT).all(), "wrote behind the output"
            res.append((st, wr, a[misalign: misalign + need]))
        return res
    finally:
        (pool or ctx).set_post()


def _check(items, got, dtype, layout, white, black=(0, 0, 0, 0), clip=False, plane=None):
    for (typ, w, h, buf, want), (st, wr, b) in zip(items, got):
        assert st == 0 and wr == w * h, (typ, w, h, st, wr)
        ref = R.ref_bytes(want, dtype, white, layout, black, clip, plane)
        if not np.array_equal(b, ref):
            bad = np.flatnonzero(b != ref)
            pytest.fail("type %d %dx%d %s %s clip=%s: %d bytes differ, first at %d" % (typ, w, h, dtype, layout, clip, bad.size, bad[0]))


# widths not a multiple of 8, heights not a multiple of 4; both codecs in ONE batch (mixed type-6 / type-7)
SHAPES_EVEN = [(256, 16, 12), (1000, 38, 12), (66, 6, 14), (1922, 10, 16), (4032, 24, 12)]
SHAPES_ODD = [(1001, 9, 10), (77, 7, 16), (63, 5, 12)]  # odd widths and heights: the mosaic layout only


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("layout", ["planes", "mosaic"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_float_out_matches_reference(gpu_ctx, dtype, layout, clip):
    shapes = SHAPES_EVEN + (SHAPES_ODD if layout == "mosaic" else [])
    items = _items(shapes, 21)
    black, white = (60, 64, 68, 1000), 4095.0
    plane = M.cfa_planes("grbg")
    got = _run(gpu_ctx, items, dtype, layout, white, black, clip, plane)
    _check(items, got, dtype, layout, white, black, clip, plane)


def test_float_out_f16_overflow_and_negatives(gpu_ctx):
    img = np.random.default_rng(22).integers(0, 1 << 16, size=(8, 128), dtype=np.uint16)
    img[1, :32] = np.arange(65504, 65536)  # 65520 and more: +inf
    img[2, :8] = 0
    items = []
    for t, enc, dec in ((7, L.encode7, L.oracle_decode7), (6, L.encode6, L.oracle_decode6)):
        buf = enc(img)
        items.append((t, 128, 8, buf, dec(buf, 128, 8)[1]))
    got = _run(gpu_ctx, items, "f16", "mosaic", 1.0)
    _check(items, got, "f16", "mosaic", 1.0)
    assert np.isinf(got[0][2].view(np.float16)).any()
    got = _run(gpu_ctx, items, "f16", "mosaic", 2.0, (1, 1, 1, 1))
    _check(items, got, "f16", "mosaic", 2.0, (1, 1, 1, 1))


def test_float_out_golden_vectors(gpu_ctx, golden):
    n = 0
    for name, g in sorted(golden.items()):
        w, h = g["w"], g["h"]
        if g["ret"] != w * h or w <= 0 or h <= 0:
            continue
        want = np.asarray(g["out"]).reshape(-1)[: w * h].view(np.uint16).reshape(h, w) if g["out"].dtype != np.uint16 else g["out"].reshape(h, w)
        items = [(g["type"], w, h, g["buf"], want)]
        layout = "planes" if (w % 2 == 0 and h % 2 == 0) else "mosaic"
        for dtype in DTYPES:
            got = _run(gpu_ctx, items, dtype, layout, 1023.0, (16, 32, 48, 64), False, M.cfa_planes("bggr"))
            _check(items, got, dtype, layout, 1023.0, (16, 32, 48, 64), False, M.cfa_planes("bggr"))
        n += 1
    assert n > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["planes", "mosaic"])
def test_float_out_off_the_16_byte_grid(gpu_ctx, dtype, layout):
    items = _items([(256, 16, 12), (1000, 38, 12)], 23)
    mis = ES[dtype]
    got = _run(gpu_ctx, items, dtype, layout, 4095.0, (64,) * 4, misalign=mis)
    _check(items, got, dtype, layout, 4095.0, (64,) * 4)


def test_float_out_f32_at_odd_2_byte_offset_is_args(gpu_ctx):
    items = _items([(256, 16, 12)], 24)
    for layout in ("planes", "mosaic"):
        got = _run(gpu_ctx, items, "f32", layout, 4095.0, misalign=2)
        for st, wr, b in got:
            assert st == M.E_ARGS and wr == 0
            assert (b == SENT).all(), "nothing may be written"


@pytest.mark.parametrize("mem", [M.MEM_DEVICE, M.MEM_HOST])
def test_float_out_planes_odd_width_is_args(gpu_ctx, mem):
    items = _items([(255, 16, 12), (256, 15, 12)], 25)
    got = _run(gpu_ctx, items, "f16", "planes", 4095.0, cap16=256 * 16, mem=mem)
    for st, wr, b in got:
        assert st == M.E_ARGS and wr == 0
        assert (b == SENT).all()


@pytest.mark.parametrize("mem", [M.MEM_DEVICE, M.MEM_HOST])
def test_float_out_f32_capacity_in_uint16_units(gpu_ctx, mem):
    items = _items([(256, 16, 12)], 26)
    w, h = 256, 16
    for layout in ("planes", "mosaic"):
        got = _run(gpu_ctx, items, "f32", layout, 4095.0, cap16=w * h, mem=mem)  # a uint16-sized capacity
        for st, wr, b in got:
            assert st == M.E_CAPACITY and wr == 0
            assert (b == SENT).all()
        got = _run(gpu_ctx, items, "f32", layout, 4095.0, cap16=2 * w * h, mem=mem)
        _check(items, got, "f32", layout, 4095.0)


@pytest.mark.parametrize("how", ["host", "ticket"])
def test_float_out_host_memory(gpu_ctx, how):
    items = _items([(256, 16, 12), (1000, 38, 14), (66, 6, 12)], 27)
    for dtype, layout in (("f16", "planes"), ("f32", "mosaic"), ("bf16", "planes")):
        got = _run(gpu_ctx, items, dtype, layout, 16383.0, (10, 20, 30, 40), True, [3, 1, 2, 0], mem=M.MEM_HOST,
                   ticket=how == "ticket")
        _check(items, got, dtype, layout, 16383.0, (10, 20, 30, 40), True, [3, 1, 2, 0])


@pytest.mark.parametrize("size", ["one", "all"])
def test_float_out_pool(size):
    devs = [0] if size == "one" else list(range(torch.cuda.device_count()))
    pool = M.Pool(devs)
    try:
        items = _items([(256, 16, 12), (1000, 38, 12)], 28) * max(1, len(devs))
        for mem, ticket in ((M.MEM_HOST, False), (M.MEM_HOST, True), (M.MEM_DEVICE, False)):
            got = _run(None, items, "f16", "planes", 4095.0, (64,) * 4, False, M.cfa_planes("rggb"), mem=mem, pool=pool, ticket=ticket)
            _check(items, got, "f16", "planes", 4095.0, (64,) * 4, False, M.cfa_planes("rggb"))
        # the pool's setter refuses a bad stage too
        with pytest.raises(M.McrawError):
            pool.set_float_out("f16", 10.0, black=(20, 0, 0, 0))
    finally:
        pool.close()


def test_invalid_stages_rejected(gpu_ctx):
    lib = gpu_ctx._lib
    good = M.float_out("f16", 4095.0)
    bad = []
    for field, v in (("dtype", 0), ("dtype", 4), ("layout", 2), ("flags", 2), ("flags", 0x80000001)):
        f = M.float_out("f16", 4095.0)
        setattr(f, field, v)
        bad.append(f)
    for white in (64.0, 10.0, float("inf"), float("nan"), -1.0):
        bad.append(M.float_out("f16", white, black=(0, 0, 0, 64)))
    for plane in ([0, 1, 2, 2], [0, 1, 2, 4], [3, 3, 3, 3]):
        bad.append(M.float_out("f16", 4095.0, plane=plane))
    for f in bad:
        assert lib.mcraw_ctx_set_float_out(gpu_ctx._h, C.byref(f)) < 0
        assert lib.mcraw_last_error()
    assert lib.mcraw_ctx_set_float_out(gpu_ctx._h, C.byref(good)) == 0
    assert lib.mcraw_ctx_set_float_out(gpu_ctx._h, None) == 0
    # a rejected stage leaves the plain mosaic
    items = _items([(64, 4, 12)], 29)
    f = M.float_out("f16", 1.0, black=(5, 0, 0, 0))
    assert lib.mcraw_ctx_set_float_out(gpu_ctx._h, C.byref(f)) < 0
    import _gpu
    written, status, outs = _gpu.decode_batch_device(gpu_ctx, [it[:4] for it in items])
    for (typ, w, h, buf, want), o, st in zip(items, outs, status):
        assert st == 0 and np.array_equal(o, want)


def test_set_post_and_set_float_out_replace_each_other(gpu_ctx):
    import _gpu
    items = _items([(256, 16, 12)], 30)
    plain = [it[:4] for it in items]
    # float stage, then set_post(black): the post stage's output (uint16 minus black levels)
    gpu_ctx.set_float_out("f32", 4095.0)
    gpu_ctx.set_post(black=[64, 64, 64, 64])
    try:
        written, status, outs = _gpu.decode_batch_device(gpu_ctx, plain)
        for (typ, w, h, buf, want), o in zip(items, outs):
            assert np.array_equal(o, np.maximum(want.astype(np.int32) - 64, 0).astype(np.uint16))
        # then set_post(None) after a float stage: the plain mosaic
        gpu_ctx.set_float_out("f16", 4095.0)
        gpu_ctx.set_post()
        written, status, outs = _gpu.decode_batch_device(gpu_ctx, plain)
        for (typ, w, h, buf, want), o in zip(items, outs):
            assert np.array_equal(o, want)
    finally:
        gpu_ctx.set_post()
    # post stage, then set_float_out: the float output
    gpu_ctx.set_post(black=[64, 64, 64, 64], pack12=True)
    got = _run(gpu_ctx, items, "bf16", "planes", 4095.0, (64,) * 4)
    _check(items, got, "bf16", "planes", 4095.0, (64,) * 4)


@pytest.mark.parametrize("layout", ["planes", "mosaic"])
def test_decode_tensor_on_side_stream(gpu_ctx, layout):
    dev = torch.device("cuda:0")
    w, h = 1000, 38
    items = _items([(w, h, 12)] * 3, 31, types=(7,)) + _items([(w, h, 12)], 32, types=(6,))
    t7 = [torch.from_numpy(np.ascontiguousarray(buf)).to(dev) for (t, _, _, buf, _) in items if t == 7]
    t6 = [(lambda x: (x, (x.data_ptr(), x.numel())))(torch.from_numpy(np.ascontiguousarray(buf)).to(dev)) for (t, _, _, buf, _) in items if t == 6]
    torch.cuda.synchronize()
    gpu_ctx.set_post(black=[1, 2, 3, 4])  # the stage the helper must restore
    try:
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            out7 = gpu_ctx.decode_tensor(t7, w, h, 7, dtype=torch.float16, white=4095, layout=layout, black=(64,) * 4,
                                         plane=M.cfa_planes("bggr"), check=False)
            doubled = out7.float() * 2.0  # queued behind the decode on the same stream, no synchronisation
            out6 = gpu_ctx.decode_tensor([p for (_, p) in t6], w, h, 6, dtype="f32", white=4095, layout=layout, clip=True)
        s.synchronize()
        assert gpu_ctx._stage == ("post", dict(black=[1, 2, 3, 4], pack12=False, bits=None))
        shape = (3, 4, h // 2, w // 2) if layout == "planes" else (3, h, w)
        assert tuple(out7.shape) == shape and out7.dtype == torch.float16 and out7.device == dev
        imgs7 = [it[4] for it in items if it[0] == 7]
        for i, img in enumerate(imgs7):
            ref = R.float_ref(img, "f16", 4095.0, layout, (64,) * 4, False, M.cfa_planes("bggr"))
            assert np.array_equal(out7[i].cpu().numpy().view(np.uint16), ref.view(np.uint16)), i
            assert np.array_equal(doubled[i].cpu().numpy(), ref.astype(np.float32) * 2.0), i
        ref6 = R.float_ref([it[4] for it in items if it[0] == 6][0], "f32", 4095.0, layout, clip=True)
        assert np.array_equal(out6[0].cpu().numpy(), ref6)
        # the restored stage is in force: a plain batch now gets the black levels
        import _gpu
        _, status, outs = _gpu.decode_batch_device(gpu_ctx, [items[0][:4]])
        want = items[0][4].astype(np.int32) - np.array([[1, 2], [3, 4]])[np.arange(h)[:, None] & 1, np.arange(w)[None, :] & 1]
        assert np.array_equal(outs[0], np.maximum(want, 0).astype(np.uint16))
    finally:
        gpu_ctx.set_post()


def test_decode_tensor_default_stream_out_and_errors(gpu_ctx):
    dev = torch.device("cuda:0")
    w, h = 256, 16
    items = _items([(w, h, 12)] * 2, 33, types=(7,))
    ins = [torch.from_numpy(np.ascontiguousarray(it[3])).to(dev) for it in items]
    out = torch.full((2, 4, h // 2, w // 2), 7.0, dtype=torch.bfloat16, device=dev)
    res = gpu_ctx.decode_tensor(ins, w, h, 7, dtype=torch.bfloat16, white=4095.0, out=out)
    total = (res.float().sum(dim=(1, 2, 3)))  # on the default stream behind the decode
    assert res.data_ptr() == out.data_ptr()
    for i, it in enumerate(items):
        ref = R.float_ref(it[4], "bf16", 4095.0, "planes")
        assert np.array_equal(res[i].cpu().view(torch.int16).numpy().view(np.uint16), ref)
    assert gpu_ctx._stage is None
    assert torch.isfinite(total).all()
    # a frame that fails is named
    broken = ins[1].clone()
    broken[:16] = 0xFF
    with pytest.raises(M.McrawError, match="frame 1"):
        gpu_ctx.decode_tensor([ins[0], broken], w, h, 7, dtype="f16", white=4095.0)
    assert gpu_ctx._stage is None
