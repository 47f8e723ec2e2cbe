"""Denoising of mosaics (mcraw_denoise_batch, Context.denoise, denoise= on the demosaic / decode methods) on the GPU: every
output sample equals the numpy statement of the contract (_denoise_ref), nothing outside the output is written, the input is
left as it was, rejected calls write nothing and say why, each queued call reads its table's contents in stream order, and
the context's decode state and the sibling entry points are undisturbed."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _denoise_ref as D
import _libs as L
import motioncam_decoder_amd as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = 0xA5A5
GEOMS = ((1, 1), (2, 2), (3, 5), (4, 9), (5, 4), (8, 8), (9, 9), (1, 64), (33, 1), (16, 64), (35, 41), (34, 520), (70, 1002))  # (H, W)
AMOUNTS = (1, 77, 256)
PROFILE = dict(S=2e-4, O=2e-6, black=64, white=4095)
SRGBISH = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)


def _np(t):
    a = t.detach()
    if a.dtype == torch.uint16:
        return a.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return a.cpu().numpy()


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _noise(rng, shape, level=800.0):
    """Noise of the profile's own sigma around a level: weights across their whole range under a noise_lut table."""
    R = PROFILE["white"] - PROFILE["black"]
    sigma = np.sqrt(PROFILE["S"] * R * (level - PROFILE["black"]) + PROFILE["O"] * R * R)
    return np.clip(np.rint(level + sigma * rng.standard_normal(shape)), 0, 65535).astype(np.uint16)


def _cases(rng, n, H, W):
    """(name, images, table, shift): the contents and tables of the contract's test plan."""
    full = rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)  # every weight 0 or small
    ties = (rng.integers(0, 1 << 12, size=(n, H, W), dtype=np.uint16) >> 6 << 6).astype(np.uint16)
    noise = _noise(rng, (n, H, W))
    rnd = lambda *shape: rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)
    out = [("full/zero", full, np.zeros((4, 64), np.uint16), 10), ("full/identity", full, np.full((4, 256), 65535, np.uint16), 8),
           ("full/random", full, rnd(4, 1024) >> 4, 6), ("full/per-frame", full, rnd(n, 4, 256) >> 6, 8),
           ("ties/random", ties, rnd(4, 256) >> 10, 4), ("ties/zero", ties, np.zeros((4, 1024), np.uint16), 2)]
    for entries in (64, 256, 1024):  # lut_log2 6, 8, 10 with the shifts that go with them
        lut, shift = M.noise_lut(entries=entries, **PROFILE)
        out.append(("noise/noise_lut %d" % entries, noise, lut, shift))
    per = np.stack([M.noise_lut(strength=2.0 + f, **PROFILE)[0] for f in range(n)])
    out.append(("noise/per-frame", noise, per, 4))
    return out


def _check(ctx, t, imgs, table, shift, what):
    """Both radii and every amount against the statement: m once per radius and frame."""
    n = imgs.shape[0]
    dl = _dev16(table)
    for radius in (1, 2):
        c = imgs.astype(np.int64)
        m = np.stack([D.mean(imgs[f], table if table.ndim == 2 else table[f], shift, radius) for f in range(n)])
        for amount in AMOUNTS:
            res = ctx.denoise(t, dl, shift, radius=radius, amount=amount / 256.0)
            torch.cuda.synchronize()
            assert tuple(res.shape) == imgs.shape and res.dtype == torch.uint16
            bad = np.argwhere(_np(res) != D.blend(c, m, amount))
            assert bad.size == 0, (what, radius, amount, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("geom", GEOMS)
def test_denoise_matches_reference(gpu_ctx, geom):
    H, W = geom
    rng = np.random.default_rng(zlib.crc32(("%dx%d" % (H, W)).encode()))
    n = 2
    kept = {}
    for name, imgs, table, shift in _cases(rng, n, H, W):
        t = kept.setdefault(id(imgs), _dev16(imgs))
        _check(gpu_ctx, t, imgs, table, shift, name)
        assert np.array_equal(_np(t), imgs), "the input was written"


def test_full_size(gpu_ctx):
    H, W, n = 2160, 3840, 2
    rng = np.random.default_rng(11)
    imgs = _noise(rng, (n, H, W))
    lut, shift = M.noise_lut(**PROFILE)
    res = gpu_ctx.denoise(_dev16(imgs), lut, shift, radius=2, amount=1.0)  # a host table: uploaded
    torch.cuda.synchronize()
    got = _np(res)
    assert np.array_equal(got[0], D.denoise(imgs[:1], lut, shift, 2, 256)[0])
    # the second frame in five windows (corners and centre); the crops reach 8 further in, so every neighbour is theirs
    for ys, xs in ((0, 0), (0, W - 96), (H - 96, 0), (H - 96, W - 96), (H // 2, W // 2)):
        y0, y1, x0, x1 = max(ys - 8, 0), min(ys + 104, H), max(xs - 8, 0), min(xs + 104, W)
        if 0 < y0 or 0 < x0:
            assert y0 % 2 == 0 and x0 % 2 == 0  # the crop keeps the CFA position of its pixels
        want = D.denoise(imgs[1:, y0:y1, x0:x1], lut, shift, 2, 256)[0]
        # rows and columns next to a cut (not a frame edge) reflect differently: compare those at least 8 from a cut
        a0, a1 = (0 if y0 == 0 else 8), (y1 - y0 if y1 == H else y1 - y0 - 8)
        b0, b1 = (0 if x0 == 0 else 8), (x1 - x0 if x1 == W else x1 - x0 - 8)
        assert np.array_equal(got[1, y0 + a0:y0 + a1, x0 + b0:x0 + b1], want[a0:a1, b0:b1]), (ys, xs)


def _strided(base, n, h, w, fstride, pitch, off):
    return torch.as_strided(base, (n, h, w), (fstride, pitch, 1), off).view(torch.uint16)


# (H, W, input pitch, input frame slack, input offset, output pitch, output frame slack, output offset): offsets in samples;
# 1 = an odd base address in samples (off the dword grid), 4 = on the 8-byte grid only, 8 with pitches and strides that are
# multiples of 8 = the 16-byte path; a pitch % 8 != 0 or a slack % 8 != 0 takes rows or frames off the 16-byte grid
VIEWS = ((35, 41, 53, 29, 1, 47, 3, 4), (34, 520, 520, 0, 4, 531, 17, 1), (70, 1002, 1008, 8, 8, 1016, 16, 8),
         (16, 64, 64, 0, 0, 72, 8, 1), (33, 1, 3, 5, 1, 1, 0, 1), (1, 64, 64, 0, 8, 64, 3, 0), (70, 1002, 1003, 1, 0, 1002, 0, 4),
         (34, 520, 528, 4, 0, 528, 0, 0), (9, 9, 11, 2, 1, 9, 0, 1))


@pytest.mark.parametrize("view", VIEWS)
def test_pitched_strided_offset_views_and_guards(gpu_ctx, view):
    H, W, ipitch, islack, ioff, opitch, oslack, ooff = view
    rng = np.random.default_rng(zlib.crc32(repr(view).encode()))
    n, guard = 3, 4096
    ifs, ofs = H * ipitch + islack, H * opitch + oslack
    imgs = _noise(rng, (n, H, W))
    ibase = torch.from_numpy(rng.integers(0, 1 << 16, size=n * ifs + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    src = _strided(ibase, n, H, W, ifs, ipitch, ioff)
    src.view(torch.int16).copy_(torch.from_numpy(imgs.view(np.int16)).to(DEV))
    before = ibase.clone()
    total = guard + ooff + n * ofs + guard
    obase = torch.full((total,), SENT - 65536, dtype=torch.int16, device=DEV)  # 0xA5A5 as int16
    dst = _strided(obase, n, H, W, ofs, opitch, guard + ooff)
    lut, shift = M.noise_lut(**PROFILE)
    per = np.stack([M.noise_lut(strength=1.5 + f, entries=64, **PROFILE)[0] for f in range(n)])
    for table, sh, radius, amount in ((lut, shift, 2, 256), (per, 6, 1, 77), (per, 6, 2, 200)):
        res = gpu_ctx.denoise(src, table, sh, radius=radius, amount=amount / 256.0, out=dst)
        torch.cuda.synchronize()
        assert res is dst
        want = D.denoise(imgs, table, sh, radius, amount)
        expect = np.full(total, SENT, np.uint16)
        np.lib.stride_tricks.as_strided(expect[guard + ooff:], (n, H, W), (ofs * 2, opitch * 2, 2))[...] = want
        got = obase.cpu().numpy().view(np.uint16)
        assert np.array_equal(got[:guard + ooff], expect[:guard + ooff]) and np.array_equal(got[-guard:], expect[-guard:]), "guards"
        assert np.array_equal(got, expect), np.argwhere(got != expect)[:4].tolist()  # the padding of rows and frames too
        assert torch.equal(ibase, before), "the input was written"
        obase.fill_(SENT - 65536)


def _struct(radius=2, amount=256, lut_log2=8, shift=4, nluts=1, reserved=(0, 0, 0), lut=0):
    s = M.Denoise()
    s.radius, s.amount, s.lut_log2, s.shift, s.nluts = radius, amount, lut_log2, shift, nluts
    s.reserved[0], s.reserved[1], s.reserved[2] = reserved
    s.lut = lut or None
    return s


def _raw(ctx, s, in_ptr, ip, ifs, w, h, n, out_ptr, op, ofs, stream=None):
    return M.load().mcraw_denoise_batch(ctx._h, C.byref(s) if s is not None else None, C.c_void_p(in_ptr), ip, ifs, w, h, n,
                                        C.c_void_p(out_ptr), op, ofs, C.c_void_p(stream))


def test_rejections_write_nothing_and_say_why(gpu_ctx):
    w, h, n = 24, 10, 2
    buf = torch.full((8192,), SENT - 65536, dtype=torch.int16, device=DEV)
    table, shift = M.noise_lut(**PROFILE)
    aux = _dev16(np.concatenate([table.reshape(-1), table.reshape(-1)]))  # room for two tables of 256 entries
    base, ab = buf.data_ptr(), aux.data_ptr()
    assert ab % 16 == 0
    ip, op = base, base + 2 * 4096
    good = dict(in_ptr=ip, ip=w, ifs=w * h, w=w, h=h, n=n, out_ptr=op, op=w, ofs=w * h)

    def call(st=None, **kw):
        a = dict(good)
        a.update(kw)
        return _raw(gpu_ctx, st if st is not None else _struct(lut=ab), a["in_ptr"], a["ip"], a["ifs"], a["w"], a["h"], a["n"],
                    a["out_ptr"], a["op"], a["ofs"])

    cases = [
        ("no struct", lambda: _raw(gpu_ctx, None, ip, w, w * h, w, h, n, op, w, w * h)),
        ("NULL in", lambda: call(in_ptr=0)),
        ("NULL out", lambda: call(out_ptr=0)),
        ("NULL lut", lambda: call(_struct(lut=0))),
        ("odd in", lambda: call(in_ptr=ip + 1)),
        ("odd out", lambda: call(out_ptr=op + 1)),
        ("lut on the 8-byte grid only", lambda: call(_struct(lut=ab + 8))),
        ("lut on the 2-byte grid only", lambda: call(_struct(lut=ab + 2))),
        ("width 0", lambda: call(w=0)),
        ("width 65537", lambda: call(w=65537, ip=65537, op=65537, n=1)),
        ("height 0", lambda: call(h=0)),
        ("height 65537", lambda: call(h=65537, n=1)),
        ("negative width", lambda: call(w=-4)),
        ("in pitch below width", lambda: call(ip=w - 1)),
        ("out pitch below width", lambda: call(op=w - 1)),
        ("in frame stride too small", lambda: call(ifs=w * h - 1)),
        ("out frame stride too small", lambda: call(ofs=(h - 1) * w + w - 1)),
        ("radius 0", lambda: call(_struct(radius=0, lut=ab))),
        ("radius 3", lambda: call(_struct(radius=3, lut=ab))),
        ("amount 0", lambda: call(_struct(amount=0, lut=ab))),
        ("amount 257", lambda: call(_struct(amount=257, lut=ab))),
        ("lut_log2 5", lambda: call(_struct(lut_log2=5, lut=ab))),
        ("lut_log2 11", lambda: call(_struct(lut_log2=11, lut=ab))),
        ("shift 16", lambda: call(_struct(shift=16, lut=ab))),
        ("nluts 0", lambda: call(_struct(nluts=0, lut=ab))),
        ("nluts 3 of 2 frames", lambda: call(_struct(nluts=3, lut=ab))),
        ("nluts 2 of 1 frame", lambda: call(_struct(nluts=2, lut=ab), n=1)),
        ("reserved[0]", lambda: call(_struct(reserved=(1, 0, 0), lut=ab))),
        ("reserved[1]", lambda: call(_struct(reserved=(0, 1, 0), lut=ab))),
        ("reserved[2]", lambda: call(_struct(reserved=(0, 0, 1), lut=ab))),
        ("negative n", lambda: call(n=-1)),
        ("in place", lambda: call(out_ptr=ip)),
        ("in place, one frame", lambda: call(out_ptr=ip, n=1)),
        ("out inside in", lambda: call(out_ptr=ip + 16)),
        ("out ends inside in", lambda: call(in_ptr=op + 2 * (n * w * h - 8))),
        ("same base, other pitch", lambda: call(out_ptr=ip, op=w + 8, ofs=(w + 8) * h)),
    ]
    serial = gpu_ctx.last_serial()
    for name, fn in cases:
        rc = fn()
        assert rc < 0, name
        msg = M.load().mcraw_last_error().decode()
        assert msg.startswith("mcraw_denoise_batch: ") and len(msg) > len("mcraw_denoise_batch: "), name
    assert call(n=0) == 0  # n == 0: a no-op
    assert call(_struct(lut=0), n=0) == 0
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert (buf.cpu().numpy().view(np.uint16) == SENT).all()
    assert np.array_equal(_np(aux)[:table.size], table.reshape(-1))
    assert gpu_ctx.last_serial() == serial
    # good calls next to them do write: the edges of the ranges, one table and one per frame
    img = _noise(np.random.default_rng(1), (n, h, w))
    buf[:n * w * h].copy_(torch.from_numpy(img.reshape(-1).view(np.int16)).to(DEV))
    for st, tab in ((_struct(lut=ab), table), (_struct(nluts=2, radius=1, amount=77, lut=ab), np.stack([table, table]))):
        assert call(st) == 0
        torch.cuda.synchronize()
        a = buf.cpu().numpy().view(np.uint16)
        assert np.array_equal(a[4096:4096 + n * w * h], D.denoise(img, tab, shift, st.radius, st.amount).reshape(-1))
        assert (a[4096 + n * w * h:] == SENT).all() and (a[n * w * h:4096] == SENT).all()
        buf[4096:].fill_(SENT - 65536)
    # Python: what the wrapper checks itself
    t = torch.zeros((2, 8, 8), dtype=torch.int16, device=DEV).view(torch.uint16)
    for kw in (dict(radius=3), dict(radius=0), dict(amount=0.0), dict(amount=1.01), dict(amount=float("nan")), dict(shift=16),
               dict(shift=-1), dict(shift=2.5), dict(lut=table.astype(np.int32)), dict(lut=table[:3]), dict(lut=table[:, :100]),
               dict(lut=np.stack([table] * 3)), dict(lut=torch.zeros((4, 256), dtype=torch.float32, device=DEV)),
               dict(out=torch.zeros((2, 8, 9), dtype=torch.int16, device=DEV).view(torch.uint16))):
        args = dict(lut=table, shift=shift)
        args.update(kw)
        with pytest.raises(ValueError):
            gpu_ctx.denoise(t, **args)
    with pytest.raises(ValueError):
        gpu_ctx.denoise(t.view(torch.int16), table, shift)
    with pytest.raises(M.McrawError, match="mcraw_denoise_batch: .*overlap"):
        gpu_ctx.denoise(t, table, shift, out=t)
    for bad in (dict(lut=table, shift=shift, out=t), [table, shift], dict(lut=table)):
        with pytest.raises((ValueError, TypeError)):
            gpu_ctx.demosaic(t, dtype="f16", white=4095.0, denoise=bad)
    ok = gpu_ctx.denoise(t, table, np.int64(shift), amount=np.float32(0.5))
    assert tuple(ok.shape) == (2, 8, 8)
    torch.cuda.synchronize()


def test_same_table_pointer_new_contents_between_queued_calls(gpu_ctx):
    rng = np.random.default_rng(9)
    n, h, w = 2, 70, 1002
    imgs = _noise(rng, (n, h, w))
    t = _dev16(imgs)
    s = torch.cuda.Stream(DEV)
    tables = [M.noise_lut(strength=st, **PROFILE)[0] for st in (1.0, 2.0, 3.5, 6.0)]
    staged = [_dev16(a) for a in tables]
    dl = torch.empty((4, 256), dtype=torch.int16, device=DEV).view(torch.uint16)
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream(DEV).cuda_stream == s.cuda_stream != 0
        for k in range(4):  # no host sync between: the table is rewritten in stream order between the calls
            dl.view(torch.int16).copy_(staged[k].view(torch.int16))
            outs.append(gpu_ctx.denoise(t, dl, 4, radius=1 + k % 2))
    s.synchronize()
    wants = [D.denoise(imgs, tables[k], 4, 1 + k % 2) for k in range(4)]
    for k, o in enumerate(outs):
        assert np.array_equal(_np(o), wants[k]), k
    assert not np.array_equal(wants[0], wants[2]) and not np.array_equal(wants[1], wants[3])
    # the same call on the null stream gives the same
    r = gpu_ctx.denoise(t, staged[3], 4, radius=2)
    torch.cuda.synchronize()
    assert np.array_equal(_np(r), wants[3])


def _frames(rng, shapes, typ):
    items = []
    for (w, h) in shapes:
        img = L.natural_image_np(w, h, 12, 12.0, int(rng.integers(1 << 30)))
        buf = L.encode7(img) if typ == 7 else L.encode6(img)
        ret, want = (L.oracle_decode7 if typ == 7 else L.oracle_decode6)(buf, w, h)
        assert ret == w * h
        items.append((buf, want))
    return items


def test_decode_state_and_siblings_untouched(gpu_ctx):
    rng = np.random.default_rng(3)
    w, h = 512, 96
    items = _frames(rng, [(w, h)] * 2, 7)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    imgs = np.stack([want for _, want in items])
    t = _dev16(imgs)
    lut, shift = M.noise_lut(**PROFILE)
    kw = dict(algo="mhc", dtype="f16", white=4095.0, black=(64,) * 4, gain=(1.9, 1.0, 1.4), matrix=SRGBISH)
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    gm = M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (1.9, 1.4, 1.45, 2.3)]))
    gpu_ctx.set_float_out("f32", 4095.0, layout="mosaic", black=(64,) * 4)
    try:
        f0 = gpu_ctx.demosaic(t, **kw)
        p0 = gpu_ctx.fix_pixels(t, abs_thr=96, black=(64,) * 4)
        s0 = gpu_ctx.shade(t, gm, black=(64,) * 4)
        torch.cuda.synchronize()
        serial, errs = gpu_ctx.last_serial(), gpu_ctx.errors(reset=False)
        res = gpu_ctx.denoise(t, lut, shift)
        empty = gpu_ctx.denoise(t[:0], lut, shift)  # n == 0
        torch.cuda.synchronize()
        assert tuple(empty.shape) == (0, h, w)
        assert gpu_ctx.last_serial() == serial and gpu_ctx.errors(reset=False) == errs
        assert np.array_equal(_np(res), D.denoise(imgs, lut, shift))
        f1 = gpu_ctx.demosaic(t, **kw)
        p1 = gpu_ctx.fix_pixels(t, abs_thr=96, black=(64,) * 4)
        s1 = gpu_ctx.shade(t, gm, black=(64,) * 4)
        torch.cuda.synchronize()
        assert torch.equal(f0.view(torch.int16), f1.view(torch.int16))
        assert torch.equal(p0.view(torch.int16), p1.view(torch.int16)) and torch.equal(s0.view(torch.int16), s1.view(torch.int16))
        # the context's stage is as it was: the next plain batch is still the float mosaic
        o = torch.full((w * h * 4,), 0xA5, dtype=torch.uint8, device=DEV)
        written, status = gpu_ctx.decode_batch(M.Context.make_frames([(ins[0].data_ptr(), ins[0].numel(), w, h, 7, o.data_ptr(), w * h * 2)]))
        assert status == [0]
        import _float_ref as FR
        assert np.array_equal(o.cpu().numpy(), FR.ref_bytes(items[0][1], "f32", 4095.0, "mosaic", (64,) * 4))
        assert gpu_ctx.last_serial() == serial + 1
    finally:
        gpu_ctx.set_post()
    assert gpu_ctx.errors() == 0


def test_denoise_shapes(gpu_ctx):
    rng = np.random.default_rng(21)
    H, W = 35, 41
    imgs = _noise(rng, (2, H, W))
    t = _dev16(imgs)
    lut, shift = M.noise_lut(**PROFILE)
    one = gpu_ctx.denoise(t[1], lut, shift)  # an (H, W) mosaic drops N
    torch.cuda.synchronize()
    assert tuple(one.shape) == (H, W) and np.array_equal(_np(one), D.denoise(imgs[1:], lut, shift)[0])
    out = torch.empty((2, H, W), dtype=torch.int16, device=DEV).view(torch.uint16)
    res = gpu_ctx.denoise(t, _dev16(lut), shift, radius=1, amount=0.5, out=out)
    torch.cuda.synchronize()
    assert res is out and np.array_equal(_np(out), D.denoise(imgs, lut, shift, 1, 128))
    e = gpu_ctx.denoise(t[:0], lut, shift)
    assert tuple(e.shape) == (0, H, W)


def test_denoise_keyword(gpu_ctx):
    n, h, w = 2, 96, 512
    clean = np.stack([L.natural_image_np(w, h, 12, 12.0, 40 + i) for i in range(n)])
    rng = np.random.default_rng(4)
    R = PROFILE["white"] - PROFILE["black"]
    sigma = np.sqrt(PROFILE["S"] * R * np.maximum(clean.astype(np.float64) - 64, 0) + PROFILE["O"] * R * R)
    imgs = np.clip(np.rint(clean + sigma * rng.standard_normal(clean.shape)), 0, 4095).astype(np.uint16)
    ys, xs = np.meshgrid(np.arange(3, h - 3, 7), np.arange(3, w - 3, 9), indexing="ij")
    imgs[:, ys, xs] = np.clip(imgs[:, ys, xs].astype(np.int64) + np.where((ys + xs) & 1, 900, -900), 0, 4095).astype(np.uint16)
    t = _dev16(imgs)
    black, cfa, gain = (64, 64, 64, 64), "grbg", (1.7, 1.0, 1.4)
    kw = dict(white=4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH)
    lut, shift = M.noise_lut(**PROFILE)
    denoise = dict(lut=lut, shift=shift, radius=2, amount=0.75)
    defects = dict(abs_thr=200, rel_thr=26 / 256, rank=2)
    y = np.linspace(-1, 1, 13)[:, None]
    x = np.linspace(-1, 1, 17)[None, :]
    gm = M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (1.9, 1.4, 1.45, 2.3)]), cfa)
    # the explicit steps: denoise alone; defects, denoise, shading
    dn = gpu_ctx.denoise(t, **denoise)
    fixed = gpu_ctx.fix_pixels(t, black=black, **defects)
    fixed_dn = gpu_ctx.denoise(fixed, **denoise)
    three = gpu_ctx.shade(fixed_dn, gm, black=black)
    torch.cuda.synchronize()
    assert np.array_equal(_np(dn), D.denoise(imgs, lut, shift, 2, 192)) and not np.array_equal(_np(dn), imgs)
    assert not torch.equal(fixed.view(torch.int16), t.view(torch.int16))  # (the injected defects are found)
    wrong_order = gpu_ctx.shade(gpu_ctx.fix_pixels(dn, black=black, **defects), gm, black=black)
    assert not torch.equal(wrong_order.view(torch.int16), three.view(torch.int16))  # (the order matters on this content)
    all3 = dict(denoise=denoise, defects=defects, shading=gm)
    ins = [torch.from_numpy(L.encode7(img)).to(DEV) for img in imgs]
    s0 = gpu_ctx.last_serial()
    plain = gpu_ctx.decode_rgb(ins, w, h, 7, algo="mhc", dtype="f32", **kw)
    s1 = gpu_ctx.last_serial()
    assert torch.equal(plain.view(torch.int32), gpu_ctx.demosaic(t, algo="mhc", dtype="f32", **kw).view(torch.int32))
    # demosaic / decode_rgb
    a = gpu_ctx.demosaic(t, algo="mhc", dtype="f32", denoise=denoise, **kw)
    b = gpu_ctx.demosaic(t, algo="mhc", dtype="f32", **all3, **kw)
    assert torch.equal(a.view(torch.int32), gpu_ctx.demosaic(dn, algo="mhc", dtype="f32", **kw).view(torch.int32))
    assert torch.equal(b.view(torch.int32), gpu_ctx.demosaic(three, algo="mhc", dtype="f32", **kw).view(torch.int32))
    ra = gpu_ctx.decode_rgb(ins, w, h, 7, algo="mhc", dtype="f32", denoise=denoise, **kw)
    rb = gpu_ctx.decode_rgb(ins, w, h, 7, algo="mhc", dtype="f32", **all3, **kw)
    assert torch.equal(ra.view(torch.int32), a.view(torch.int32)) and torch.equal(rb.view(torch.int32), b.view(torch.int32))
    # demosaic_display / decode_display
    d = gpu_ctx.demosaic_display(t, algo="mhc", transfer="srgb", denoise=denoise, **kw)
    e = gpu_ctx.demosaic_display(t, algo="bin2", transfer="srgb", **all3, **kw)
    assert torch.equal(d, gpu_ctx.demosaic_display(dn, algo="mhc", transfer="srgb", **kw))
    assert torch.equal(e, gpu_ctx.demosaic_display(three, algo="bin2", transfer="srgb", **kw))
    assert torch.equal(gpu_ctx.decode_display(ins, w, h, 7, algo="mhc", transfer="srgb", denoise=denoise, **kw), d)
    assert torch.equal(gpu_ctx.decode_display(ins, w, h, 7, algo="bin2", transfer="srgb", **all3, **kw), e)
    # demosaic_yuv / decode_yuv
    v = gpu_ctx.demosaic_yuv(t, algo="bin2", fmt="nv12", denoise=denoise, **kw)
    u = gpu_ctx.demosaic_yuv(t, algo="mhc", fmt="p010", **all3, **kw)
    assert torch.equal(v, gpu_ctx.demosaic_yuv(dn, algo="bin2", fmt="nv12", **kw))
    assert torch.equal(u, gpu_ctx.demosaic_yuv(three, algo="mhc", fmt="p010", **kw))
    assert torch.equal(gpu_ctx.decode_yuv(ins, w, h, 7, algo="bin2", fmt="nv12", denoise=denoise, **kw), v)
    assert torch.equal(gpu_ctx.decode_yuv(ins, w, h, 7, algo="mhc", fmt="p010", **all3, **kw), u)
    torch.cuda.synchronize()
    assert gpu_ctx.last_serial() == s1 + 6 * (s1 - s0)  # six more decodes; the denoiser takes no serial
    assert np.array_equal(_np(t), imgs), "the caller's mosaic was written"
    # denoise=None is the call as it always was
    p0 = gpu_ctx.demosaic(t, algo="mhc", dtype="f16", denoise=None, **kw)
    p1 = gpu_ctx.demosaic(t, algo="mhc", dtype="f16", **kw)
    torch.cuda.synchronize()
    import _rgb_ref as R_
    assert torch.equal(p0.view(torch.int16), p1.view(torch.int16))
    assert np.array_equal(p0[1].cpu().numpy().view(np.uint16),
                          R_.ref_bits(imgs[1], "mhc", "f16", 4095.0, black=black, cfa=cfa, gain=gain, matrix=SRGBISH))
    assert gpu_ctx.errors() == 0
