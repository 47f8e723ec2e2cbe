"""Temporal merge of mosaics (mcraw_merge_batch, Context.merge / stack / decode_merge) on the GPU: every output sample equals the
numpy statement of the contract (_merge_ref), nothing outside the output is written, the input is left as it was, rejected
calls write nothing and say why, each queued call reads its table's and its positions' contents in stream order, and the
context's decode state is undisturbed."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _libs as L
import _merge_ref as R
import motioncam_decoder_amd as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = 0xA5A5
# (H, W); the kernel's tile is 256 columns x 32 rows (16 in the other build): one under, at and over it in each direction
GEOMS = ((1, 1), (2, 2), (3, 5), (5, 4), (9, 9), (1, 64), (33, 1), (35, 41), (34, 520), (70, 1002),
         (15, 255), (16, 256), (17, 257), (31, 255), (32, 256), (33, 257))
AMOUNTS = (1, 77, 256)
PROFILE = dict(S=2e-4, O=2e-6, black=64, white=4095)


def _np(t):
    a = t.detach()
    if a.dtype == torch.uint16:
        return a.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return a.cpu().numpy()


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _devpos(p):
    return torch.from_numpy(np.ascontiguousarray(p, dtype=np.int16)).to(DEV)


def _noise(rng, shape, level=800.0):
    """Noise of the profile's own sigma around a level: weights across their whole range under a noise_lut table."""
    Rg = PROFILE["white"] - PROFILE["black"]
    sigma = np.sqrt(PROFILE["S"] * Rg * (level - PROFILE["black"]) + PROFILE["O"] * Rg * Rg)
    return np.clip(np.rint(level + sigma * rng.standard_normal(shape)), 0, 65535).astype(np.uint16)


def _positions(rng, n):
    """Random positions within +-6 with odd values among them."""
    p = rng.integers(-6, 7, size=(n, 2))
    p[0] = (3, -5)
    return p


def _cases(rng, n, H, W):
    """(name, images, table, shift): the contents and tables of the contract's test plan."""
    full = rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)
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


def _means(imgs, table, shift, before, after, first, count, support, pos):
    return np.stack([R.mean(imgs, first + j, table if table.ndim == 2 else table[first + j], shift, before, after, support, pos)
                     for j in range(count)])


def _check(ctx, t, imgs, table, shift, what, before=2, after=2, first=0, count=None, positions=(None,), amounts=AMOUNTS):
    """Both supports, the given positions and amounts against the statement: m once per support, positions and base."""
    n = imgs.shape[0]
    count = n - first if count is None else count
    dl = _dev16(table)
    c = imgs[first:first + count].astype(np.int64)
    for pos in positions:
        dp = None if pos is None else _devpos(pos)
        for support in (0, 1):
            m = _means(imgs, table, shift, before, after, first, count, support, pos)
            for amount in amounts:
                res = ctx.merge(t, dl, shift, before=before, after=after, first=first, count=count, support=support,
                                amount=amount / 256.0, pos=dp)
                torch.cuda.synchronize()
                assert tuple(res.shape) == c.shape and res.dtype == torch.uint16
                bad = np.argwhere(_np(res) != R.blend(c, m, amount))
                assert bad.size == 0, (what, before, after, first, count, support, amount, pos is not None, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("geom", GEOMS)
def test_merge_matches_reference(gpu_ctx, geom):
    H, W = geom
    rng = np.random.default_rng(zlib.crc32(("%dx%d" % (H, W)).encode()))
    n = 6
    kept = {}
    pos = _positions(rng, n)
    for k, (name, imgs, table, shift) in enumerate(_cases(rng, n, H, W)):
        t = kept.setdefault(id(imgs), _dev16(imgs))
        _check(gpu_ctx, t, imgs, table, shift, name, positions=(None, pos), amounts=AMOUNTS if k in (2, 7) else (AMOUNTS[k % 3],))
        assert np.array_equal(_np(t), imgs), "the input was written"
    # the consequences of the contract, on the device
    full, noise = _cases(rng, n, H, W)[0][1], _noise(rng, (n, H, W))
    tf, tn = _dev16(full), _dev16(noise)
    lut, shift = M.noise_lut(**PROFILE)
    far = np.arange(n)[:, None] * np.array([[2 * H + 1, -2 * W - 1]])
    for support in (0, 1):
        same = gpu_ctx.merge(tf, np.full((4, 64), 65535, np.uint16), 10, support=support, pos=pos)
        none = gpu_ctx.merge(tn, lut, shift, before=0, after=0, support=support, pos=pos)
        gone = gpu_ctx.merge(tn, lut, shift, before=3, after=4, support=support, pos=far)
        mean = gpu_ctx.merge(tf, np.zeros((4, 128), np.uint16), 9, before=1, after=2, support=support)
        torch.cuda.synchronize()
        assert np.array_equal(_np(same), full) and np.array_equal(_np(none), noise) and np.array_equal(_np(gone), noise)
        for b in range(n):
            lo, hi = max(0, b - 1), min(n - 1, b + 2)
            assert np.array_equal(_np(mean[b]), (full[lo:hi + 1].astype(np.int64).sum(axis=0) + (hi - lo + 1) // 2) // (hi - lo + 1))


# (n, before, after, first, count)
WINDOWS = ((1, 2, 2, 0, 1), (1, 0, 0, 0, 1), (6, 0, 0, 0, 6), (6, 2, 2, 0, 6), (6, 0, 5, 0, 6), (6, 5, 0, 0, 6), (16, 7, 8, 0, 16),
           (16, 0, 15, 0, 16), (16, 15, 0, 0, 16), (6, 2, 2, 2, 2), (6, 2, 2, 3, 1), (16, 7, 8, 8, 1), (6, 2, 2, 5, 1), (6, 1, 3, 0, 0),
           (16, 0, 15, 0, 1), (16, 15, 0, 15, 1))


@pytest.mark.parametrize("win", WINDOWS)
def test_windows_and_subsets(gpu_ctx, win):
    n, before, after, first, count = win
    rng = np.random.default_rng(zlib.crc32(repr(win).encode()))
    H, W = 35, 41
    imgs = _noise(rng, (n, H, W))
    per = np.stack([M.noise_lut(strength=2.0 + 0.25 * f, entries=128, **PROFILE)[0] for f in range(n)])
    t = _dev16(imgs)
    if count == 0:
        res = gpu_ctx.merge(t, per, 5, before=before, after=after, first=first, count=0)
        assert tuple(res.shape) == (0, H, W)
        return
    _check(gpu_ctx, t, imgs, per, 5, "windows", before, after, first, count, positions=(None, _positions(rng, n)), amounts=(256,))
    if first == 0 and count == n:  # count=None means all frames from first on
        a = gpu_ctx.merge(t, per, 5, before=before, after=after)
        b = gpu_ctx.merge(t, per, 5, before=before, after=after, first=0, count=n)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_shift_forms(gpu_ctx):
    rng = np.random.default_rng(17)
    n, H, W = 6, 34, 520
    imgs = _noise(rng, (n, H, W))
    t = _dev16(imgs)
    lut, shift = M.noise_lut(**PROFILE)
    kw = dict(before=2, after=3, support=1)
    want0 = R.merge(imgs, lut, shift, 2, 3)
    null = gpu_ctx.merge(t, lut, shift, **kw)
    zeros = gpu_ctx.merge(t, lut, shift, pos=torch.zeros((n, 2), dtype=torch.int16, device=DEV), **kw)
    const = gpu_ctx.merge(t, lut, shift, pos=np.full((n, 2), -77), **kw)  # equal positions: every shift is 0
    torch.cuda.synchronize()
    for r in (null, zeros, const):
        assert np.array_equal(_np(r), want0)
    pos = _positions(rng, n)
    assert (pos & 1).any() and ((pos[:, None] - pos[None]) < 0).any()
    want = R.merge(imgs, lut, shift, 2, 3, pos=pos)
    assert not np.array_equal(want, want0)
    host = gpu_ctx.merge(t, lut, shift, pos=pos, **kw)  # a host array: uploaded
    lst = gpu_ctx.merge(t, lut, shift, pos=pos.tolist(), **kw)
    devt = gpu_ctx.merge(t, lut, shift, pos=_devpos(pos), **kw)
    torch.cuda.synchronize()
    for r in (host, lst, devt):
        assert np.array_equal(_np(r), want)
    # shifts by multiples of 8 (the aligned loads), and large ones that leave a sliver of the frame
    for pos in (np.array([[0, 0], [8, -16], [-8, 24], [16, 8], [2, 256], [-32, -264]]), np.array([[0, 0], [H - 1, W - 3], [1 - H, 3 - W]] * 2),
                np.array([[-32768, 32767], [32767, -32768]] * 3)):
        got = gpu_ctx.merge(t, lut, shift, pos=pos, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(_np(got), R.merge(imgs, lut, shift, 2, 3, pos=pos)), pos.tolist()
    far = np.arange(n)[:, None] * np.array([[H, -W - 1]])
    got = gpu_ctx.merge(t, lut, shift, pos=far, **kw)  # differences beyond the frame: the identity
    torch.cuda.synchronize()
    assert np.array_equal(_np(got), imgs)


def test_full_size(gpu_ctx):
    H, W, n = 2160, 3840, 3
    rng = np.random.default_rng(11)
    imgs = _noise(rng, (n, H, W))
    lut, shift = M.noise_lut(**PROFILE)
    pos = np.array([[0, 0], [3, -4], [-2, 6]])
    res = gpu_ctx.merge(_dev16(imgs), lut, shift, before=1, after=1, pos=pos)  # host table and positions: uploaded
    torch.cuda.synchronize()
    got = _np(res)
    assert np.array_equal(got[1], R.merge(imgs, lut, shift, 1, 1, 1, 1, pos=pos)[0])
    # the other frames in five windows (corners and centre); the crops reach 16 further in, so every sample read is theirs
    for f in (0, 2):
        for ys, xs in ((0, 0), (0, W - 96), (H - 96, 0), (H - 96, W - 96), (H // 2, W // 2)):
            y0, y1, x0, x1 = max(ys - 16, 0), min(ys + 112, H), max(xs - 16, 0), min(xs + 112, W)
            assert y0 % 2 == 0 and x0 % 2 == 0  # the crop keeps the CFA position of its pixels
            want = R.merge(imgs[:, y0:y1, x0:x1], lut, shift, 1, 1, f, 1, pos=pos)[0]
            # next to a cut (not a frame edge) the crop's members end early: compare what lies at least 16 from a cut
            a0, a1 = (0 if y0 == 0 else 16), (y1 - y0 if y1 == H else y1 - y0 - 16)
            b0, b1 = (0 if x0 == 0 else 16), (x1 - x0 if x1 == W else x1 - x0 - 16)
            assert np.array_equal(got[f, y0 + a0:y0 + a1, x0 + b0:x0 + b1], want[a0:a1, b0:b1]), (f, ys, xs)


def _strided(base, n, h, w, fstride, pitch, off):
    return torch.as_strided(base, (n, h, w), (fstride, pitch, 1), off).view(torch.uint16)


# (H, W, input pitch, input frame slack, input offset, output pitch, output frame slack, output offset): offsets in samples;
# 1 = an odd base address in samples (off the dword grid), 4 = on the 8-byte grid only, 8 with pitches and strides that are
# multiples of 8 = the 16-byte path; a pitch % 8 != 0 or a slack % 8 != 0 takes rows or frames off the 16-byte grid
VIEWS = ((35, 41, 53, 29, 1, 47, 3, 4), (34, 520, 520, 0, 4, 531, 17, 1), (70, 1002, 1008, 8, 8, 1016, 16, 8),
         (33, 1, 3, 5, 1, 1, 0, 1), (1, 64, 64, 0, 8, 64, 3, 0), (70, 1002, 1003, 1, 0, 1002, 0, 4), (34, 520, 528, 4, 0, 528, 0, 0),
         (9, 9, 11, 2, 1, 9, 0, 1))


@pytest.mark.parametrize("view", VIEWS)
def test_pitched_strided_offset_views_and_guards(gpu_ctx, view):
    H, W, ipitch, islack, ioff, opitch, oslack, ooff = view
    rng = np.random.default_rng(zlib.crc32(repr(view).encode()))
    n, guard = 4, 4096
    ifs, ofs = H * ipitch + islack, H * opitch + oslack
    imgs = _noise(rng, (n, H, W))
    ibase = torch.from_numpy(rng.integers(0, 1 << 16, size=n * ifs + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    src = _strided(ibase, n, H, W, ifs, ipitch, ioff)
    src.view(torch.int16).copy_(torch.from_numpy(imgs.view(np.int16)).to(DEV))
    before = ibase.clone()
    lut, shift = M.noise_lut(**PROFILE)
    per = np.stack([M.noise_lut(strength=1.5 + f, entries=64, **PROFILE)[0] for f in range(n)])
    pos = _positions(rng, n)
    for table, sh, kw in ((lut, shift, dict(before=1, after=2, support=1, amount=256)),
                          (per, 6, dict(before=2, after=1, first=1, count=2, support=0, amount=77, pos=pos)),
                          (per, 6, dict(before=0, after=3, first=2, count=1, support=1, amount=200, pos=pos))):
        count = kw.get("count", n)
        total = guard + ooff + count * ofs + guard
        obase = torch.full((total,), SENT - 65536, dtype=torch.int16, device=DEV)  # 0xA5A5 as int16
        dst = _strided(obase, count, H, W, ofs, opitch, guard + ooff)
        res = gpu_ctx.merge(src, table, sh, out=dst, **dict(kw, amount=kw["amount"] / 256.0))
        torch.cuda.synchronize()
        assert res is dst
        want = R.merge(imgs, table, sh, **kw)
        expect = np.full(total, SENT, np.uint16)
        np.lib.stride_tricks.as_strided(expect[guard + ooff:], (count, H, W), (ofs * 2, opitch * 2, 2))[...] = want
        got = obase.cpu().numpy().view(np.uint16)
        assert np.array_equal(got[:guard + ooff], expect[:guard + ooff]) and np.array_equal(got[-guard:], expect[-guard:]), "guards"
        assert np.array_equal(got, expect), np.argwhere(got != expect)[:4].tolist()  # the padding of rows and frames too
        assert torch.equal(ibase, before), "the input was written"


def _struct(before=1, after=1, first=0, count=2, support=1, amount=256, lut_log2=8, shift=4, nluts=1, reserved=0, lut=0, pos=0):
    s = M.Merge()
    s.before, s.after, s.first, s.count, s.support, s.amount = before, after, first, count, support, amount
    s.lut_log2, s.shift, s.nluts, s.reserved = lut_log2, shift, nluts, reserved
    s.lut = lut or None
    s.pos = pos or None
    return s


def _raw(ctx, s, in_ptr, ip, ifs, w, h, n, out_ptr, op, ofs, stream=None):
    return M.load().mcraw_merge_batch(ctx._h, C.byref(s) if s is not None else None, C.c_void_p(in_ptr), ip, ifs, w, h, n,
                                      C.c_void_p(out_ptr), op, ofs, C.c_void_p(stream))


def test_rejections_write_nothing_and_say_why(gpu_ctx):
    w, h, n = 24, 10, 2
    buf = torch.full((8192,), SENT - 65536, dtype=torch.int16, device=DEV)
    table, shift = M.noise_lut(**PROFILE)
    aux = _dev16(np.concatenate([table.reshape(-1), table.reshape(-1)]))  # room for two tables of 256 entries
    dpos = _devpos(np.array([[0, 0], [2, -2], [0, 0]]))
    base, ab, pb = buf.data_ptr(), aux.data_ptr(), dpos.data_ptr()
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
        ("odd pos", lambda: call(_struct(lut=ab, pos=pb + 1))),
        ("lut on the 8-byte grid only", lambda: call(_struct(lut=ab + 8))),
        ("lut on the 2-byte grid only", lambda: call(_struct(lut=ab + 2))),
        ("width 0", lambda: call(w=0)),
        ("width 65537", lambda: call(_struct(count=1, lut=ab), w=65537, ip=65537, op=65537, n=1)),
        ("height 0", lambda: call(h=0)),
        ("height 65537", lambda: call(_struct(count=1, lut=ab), h=65537, n=1)),
        ("negative width", lambda: call(w=-4)),
        ("in pitch below width", lambda: call(ip=w - 1)),
        ("out pitch below width", lambda: call(op=w - 1)),
        ("in frame stride too small", lambda: call(ifs=w * h - 1)),
        ("in frame stride too small, one output", lambda: call(_struct(count=1, lut=ab), ifs=w * h - 1)),
        ("out frame stride too small", lambda: call(ofs=(h - 1) * w + w - 1)),
        ("before + after 16", lambda: call(_struct(before=8, after=8, lut=ab))),
        ("before 16", lambda: call(_struct(before=16, after=0, lut=ab))),
        ("before 2^32 - 1", lambda: call(_struct(before=0xFFFFFFFF, after=1, lut=ab))),
        ("after 2^32 - 1", lambda: call(_struct(before=1, after=0xFFFFFFFF, lut=ab))),
        ("first + count 3 of 2", lambda: call(_struct(first=1, count=2, lut=ab))),
        ("first 3 of 2", lambda: call(_struct(first=3, count=1, lut=ab))),
        ("first + count wraps", lambda: call(_struct(first=2, count=0xFFFFFFFF, lut=ab))),
        ("support 2", lambda: call(_struct(support=2, lut=ab))),
        ("amount 0", lambda: call(_struct(amount=0, lut=ab))),
        ("amount 257", lambda: call(_struct(amount=257, lut=ab))),
        ("lut_log2 5", lambda: call(_struct(lut_log2=5, lut=ab))),
        ("lut_log2 11", lambda: call(_struct(lut_log2=11, lut=ab))),
        ("shift 16", lambda: call(_struct(shift=16, lut=ab))),
        ("nluts 0", lambda: call(_struct(nluts=0, lut=ab))),
        ("nluts 3 of 2 frames", lambda: call(_struct(nluts=3, lut=ab))),
        ("nluts 2 of 1 frame", lambda: call(_struct(count=1, nluts=2, lut=ab), n=1)),
        ("reserved", lambda: call(_struct(reserved=1, lut=ab))),
        ("negative n", lambda: call(n=-1)),
        ("in place", lambda: call(out_ptr=ip)),
        ("in place, one frame", lambda: call(_struct(count=1, lut=ab), out_ptr=ip, n=1)),
        ("one output inside the second input", lambda: call(_struct(first=0, count=1, lut=ab), out_ptr=ip + 2 * w * h)),
        ("out inside in", lambda: call(out_ptr=ip + 16)),
        ("out ends inside in", lambda: call(in_ptr=op + 2 * (n * w * h - 8))),
        ("same base, other pitch", lambda: call(out_ptr=ip, op=w + 8, ofs=(w + 8) * h)),
    ]
    serial = gpu_ctx.last_serial()
    for name, fn in cases:
        rc = fn()
        assert rc < 0, name
        msg = M.load().mcraw_last_error().decode()
        assert msg.startswith("mcraw_merge_batch: ") and len(msg) > len("mcraw_merge_batch: "), name
    assert call(n=0) == 0  # n == 0 or count == 0: a no-op
    assert call(_struct(lut=0), n=0) == 0
    assert call(_struct(count=0, lut=ab)) == 0
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert (buf.cpu().numpy().view(np.uint16) == SENT).all()
    assert np.array_equal(_np(aux)[:table.size], table.reshape(-1))
    assert gpu_ctx.last_serial() == serial
    # good calls next to them do write: one table and one per frame, with and without positions, a single output
    img = _noise(np.random.default_rng(1), (n, h, w))
    buf[:n * w * h].copy_(torch.from_numpy(img.reshape(-1).view(np.int16)).to(DEV))
    pos = np.array([[0, 0], [2, -2]])
    for st, tab, p in ((_struct(lut=ab), table, None), (_struct(nluts=2, support=0, amount=77, lut=ab, pos=pb), np.stack([table, table]), pos),
                       (_struct(first=1, count=1, before=15, after=0, lut=ab, pos=pb), table, pos)):
        assert call(st) == 0
        torch.cuda.synchronize()
        a = buf.cpu().numpy().view(np.uint16)
        want = R.merge(img, tab, shift, st.before, st.after, st.first, st.count, st.support, st.amount, p)
        assert np.array_equal(a[4096:4096 + want.size], want.reshape(-1))
        assert (a[4096 + want.size:] == SENT).all() and (a[n * w * h:4096] == SENT).all()
        buf[4096:].fill_(SENT - 65536)
    # Python: what the wrapper checks itself
    t = torch.zeros((3, 8, 8), dtype=torch.int16, device=DEV).view(torch.uint16)
    for kw in (dict(support=2), dict(amount=0.0), dict(amount=1.01), dict(amount=float("nan")), dict(shift=16), dict(shift=-1),
               dict(shift=2.5), dict(before=8, after=8), dict(before=-1), dict(after=1.5), dict(first=4), dict(first=2, count=2),
               dict(count=-1), dict(lut=table.astype(np.int32)), dict(lut=table[:3]), dict(lut=table[:, :100]),
               dict(lut=np.stack([table] * 2)), dict(lut=torch.zeros((4, 256), dtype=torch.float32, device=DEV)),
               dict(pos=np.zeros((2, 2), np.int64)), dict(pos=np.zeros((3, 2))), dict(pos=np.array([[0, 0], [0, 40000], [0, 0]])),
               dict(pos=np.array([[0, 0], [-32769, 0], [0, 0]])), dict(pos=torch.zeros((3, 2), dtype=torch.int32, device=DEV)),
               dict(pos=torch.zeros((3, 2), dtype=torch.int16)),
               dict(out=torch.zeros((3, 8, 9), dtype=torch.int16, device=DEV).view(torch.uint16)),
               dict(first=1, out=torch.zeros((3, 8, 8), dtype=torch.int16, device=DEV).view(torch.uint16))):
        args = dict(lut=table, shift=shift)
        args.update(kw)
        with pytest.raises(ValueError):
            gpu_ctx.merge(t, **args)
    for bad in (t.view(torch.int16), t[0]):
        with pytest.raises(ValueError):
            gpu_ctx.merge(bad, table, shift)
    with pytest.raises(M.McrawError, match="mcraw_merge_batch: .*overlap"):
        gpu_ctx.merge(t, table, shift, out=t)
    for kw in (dict(ref=3), dict(ref=-1), dict(before=1), dict(count=1), dict(out=t)):
        with pytest.raises(ValueError):
            gpu_ctx.stack(t, table, shift, **kw)
    with pytest.raises(ValueError):
        gpu_ctx.stack(torch.zeros((17, 8, 8), dtype=torch.int16, device=DEV).view(torch.uint16), table, shift)
    ok = gpu_ctx.merge(t, table, np.int64(shift), amount=np.float32(0.5), before=np.int32(1), after=1)
    assert tuple(ok.shape) == (3, 8, 8)
    torch.cuda.synchronize()


def test_table_and_positions_are_read_in_stream_order(gpu_ctx):
    rng = np.random.default_rng(9)
    n, h, w = 4, 70, 1002
    imgs = _noise(rng, (n, h, w))
    t = _dev16(imgs)
    s = torch.cuda.Stream(DEV)
    tables = [M.noise_lut(strength=st, **PROFILE)[0] for st in (1.0, 2.0, 3.5, 6.0)]
    poss = [rng.integers(-6, 7, size=(n, 2)) for _ in range(4)]
    staged = [(_dev16(a), _devpos(p)) for a, p in zip(tables, poss)]
    dl = torch.empty((4, 256), dtype=torch.int16, device=DEV).view(torch.uint16)
    dp = torch.empty((n, 2), dtype=torch.int16, device=DEV)
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream(DEV).cuda_stream == s.cuda_stream != 0
        for k in range(4):  # no host sync between: the table and the positions are rewritten in stream order between the calls
            dl.view(torch.int16).copy_(staged[k][0].view(torch.int16))
            dp.copy_(staged[k][1])
            outs.append(gpu_ctx.merge(t, dl, 4, before=1, after=2, support=k % 2, pos=dp))
    s.synchronize()
    wants = [R.merge(imgs, tables[k], 4, 1, 2, support=k % 2, pos=poss[k]) for k in range(4)]
    for k, o in enumerate(outs):
        assert np.array_equal(_np(o), wants[k]), k
    assert not np.array_equal(wants[0], wants[2]) and not np.array_equal(wants[1], wants[3])
    # the same call on the null stream gives the same
    r = gpu_ctx.merge(t, staged[3][0], 4, before=1, after=2, support=1, pos=staged[3][1])
    torch.cuda.synchronize()
    assert np.array_equal(_np(r), wants[3])


def test_decode_state_untouched_and_the_other_forms(gpu_ctx):
    rng = np.random.default_rng(3)
    w, h, n = 512, 96, 4
    items = []
    for i in range(n):
        img = L.natural_image_np(w, h, 12, 12.0, int(rng.integers(1 << 30)))
        buf = L.encode7(img)
        ret, want = L.oracle_decode7(buf, w, h)
        assert ret == w * h
        items.append((buf, want))
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    imgs = np.stack([want for _, want in items])
    t = _dev16(imgs)
    lut, shift = M.noise_lut(**PROFILE)
    pos = _positions(rng, n)
    gpu_ctx.set_float_out("f32", 4095.0, layout="mosaic", black=(64,) * 4)
    try:
        d0 = gpu_ctx.denoise(t, lut, shift)
        torch.cuda.synchronize()
        serial, errs = gpu_ctx.last_serial(), gpu_ctx.errors(reset=False)
        res = gpu_ctx.merge(t, lut, shift, before=1, after=2, pos=pos)
        empty = gpu_ctx.merge(t[:0], lut, shift)  # n == 0
        none = gpu_ctx.merge(t, lut, shift, first=2, count=0)
        stacked = [gpu_ctx.stack(t, lut, shift, ref=r, pos=pos, support=r & 1, amount=0.5) for r in range(n)]
        so = torch.empty((h, w), dtype=torch.int16, device=DEV).view(torch.uint16)
        assert gpu_ctx.stack(t, lut, shift, out=so).data_ptr() == so.data_ptr()
        torch.cuda.synchronize()
        assert tuple(empty.shape) == (0, h, w) and tuple(none.shape) == (0, h, w)
        assert gpu_ctx.last_serial() == serial and gpu_ctx.errors(reset=False) == errs
        assert np.array_equal(_np(res), R.merge(imgs, lut, shift, 1, 2, pos=pos))
        for r in range(n):
            assert tuple(stacked[r].shape) == (h, w)
            assert np.array_equal(_np(stacked[r]), R.merge(imgs, lut, shift, r, n - 1 - r, r, 1, r & 1, 128, pos)[0]), r
        assert np.array_equal(_np(so), R.merge(imgs, lut, shift, 0, n - 1, 0, 1)[0])
        d1 = gpu_ctx.denoise(t, lut, shift)
        torch.cuda.synchronize()
        assert torch.equal(d0.view(torch.int16), d1.view(torch.int16))
        # the context's stage is as it was: the next plain batch is still the float mosaic
        o = torch.full((w * h * 4,), 0xA5, dtype=torch.uint8, device=DEV)
        written, status = gpu_ctx.decode_batch(M.Context.make_frames([(ins[0].data_ptr(), ins[0].numel(), w, h, 7, o.data_ptr(), w * h * 2)]))
        assert status == [0]
        import _float_ref as FR
        assert np.array_equal(o.cpu().numpy(), FR.ref_bytes(items[0][1], "f32", 4095.0, "mosaic", (64,) * 4))
        assert gpu_ctx.last_serial() == serial + 1
        # decode_merge: the decode and the merge in one call; the stage is restored
        s0 = gpu_ctx.last_serial()
        dm = gpu_ctx.decode_merge(ins, w, h, 7, lut=lut, shift=shift, before=1, after=2, pos=pos)
        torch.cuda.synchronize()
        assert gpu_ctx.last_serial() > s0
        assert torch.equal(dm.view(torch.int16), res.view(torch.int16))
        o.fill_(0xA5)
        written, status = gpu_ctx.decode_batch(M.Context.make_frames([(ins[1].data_ptr(), ins[1].numel(), w, h, 7, o.data_ptr(), w * h * 2)]))
        assert status == [0]
        assert np.array_equal(o.cpu().numpy(), FR.ref_bytes(items[1][1], "f32", 4095.0, "mosaic", (64,) * 4))
    finally:
        gpu_ctx.set_post()
    assert gpu_ctx.errors() == 0
