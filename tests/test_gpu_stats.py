"""Per-frame mosaic statistics (mcraw_stats_batch, Context.stats, Context.decode_stats) on the GPU: every record equals the
numpy statement of the contract (_stats_ref) byte for byte -- everything is an integer, so there is no tolerance --, the call
initialises its records itself and writes nothing else, the input is left as it was, accumulation adds up, rejected calls
write nothing and say why, a queued call reads its input in stream order, and the context's decode state is undisturbed."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _libs as L
import _stats_ref as S
import motioncam_decoder_amd as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GEOMS = ((2, 2), (1, 64), (33, 1), (35, 41), (34, 520), (70, 1002), (71, 1001), (1080, 1920))  # (H, W)
CONTENTS = ("noise", "flat-below", "flat-saturated", "checker", "ramp")
BINS_SHIFTS = [(b, s) for b in (64, 256, 4096) for s in (0, 4, 8, 15)]  # with shifts whose last bin absorbs the overflow
SATS = ((65535,) * 4, (0, 65535, 40000, 1000), (4095,) * 4, (30000, 1, 65535, 0))
FLAT_SAT = 5000


def _np(t):
    a = t.detach()
    if a.dtype == torch.uint16:
        return a.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return a.cpu().numpy()


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _content(kind, rng, n, H, W):
    if kind == "noise":
        return rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)
    if kind == "flat-below":  # every sample equal: all lanes of a wave on one counter
        return np.full((n, H, W), FLAT_SAT - 1, np.uint16)
    if kind == "flat-saturated":
        return np.full((n, H, W), FLAT_SAT, np.uint16)
    if kind == "checker":  # two values, in a checker by CFA position
        img = np.empty((n, H, W), np.uint16)
        img[:, 0::2, 0::2], img[:, 1::2, 1::2] = 700, 700
        img[:, 0::2, 1::2], img[:, 1::2, 0::2] = 51000, 51000
        return img
    ramp = (np.arange(W, dtype=np.int64) * 65535 // max(W - 1, 1)).astype(np.uint16)  # a horizontal ramp
    return np.broadcast_to(ramp, (n, H, W)).copy()


def _check(got, want_fields, what=""):
    got = got.raw if isinstance(got, M.FrameStats) else got
    a, b = _np(got), S.record(want_fields)
    if a.ndim == 1:
        a = a[None]
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        bins = want_fields["hist"].shape[2]
        g = S.parse(a, bins)
        bad = {k: np.argwhere(g[k] != want_fields[k])[:3].tolist() for k in g if not np.array_equal(g[k], want_fields[k])}
        raise AssertionError("%s: records differ in %r" % (what, bad))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("geom", GEOMS)
def test_content_matches_reference(gpu_ctx, geom, content):
    H, W = geom
    k = GEOMS.index(geom) * len(CONTENTS) + CONTENTS.index(content)
    rng = np.random.default_rng(zlib.crc32(("%dx%d %s" % (H, W, content)).encode()))
    n = 2 if H * W > 1 << 20 else 3
    imgs = _content(content, rng, n, H, W)
    t = _dev16(imgs)
    bins, shift = BINS_SHIFTS[k % len(BINS_SHIFTS)]
    sat = (FLAT_SAT,) * 4 if content.startswith("flat") else SATS[(k // 2) % len(SATS)]
    res = gpu_ctx.stats(t, bins=bins, shift=shift, sat=sat)
    torch.cuda.synchronize()
    assert isinstance(res, M.FrameStats) and tuple(res.raw.shape) == (n, 16 * bins + 96) and res.raw.dtype == torch.uint8
    assert res.bins == bins and res.shift == shift
    want = S.stats(imgs, bins, shift, sat)
    _check(res, want, "%s %dx%d bins %d shift %d" % (content, H, W, bins, shift))
    assert np.array_equal(_np(t), imgs), "the input was written"
    # the views are the record's fields
    for f in ("hist", "cnt", "nsat", "min", "max", "sum"):
        v = getattr(res, f)
        assert v.dtype == (torch.int64 if f == "sum" else torch.int32)
        assert np.array_equal(v.cpu().numpy().astype(np.int64), want[f].astype(np.int64)), f
    assert tuple(res.hist.shape) == (n, 4, bins) and tuple(res.sum.shape) == (n, 4)
    if content == "flat-saturated":
        assert (res.nsat == res.cnt).all() and (res.sum == 0).all()
    # a single (H, W) mosaic drops N; the default shift gives max(sat) a bin below the last
    one = gpu_ctx.stats(t[n - 1], bins=bins, sat=sat)
    torch.cuda.synchronize()
    assert (max(sat) >> one.shift) < bins and (one.shift == 0 or (max(sat) >> (one.shift - 1)) >= bins)
    assert tuple(one.raw.shape) == (16 * bins + 96,) and tuple(one.hist.shape) == (4, bins) and tuple(one.cnt.shape) == (4,)
    _check(one, S.stats(imgs[n - 1:], bins, one.shift, sat), "single")


def test_every_bins_shift_and_sat(gpu_ctx):
    H, W, n = 71, 1001, 2
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)
    imgs[1] >>= 4  # a 12-bit frame next to a 16-bit one
    t = _dev16(imgs)
    for bins in (64, 128, 256, 512, 1024, 2048, 4096):
        for shift in ((0, 4, 8, 15) if bins in (64, 256, 4096) else (3,)):
            for sat in SATS:
                res = gpu_ctx.stats(t, bins=bins, shift=shift, sat=sat)
                _check(res, S.stats(imgs, bins, shift, sat), "bins %d shift %d sat %r" % (bins, shift, sat))


def _windows(H, W):
    ws = [None, (H // 2, W // 2, 1, 1), (H - 1, 0, 1, W), (0, W - 1, H, 1), (H // 3, 0, 1, W), (0, W // 3, H, 1)]
    if H > 2 and W > 2:
        ws += [(1, 1, H - 2, W - 2), (1, 0, H - 1, W - 1), (0, 1, H - 1, W - 1), (H // 2 | 1, W // 2 | 1, H - (H // 2 | 1), W - (W // 2 | 1))]
    if W > 300:
        ws += [(3, 9, H - 5, 257), (2, 8, H - 2, W - 16), (0, W - 265, H, 264)]
    return ws


@pytest.mark.parametrize("geom", ((35, 41), (34, 520), (70, 1002), (71, 1001), (1, 64), (33, 1)))
def test_views_and_windows(gpu_ctx, geom):
    H, W = geom
    rng = np.random.default_rng(zlib.crc32(repr(geom).encode()))
    n = 3
    big = rng.integers(0, 1 << 16, size=(2 * n, H + 1, W + 16), dtype=np.uint16)
    tb = _dev16(big)
    flatb = _dev16(np.concatenate([big.ravel(), np.zeros(8, np.uint16)]))
    views = {
        "contiguous": (_dev16(big[:n, :H, :W]), big[:n, :H, :W]),
        "pitched": (tb[:n, :H, 3:3 + W], big[:n, :H, 3:3 + W]),
        "pitched on the 16-byte grid": (tb[:n, 1:H + 1, 8:8 + W], big[:n, 1:H + 1, 8:8 + W]),
        "frame-strided": (tb[::2, :H, :W], big[::2, :H, :W]),
        # the same frames from an address that is 2-byte aligned only
        "base off by one element": (torch.as_strided(flatb.view(torch.int16), (n, H, W), ((H + 1) * (W + 16), W + 16, 1), 1).view(torch.uint16),
                                    np.lib.stride_tricks.as_strided(big.ravel()[1:], (n, H, W), ((H + 1) * (W + 16) * 2, (W + 16) * 2, 2))),
    }
    if W % 8 == 0:  # the contiguous frames themselves sit on the 16-byte grid
        views["frame-strided, contiguous rows"] = (_dev16(big[:, :H, :W])[::2], big[::2, :H, :W])
    k = 0
    for name, (tv, ref) in views.items():
        assert tv.data_ptr() % 2 == 0
        for roi in _windows(H, W):
            bins, shift = BINS_SHIFTS[k % len(BINS_SHIFTS)]
            sat = SATS[k % len(SATS)]
            k += 1
            res = gpu_ctx.stats(tv, bins=bins, shift=shift, sat=sat, roi=roi)
            _check(res, S.stats(np.ascontiguousarray(ref), bins, shift, sat, roi), "%s roi %r" % (name, roi))
    torch.cuda.synchronize()
    assert np.array_equal(_np(tb), big), "the input was written"


def _stats_struct(bins_log2=8, shift=8, roi=(0, 0, 1, 1), sat=(65535,) * 4, flags=0, reserved=0):
    s = M.Stats()
    s.bins_log2, s.shift = bins_log2, shift
    s.y0, s.x0, s.h, s.w = roi
    for i in range(4):
        s.sat[i] = sat[i]
    s.flags, s.reserved = flags, reserved
    return s


def _raw(ctx, s, in_ptr, ip, ifs, w, h, n, out_ptr, out_bytes, stream=None):
    return M.load().mcraw_stats_batch(ctx._h, C.byref(s) if s is not None else None, C.c_void_p(in_ptr), ip, ifs, w, h, n,
                                      C.c_void_p(out_ptr), out_bytes, C.c_void_p(stream))


def test_initialises_its_records_and_nothing_else(gpu_ctx):
    H, W, n, bins, shift = 70, 1002, 3, 256, 8
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)
    t = _dev16(imgs)
    rec, guard = 16 * bins + 96, 4096
    buf = torch.full((guard + n * rec + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    assert (buf.data_ptr() + guard) % 8 == 0
    s = _stats_struct(8, shift, (0, 0, H, W), (60000,) * 4)
    want = S.record(S.stats(imgs, bins, shift, (60000,) * 4))
    for again in range(2):  # the second call into the same out gives the same bytes
        assert _raw(gpu_ctx, s, t.data_ptr(), W, H * W, W, H, n, buf.data_ptr() + guard, n * rec) == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:guard] == 0xA5).all() and (got[guard + n * rec:] == 0xA5).all(), "written outside out_bytes"
        assert np.array_equal(got[guard:guard + n * rec].reshape(n, rec), want), again
    assert np.array_equal(_np(t), imgs), "the input was written"
    # Python: out= is used and initialised by the call
    out = torch.full((n, rec), 0xA5, dtype=torch.uint8, device=DEV)
    res = gpu_ctx.stats(t, bins=bins, shift=shift, sat=60000, out=out)
    assert res.raw is out
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("geom", ((35, 41), (70, 1002), (1080, 1920)))
def test_accumulate(gpu_ctx, geom):
    H, W = geom
    n, bins, shift, sat = 2, 256, 8, (65535, 30000, 65000, 12)
    rng = np.random.default_rng(H)
    a, b = (rng.integers(lo, hi, size=(n, H, W), dtype=np.uint16) for lo, hi in ((100, 1 << 16), (0, 50000)))
    ta, tb = _dev16(a), _dev16(b)
    whole = S.stats(a, bins, shift, sat)
    # two half windows (the second starts on an odd column / row) equal the full window
    cx, cy = W // 2 | 1, H // 2 | 1
    for first, second in (((0, 0, H, cx), (0, cx, H, W - cx)), ((0, 0, cy, W), (cy, 0, H - cy, W))):
        res = gpu_ctx.stats(ta, bins=bins, shift=shift, sat=sat, roi=first)
        res2 = gpu_ctx.stats(ta, bins=bins, shift=shift, sat=sat, roi=second, out=res.raw, accumulate=True)
        assert res2.raw is res.raw
        _check(res2, whole, "halves %r %r" % (first, second))
    # two batches into one set of records: the counts add, min / max combine
    res = gpu_ctx.stats(ta, bins=bins, shift=shift, sat=sat)
    gpu_ctx.stats(tb, bins=bins, shift=shift, sat=sat, out=res.raw, accumulate=True)
    both = S.stats(b, bins, shift, sat, into=whole)
    _check(res, both, "two batches")
    fa, fb = S.stats(a, bins, shift, sat), S.stats(b, bins, shift, sat)
    assert np.array_equal(both["hist"], fa["hist"] + fb["hist"]) and np.array_equal(both["min"], np.minimum(fa["min"], fb["min"]))
    with pytest.raises(ValueError):
        gpu_ctx.stats(ta, accumulate=True)


def test_more_frames_than_one_launch_takes(gpu_ctx):
    n, bins, shift = 65537, 64, 10
    rng = np.random.default_rng(65537)
    imgs = rng.integers(0, 1 << 16, size=(n, 2, 2), dtype=np.uint16)
    sat = (65535, 20000, 65535, 40000)
    res = gpu_ctx.stats(_dev16(imgs), bins=bins, shift=shift, sat=sat)
    # one sample per position: the fields in closed form (checked against the reference on the first and last frames)
    v = imgs.reshape(n, 4).astype(np.int64)
    s = v >= np.asarray(sat)[None, :]
    want = S.empty(n, bins)
    want["hist"][np.arange(n)[:, None], np.arange(4)[None, :], np.minimum(v >> shift, bins - 1)] = 1
    want["cnt"][...] = 1
    want["nsat"][...] = s
    want["min"][...] = v
    want["max"][...] = v
    want["sum"][...] = np.where(s, 0, v)
    for sl in (slice(0, 40), slice(n - 40, n)):
        ref = S.stats(imgs[sl], bins, shift, sat)
        assert all(np.array_equal(ref[f], want[f][sl]) for f in ref)
    _check(res, want, "65537 frames")


def test_queued_call_sees_the_input_of_its_place_in_the_stream(gpu_ctx):
    H, W, n = 70, 1002, 2
    rng = np.random.default_rng(9)
    versions = [rng.integers(0, 1 << (10 + 2 * k), size=(n, H, W), dtype=np.uint16) for k in range(4)]
    staged = [torch.from_numpy(v.view(np.int16)).to(DEV) for v in versions]
    live = torch.empty((n, H, W), dtype=torch.int16, device=DEV)
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s):
        for k in range(4):  # no host sync between: the input is rewritten in stream order between the calls
            live.copy_(staged[k])
            outs.append(gpu_ctx.stats(live.view(torch.uint16), bins=256, shift=8))
    s.synchronize()
    for k, o in enumerate(outs):
        _check(o, S.stats(versions[k], 256, 8), "version %d" % k)


def test_rejections_write_nothing_and_say_why(gpu_ctx):
    w, h, n, rec = 24, 10, 2, 16 * 256 + 96
    buf = torch.full((4 * 16384,), 0xA5, dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    ip, op = base, base + 16384
    assert base % 16 == 0
    good = dict(in_ptr=ip, ip=w, ifs=w * h, w=w, h=h, n=n, out_ptr=op, out_bytes=n * rec)
    full = (0, 0, h, w)

    def call(st=None, **kw):
        a = dict(good)
        a.update(kw)
        st = st if st is not None else _stats_struct(roi=full)
        return _raw(gpu_ctx, st, a["in_ptr"], a["ip"], a["ifs"], a["w"], a["h"], a["n"], a["out_ptr"], a["out_bytes"])

    cases = [
        ("no struct", lambda: _raw(gpu_ctx, None, ip, w, w * h, w, h, n, op, n * rec)),
        ("NULL in", lambda: call(in_ptr=0)),
        ("NULL out", lambda: call(out_ptr=0)),
        ("odd in", lambda: call(in_ptr=ip + 1)),
        ("out off the 8-byte grid by 4", lambda: call(out_ptr=op + 4)),
        ("out off the 8-byte grid by 1", lambda: call(out_ptr=op + 1)),
        ("width 0", lambda: call(w=0)),
        ("width 65537", lambda: call(w=65537, ip=65537, n=1)),
        ("negative width", lambda: call(w=-4)),
        ("height 0", lambda: call(h=0)),
        ("height 65537", lambda: call(h=65537, n=1)),
        ("pitch below width", lambda: call(ip=w - 1)),
        ("frame stride too small", lambda: call(ifs=(h - 1) * w + w - 1)),
        ("bins_log2 5", lambda: call(_stats_struct(5, roi=full))),
        ("bins_log2 13", lambda: call(_stats_struct(13, roi=full), out_bytes=4 * 16384)),
        ("shift 16", lambda: call(_stats_struct(8, 16, roi=full))),
        ("w 0", lambda: call(_stats_struct(roi=(0, 0, h, 0)))),
        ("h 0", lambda: call(_stats_struct(roi=(0, 0, 0, w)))),
        ("window past the right edge", lambda: call(_stats_struct(roi=(0, 1, h, w)))),
        ("window past the bottom edge", lambda: call(_stats_struct(roi=(1, 0, h, w)))),
        ("x0 behind the frame", lambda: call(_stats_struct(roi=(0, w, h, 1)))),
        ("x0 + w wraps around", lambda: call(_stats_struct(roi=(0, 8, h, 0xFFFFFFFF - 3)))),
        ("y0 + h wraps around", lambda: call(_stats_struct(roi=(0xFFFFFFFF, 0, 2, w)))),
        ("unknown flag", lambda: call(_stats_struct(roi=full, flags=2))),
        ("unknown flag next to the known one", lambda: call(_stats_struct(roi=full, flags=0x80000001))),
        ("reserved", lambda: call(_stats_struct(roi=full, reserved=1))),
        ("out_bytes one short", lambda: call(out_bytes=n * rec - 1)),
        ("out_bytes of one record", lambda: call(out_bytes=rec)),
        ("negative n", lambda: call(n=-1)),
        ("out starts inside the input", lambda: call(out_ptr=ip + 16)),
        ("out ends inside the input", lambda: call(in_ptr=op + n * rec - 8)),
        ("out around the input", lambda: call(in_ptr=op + 64)),
    ]
    serial = gpu_ctx.last_serial()
    for name, fn in cases:
        rc = fn()
        assert rc < 0, name
        msg = M.load().mcraw_last_error().decode()
        assert msg.startswith("mcraw_stats_batch: ") and len(msg) > len("mcraw_stats_batch: "), name
    assert call(n=0) == 0  # n == 0: a no-op
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all()
    assert gpu_ctx.last_serial() == serial
    # a good call next to them does write: out directly behind the input's last sample, out_bytes to the byte
    assert call(out_ptr=ip + 2 * n * w * h) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    img = np.full((n, h, w), 0xA5A5, np.uint16)
    lo = 2 * n * w * h
    assert np.array_equal(got[lo:lo + n * rec].reshape(n, rec), S.record(S.stats(img, 256, 8)))
    assert (got[:lo] == 0xA5).all() and (got[lo + n * rec:] == 0xA5).all()
    # Python: what the wrapper checks itself
    t = torch.zeros((2, 8, 8), dtype=torch.int16, device=DEV).view(torch.uint16)
    for kw in (dict(bins=100), dict(bins=32), dict(bins=8192), dict(sat=(1, 2, 3)), dict(sat=70000), dict(roi=(0, 0, 9, 8)),
               dict(roi=(0, 7, 8, 2)), dict(roi=(0, 0, 0, 8)), dict(out=torch.zeros((2, 100), dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            gpu_ctx.stats(t, **kw)
    with pytest.raises(ValueError):
        gpu_ctx.stats(t.view(torch.int16))
    with pytest.raises(M.McrawError, match="mcraw_stats_batch: .*shift"):
        gpu_ctx.stats(t, shift=16)


def _frames(rng, shapes, typ):
    items = []
    for (w, h) in shapes:
        img = L.natural_image_np(w, h, 12, 12.0, int(rng.integers(1 << 30)))
        buf = L.encode7(img) if typ == 7 else L.encode6(img)
        ret, want = (L.oracle_decode7 if typ == 7 else L.oracle_decode6)(buf, w, h)
        assert ret == w * h
        items.append((buf, want))
    return items


@pytest.mark.parametrize("typ", (7, 6))
def test_decode_stats_and_decode_state(gpu_ctx, typ):
    rng = np.random.default_rng(typ)
    w, h = 512, 96
    items = _frames(rng, [(w, h)] * 3, typ)
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    imgs = np.stack([want for _, want in items])
    kw = dict(bins=1024, sat=(4095, 4000, 4095, 3000), roi=(1, 3, h - 2, w - 7))

    def decode():
        o = torch.full((w * h,), 0x5A5A, dtype=torch.int16, device=DEV)
        written, status = gpu_ctx.decode_batch(M.Context.make_frames([(ins[0].data_ptr(), ins[0].numel(), w, h, typ, o.data_ptr(), w * h * 2)]))
        assert status == [0]
        return o

    s0 = gpu_ctx.last_serial()
    before = decode()
    s1 = gpu_ctx.last_serial()
    errs = gpu_ctx.errors(reset=False)
    res = gpu_ctx.decode_stats(ins, w, h, typ, **kw)
    torch.cuda.synchronize()
    s2 = gpu_ctx.last_serial()
    assert s2 - s1 == s1 - s0  # the decode took its serial; the statistics took none
    assert res.shift == 2 and res.bins == 1024
    _check(res, S.stats(imgs, 1024, 2, kw["sat"], kw["roi"]), "decode_stats")
    # ... and equals stats() of the decoded mosaics, which takes no serial at all
    direct = gpu_ctx.stats(_dev16(imgs), **kw)
    torch.cuda.synchronize()
    assert torch.equal(direct.raw, res.raw)
    assert gpu_ctx.last_serial() == s2 and gpu_ctx.errors(reset=False) == errs
    after = decode()
    torch.cuda.synchronize()
    assert gpu_ctx.last_serial() - s2 == s1 - s0
    assert torch.equal(before, after) and np.array_equal(after.cpu().numpy().view(np.uint16).reshape(h, w), imgs[0])
    assert gpu_ctx.errors() == 0


def test_white_balance_from_the_gpu_record(gpu_ctx):
    rng = np.random.default_rng(21)
    n, H, W = 3, 70, 1002
    black = (64, 66, 62, 65)
    imgs = np.empty((n, H, W), np.uint16)
    for p, level in enumerate((1000, 2000, 2100, 750)):  # rggb: a greenish cast with noise on top
        imgs[:, p >> 1::2, p & 1::2] = np.clip(rng.normal(level, 300, size=imgs[:, p >> 1::2, p & 1::2].shape) + black[p], 0, 4094)
    imgs[:, 0:2, 0:2] = 4095  # one clipped sample per position and frame
    res = gpu_ctx.stats(_dev16(imgs), bins=256, sat=4095)
    torch.cuda.synchronize()
    want = S.stats(imgs, 256, res.shift, (4095,) * 4)
    _check(res, want, "white balance input")
    ref = S.helper_input(want, 256, res.shift)
    for cfa in ("rggb", "grbg"):
        g = M.stats_white_balance(res, black=black, cfa=cfa)
        assert np.array_equal(g, M.stats_white_balance(ref, black=black, cfa=cfa)) and g.shape == (n, 3)
    g = M.stats_white_balance(res, black=black)
    assert (g[:, 1] == 1).all() and (g[:, 0] > 1.5).all() and (g[:, 2] > 2).all()
    assert (res.nsat == 1).all()
    assert np.array_equal(M.stats_percentile(res, 0.99), M.stats_percentile(ref, 0.99))
    assert np.array_equal(M.stats_clipped(res), M.stats_clipped(ref)) and (M.stats_clipped(res) > 0).all()
    # the gains are what the demosaic takes: the channel means of the white-balanced frame agree.  (The black levels differ by
    # up to 4 in a range of about 4000 and one sample in 175,000 is clipped: 5e-3 leaves room for how the demosaic normalises.)
    rgb = gpu_ctx.demosaic(_dev16(imgs), algo="bin2", dtype="f32", white=float(M.stats_percentile(res, 1.0).max()), black=black,
                           gain=g.astype(np.float32))
    torch.cuda.synchronize()
    m = rgb.mean(dim=(2, 3)).cpu().numpy()
    assert np.allclose(m[:, 0] / m[:, 1], 1.0, atol=5e-3) and np.allclose(m[:, 2] / m[:, 1], 1.0, atol=5e-3)
