"""Per-frame global shifts of mosaics (mcraw_align_batch, Context.align) on the GPU: pos and sad equal the numpy statement of the
contract (_align_ref) bit for bit, the result is what merge() takes, rejected calls write nothing and say why, and calls queued
back to back keep their order."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _align_ref as R
import _merge_ref as MR
import motioncam_decoder_amd as M
from _align_scenes import clamp_frames, scene_frames

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BLACK = (64, 64, 64, 64)
# (H, W), levels, radius, blur of the scene.  The SAD kernel's tile is 128 x 32 pixels of a level's window, the pyramid kernel's
# 256 x 64 samples of the mosaic (levels 0 .. 2 in one pass, one more launch per level above).
CASES = (((6, 6), 1, 1, 3),        # the smallest legal call: a 1 x 1 window
         ((7, 9), 1, 1, 3),        # odd sizes
         ((24, 24), 1, 2, 9), ((40, 48), 2, 2, 9), ((72, 136), 3, 2, 17), ((130, 70), 3, 2, 17),  # the recovery scenes
         ((150, 1030), 1, 2, 9),   # a quad plane wider and higher than one tile of either kernel, cropped last tiles
         ((150, 1030), 2, 2, 9),   # ... with a refinement level over several tiles
         ((256, 256), 4, 2, 33),   # a level above the pyramid kernel's own three
         ((260, 264), 6, 1, 9),    # every level there is, windows of 2 .. 4 pixels
         ((70, 74), 1, 8, 9))      # the widest search: 289 candidates


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _same(got, want, what):
    pos, sad = got
    assert pos.dtype == torch.int16 and tuple(pos.shape) == want[0].shape and pos.is_contiguous(), what
    assert sad.dtype == torch.int64 and tuple(sad.shape) == want[1].shape, what
    gp, gs = pos.cpu().numpy(), sad.cpu().numpy()
    assert np.array_equal(gp, want[0]), (what, gp.tolist(), want[0].tolist())
    assert np.array_equal(gs, want[1].astype(np.int64)), (what, gs.tolist(), want[1].tolist())


@pytest.mark.parametrize("case", CASES)
def test_align_matches_reference(gpu_ctx, case):
    (H, W), levels, radius, k = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
    n = 5
    scene, off = scene_frames(H * 7 + W, H, W, levels, radius, k, n)
    contents = (("scene", scene, BLACK), ("full", rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16), (0, 0, 0, 0)),
                ("ties", (rng.integers(0, 8, size=(n, H, W)) * 100).astype(np.uint16), (64, 60, 70, 65535)))
    for name, imgs, black in contents:
        t = _dev16(imgs)
        for ref in (None, 0, 2, 4):  # the chain, and the anchor first, in the middle and last
            got = gpu_ctx.align(t, black=black, levels=levels, radius=radius, ref=ref, sad=True)
            torch.cuda.synchronize()
            _same(got, R.align(imgs, black, levels, radius, -1 if ref is None else ref), (name, ref))
        for m in (1, 2):  # n = 1 writes (0, 0); n = 2 is one pair
            got = gpu_ctx.align(t[:m], black=black, levels=levels, radius=radius, sad=True)
            torch.cuda.synchronize()
            _same(got, R.align(imgs[:m], black, levels, radius), (name, "n", m))
        assert np.array_equal(t.view(torch.int16).cpu().numpy().view(np.uint16), imgs), "the input was written"
    if k >= 2 ** (levels + 1) + 1 and min(H, W) >= 24:  # the recovery scenes: the stage finds the crops' offsets
        pos = gpu_ctx.align(_dev16(scene), black=BLACK, levels=levels, radius=radius)
        assert isinstance(pos, torch.Tensor)
        assert np.array_equal(np.diff(pos.cpu().numpy().astype(np.int64), axis=0), off[:-1] - off[1:])
    empty = gpu_ctx.align(_dev16(scene)[:0], levels=levels, radius=radius, sad=True)  # n == 0
    assert tuple(empty[0].shape) == (0, 2) and tuple(empty[1].shape) == (0,)


def test_sums_beyond_32_bits(gpu_ctx):
    """A window of 258 x 258 differences of 65535: above 2^32, for every candidate, so (0, 0) wins the tie."""
    imgs = np.zeros((2, 520, 520), np.uint16)
    imgs[0] = 65535
    got = gpu_ctx.align(_dev16(imgs), levels=1, radius=1, sad=True)
    torch.cuda.synchronize()
    assert got[0].cpu().tolist() == [[0, 0], [0, 0]]
    assert got[1].cpu().tolist() == [0, 258 * 258 * 65535] and 258 * 258 * 65535 > 1 << 32
    _same(got, R.align(imgs, (0, 0, 0, 0), 1, 1), "2^32")


def test_flat_and_identical_frames(gpu_ctx):
    H, W, levels, radius = 72, 136, 3, 2
    wh, ww = M.align_window(H, W, levels, radius)
    flat = np.stack([np.full((H, W), v, np.uint16) for v in (1000, 1300, 200)])
    for ref, diffs in ((None, (0, 300, 1100)), (1, (300, 0, 1100))):
        pos, sad = gpu_ctx.align(_dev16(flat), levels=levels, radius=radius, ref=ref, sad=True)
        torch.cuda.synchronize()
        assert not pos.cpu().numpy().any() and sad.cpu().tolist() == [d * wh * ww for d in diffs]
    img = np.random.default_rng(8).integers(0, 1 << 16, size=(H, W), dtype=np.uint16)
    pos, sad = gpu_ctx.align(_dev16(np.stack([img] * 4)), levels=levels, radius=radius, sad=True)
    torch.cuda.synchronize()
    assert not pos.cpu().numpy().any() and not sad.cpu().numpy().any()
    pos, sad = gpu_ctx.align(_dev16(np.stack([img >> 4] * 2)), black=(4096,) * 4, levels=levels, radius=radius, sad=True)  # black above the samples
    torch.cuda.synchronize()
    assert not pos.cpu().numpy().any() and not sad.cpu().numpy().any()


def test_the_clamp(gpu_ctx):
    n = 2100
    frames, off = clamp_frames(n)
    want = R.align(frames, BLACK, 1, 8)
    assert np.array_equal(want[0][:, 1], np.maximum(-16 * np.arange(n), -32768)) and want[0][-1, 1] == -32768
    got = gpu_ctx.align(_dev16(frames), black=BLACK, levels=1, radius=8, sad=True)
    torch.cuda.synchronize()
    _same(got, want, "clamp")


def _strided(base, n, h, w, fstride, pitch, off):
    return torch.as_strided(base, (n, h, w), (fstride, pitch, 1), off).view(torch.uint16)


# (H, W, pitch, frame slack, offset in samples): 1 = an odd base in samples (off the dword grid), 4 = on the 8-byte grid only, 8
# with a pitch and a stride that are multiples of 8 = the 16-byte path
VIEWS = ((72, 136, 149, 29, 1), (72, 136, 136, 0, 4), (72, 136, 144, 8, 8), (41, 47, 53, 5, 3), (150, 1030, 1031, 1, 0))


@pytest.mark.parametrize("view", VIEWS)
def test_pitched_strided_offset_views(gpu_ctx, view):
    H, W, pitch, slack, off = view
    rng = np.random.default_rng(zlib.crc32(repr(view).encode()))
    n, levels, radius = 4, 2, 2
    fs = H * pitch + slack
    imgs = scene_frames(H + W, H, W, levels, radius, 9, n)[0]
    base = torch.from_numpy(rng.integers(0, 1 << 16, size=n * fs + 64, dtype=np.uint16).view(np.int16)).to(DEV)
    src = _strided(base, n, H, W, fs, pitch, off)
    src.view(torch.int16).copy_(torch.from_numpy(imgs.view(np.int16)).to(DEV))
    before = base.clone()
    for ref in (None, 3):
        got = gpu_ctx.align(src, black=BLACK, levels=levels, radius=radius, ref=ref, sad=True)
        torch.cuda.synchronize()
        _same(got, R.align(imgs, BLACK, levels, radius, -1 if ref is None else ref), ref)
    assert torch.equal(base, before), "the input was written"


def test_merge_takes_the_result(gpu_ctx):
    H, W, levels, radius = 96, 200, 3, 2
    frames, off = scene_frames(5, H, W, levels, radius, 17)
    t = _dev16(frames)
    lut, shift = M.noise_lut(S=2e-4, O=2e-6, black=64, white=4095)
    pos = gpu_ctx.align(t, black=BLACK, levels=levels, radius=radius)
    out = gpu_ctx.merge(t, lut, shift, pos=pos)
    st = gpu_ctx.stack(t, lut, shift, ref=2, pos=gpu_ctx.align(t, black=BLACK, levels=levels, radius=radius, ref=2))
    torch.cuda.synchronize()
    want_pos = R.align(frames, BLACK, levels, radius)[0]
    assert np.array_equal(np.diff(want_pos.astype(np.int64), axis=0), off[:-1] - off[1:])
    assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), MR.merge(frames, lut, shift, pos=want_pos))
    want_st = MR.merge(frames, lut, shift, 2, 2, 2, 1, pos=R.align(frames, BLACK, levels, radius, 2)[0])[0]
    assert np.array_equal(st.view(torch.int16).cpu().numpy().view(np.uint16), want_st)
    assert not np.array_equal(want_st, MR.merge(frames, lut, shift, 2, 2, 2, 1)[0])  # the positions matter


def test_calls_back_to_back_keep_their_order(gpu_ctx):
    H, W, levels, radius = 150, 1030, 2, 2
    a = scene_frames(21, H, W, levels, radius, 9, 6)[0]
    b = scene_frames(22, H, W, levels, radius, 9, 6)[0]
    wa, wb = R.align(a, BLACK, levels, radius), R.align(b, BLACK, levels, radius)
    assert not np.array_equal(wa[0], wb[0])
    ta, tb = _dev16(a), _dev16(b)
    torch.cuda.synchronize()
    kw = dict(black=BLACK, levels=levels, radius=radius, sad=True)
    outs = [gpu_ctx.align(ta, **kw), gpu_ctx.align(tb, **kw), gpu_ctx.align(ta, **kw)]  # the null stream: the context's side stream
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream(DEV).cuda_stream == s.cuda_stream != 0
        outs += [gpu_ctx.align(tb, **kw), gpu_ctx.align(ta, **kw), gpu_ctx.align(tb, **kw)]  # no host sync between
    s.synchronize()
    torch.cuda.synchronize()
    for got, want in zip(outs, (wa, wb, wa, wb, wa, wb)):
        _same(got, want, "order")


def _struct(levels=1, radius=1, ref=-1, reserved=0, black=(0, 0, 0, 0), pos=0, sad=0, work=0, work_bytes=0):
    a = M.Align()
    a.levels, a.radius, a.ref, a.reserved = levels, radius, ref, reserved
    for i in range(4):
        a.black[i] = black[i]
    a.pos, a.sad, a.work, a.work_bytes = pos or None, sad or None, work or None, work_bytes
    return a


def test_rejections_write_nothing_and_say_why(gpu_ctx):
    lib = M.load()
    w, h, n = 24, 10, 3
    SENT = 0x5A
    buf = torch.full((1 << 16,), SENT, dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    assert base % 256 == 0
    ip, pp, sp, kp = base, base + 4096, base + 8192, base + 16384
    need = lib.mcraw_align_work_bytes(w, h, n, 1, 1)
    assert 0 < need <= (1 << 16) - 16384
    good = dict(in_ptr=ip, ip=w, ifs=w * h, w=w, h=h, n=n)

    def call(st=None, **kw):
        a = dict(good)
        a.update(kw)
        st = st if st is not None else _struct(pos=pp, sad=sp, work=kp, work_bytes=need)
        return lib.mcraw_align_batch(gpu_ctx._h, C.byref(st), C.c_void_p(a["in_ptr"]), a["ip"], a["ifs"], a["w"], a["h"], a["n"], None)

    S = lambda **kw: _struct(**dict(dict(pos=pp, sad=sp, work=kp, work_bytes=need), **kw))
    cases = [
        ("no struct", lambda: lib.mcraw_align_batch(gpu_ctx._h, None, C.c_void_p(ip), w, w * h, w, h, n, None)),
        ("NULL in", lambda: call(in_ptr=0)),
        ("odd in", lambda: call(in_ptr=ip + 1)),
        ("NULL pos", lambda: call(S(pos=0))),
        ("odd pos", lambda: call(S(pos=pp + 1))),
        ("sad on the 4-byte grid only", lambda: call(S(sad=sp + 4))),
        ("NULL work", lambda: call(S(work=0))),
        ("work on the 8-byte grid only", lambda: call(S(work=kp + 8))),
        ("work_bytes one short", lambda: call(S(work_bytes=need - 1))),
        ("work_bytes 0", lambda: call(S(work_bytes=0))),
        ("levels 0", lambda: call(S(levels=0))),
        ("levels 7", lambda: call(S(levels=7))),
        ("radius 0", lambda: call(S(radius=0))),
        ("radius 9", lambda: call(S(radius=9))),
        ("ref -2", lambda: call(S(ref=-2))),
        ("ref n", lambda: call(S(ref=n))),
        ("reserved", lambda: call(S(reserved=1))),
        ("width 0", lambda: call(w=0)),
        ("height 65537", lambda: call(h=65537, n=1)),
        ("negative n", lambda: call(n=-1)),
        ("pitch below width", lambda: call(ip=w - 1)),
        ("frame stride too small", lambda: call(ifs=w * h - 1)),
        ("an empty window: height 5", lambda: call(h=5)),
        ("an empty window: radius 3 on 5 quad rows", lambda: call(S(radius=3))),
        ("an empty window at the second level", lambda: call(S(levels=2))),
        ("pos inside the input", lambda: call(S(pos=ip + 64))),
        ("sad inside the input", lambda: call(S(sad=ip + 2 * n * w * h - 8))),
        ("work inside the input", lambda: call(S(work=ip + 16))),
        ("the input ends inside work", lambda: call(in_ptr=kp - 64)),
        ("pos inside work", lambda: call(S(pos=kp + 32))),
        ("sad inside work", lambda: call(S(sad=kp + need - 8))),
        ("pos and sad overlap", lambda: call(S(sad=pp + 8))),
    ]
    serial = gpu_ctx.last_serial()
    for name, fn in cases:
        rc = fn()
        assert rc < 0, name
        msg = lib.mcraw_last_error().decode()
        assert msg.startswith("mcraw_align_batch: ") and len(msg) > len("mcraw_align_batch: "), name
    assert call(n=0) == 0 and call(_struct(), n=0) == 0  # n == 0: a no-op
    torch.cuda.synchronize()
    gpu_ctx.synchronize()
    assert (buf.cpu().numpy() == SENT).all()
    assert gpu_ctx.last_serial() == serial
    # a good call next to them does write: pos, sad and nothing outside its three areas
    imgs = scene_frames(3, h, w, 1, 1, 3, n)[0]
    buf[:2 * n * w * h].copy_(torch.from_numpy(imgs.reshape(-1).view(np.uint8)).to(DEV))
    for ref, with_sad in ((-1, True), (1, False), (-1, True)):
        assert call(S(ref=ref, black=BLACK, sad=sp if with_sad else 0)) == 0
        torch.cuda.synchronize()
        a = buf.cpu().numpy()
        want = R.align(imgs, BLACK, 1, 1, ref)
        assert np.array_equal(a[4096:4096 + 4 * n].view(np.int16).reshape(n, 2), want[0])
        if with_sad:
            assert np.array_equal(a[8192:8192 + 8 * n].view(np.uint64), want[1])
        else:
            assert (a[8192:8192 + 8 * n] == SENT).all()
        assert (a[2 * n * w * h:4096] == SENT).all() and (a[4096 + 4 * n:8192] == SENT).all() and (a[8192 + 8 * n:16384] == SENT).all()
        assert (a[16384 + need:] == SENT).all()
        assert np.array_equal(a[:2 * n * w * h].view(np.uint16).reshape(n, h, w), imgs)
        buf[4096:].fill_(SENT)
    assert call(S(black=BLACK), n=1) == 0  # n == 1 writes (0, 0) and sad 0
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert not a[4096:4100].any() and not a[8192:8200].any() and (a[4100:8192] == SENT).all() and (a[8200:16384] == SENT).all()
    assert gpu_ctx.last_serial() == serial and gpu_ctx.errors(reset=False) == 0
    # Python: what the wrapper checks itself
    t = torch.zeros((3, 24, 24), dtype=torch.int16, device=DEV).view(torch.uint16)
    for kw in (dict(levels=0), dict(levels=7), dict(levels=1.5), dict(radius=0), dict(radius=9), dict(ref=3), dict(ref=-1), dict(ref=0.5),
               dict(black=(1, 2, 3)), dict(black=-1), dict(black=(0, 0, 0, 65536)), dict(black=0.5), dict(levels=3, radius=2)):
        with pytest.raises(ValueError):
            gpu_ctx.align(t, **kw)
    for bad in (t.view(torch.int16), t[0], t.cpu()):
        with pytest.raises(ValueError):
            gpu_ctx.align(bad)
    ok = gpu_ctx.align(t, black=64, levels=np.int64(1), radius=np.int32(2), ref=np.int64(1))
    torch.cuda.synchronize()
    assert tuple(ok.shape) == (3, 2) and not ok.cpu().numpy().any()


def test_decode_merge_with_align(gpu_ctx):
    """decode_merge(align={...}) is the decode, the estimate and the merge in one call; without the keyword it is what it was."""
    import _libs as L
    w, h, n, levels, radius = 512, 96, 4, 2, 2
    scene = L.natural_image_np(w + 64, h + 64, 12, 12.0, 9)
    offs = ((16, 16), (20, 10), (14, 22), (18, 18))
    imgs = np.stack([scene[oy:oy + h, ox:ox + w] for oy, ox in offs])
    ins = [torch.from_numpy(L.encode7(f)).to(DEV) for f in imgs]
    lut, shift = M.noise_lut(S=2e-4, O=2e-6, black=64, white=4095)
    want_pos = R.align(imgs, BLACK, levels, radius)[0]
    assert want_pos[1:].any(axis=1).all()
    try:
        got = gpu_ctx.decode_merge(ins, w, h, 7, lut=lut, shift=shift, before=1, after=2, align=dict(black=BLACK, levels=levels, radius=radius))
        plain = gpu_ctx.decode_merge(ins, w, h, 7, lut=lut, shift=shift, before=1, after=2)
        torch.cuda.synchronize()
        bits = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(bits(got), MR.merge(imgs, lut, shift, 1, 2, pos=want_pos))
        assert np.array_equal(bits(plain), MR.merge(imgs, lut, shift, 1, 2))
        for bad in (dict(align=dict(sad=True)), dict(align=3), dict(align=dict(levels=levels), pos=want_pos)):
            with pytest.raises(ValueError):
                gpu_ctx.decode_merge(ins, w, h, 7, lut=lut, shift=shift, **bad)
    finally:
        gpu_ctx.set_post()
    assert gpu_ctx.errors() == 0
