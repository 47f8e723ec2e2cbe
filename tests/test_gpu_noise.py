"""The noise measurement (mcraw_noise_batch, Context.noise_stats, decode_noise_stats, estimate_noise) on the GPU: every record equals
the numpy statement of the contract (_noise_ref) byte for byte -- everything is an integer, so there is no tolerance --, the call
initialises its records itself and writes nothing around them, the input is left as it was, accumulation adds up, a repeated call
gives the same bytes, and the profile that estimate_noise fits feeds noise_lut and denoise()."""
import os

import numpy as np
import pytest
import torch

import _libs as L
import _noise_ref as NR
import _paths_harness as PH
import motioncam_decoder_amd as M
from motioncam_decoder_amd import build as B

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENT = 4096, 0xA5


def _np(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _run(ctx, t, n, shift, want=None, what="", **kw):
    """noise_stats(t, shift=shift, **kw) into records with sentinels around them; compares with `want` (the statement's fields)
    unless None.  Returns the records' bytes."""
    buf = torch.full((GUARD + n * NR.REC_BYTES + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 8 == 0
    out = buf[GUARD:GUARD + n * NR.REC_BYTES].view(n, NR.REC_BYTES)
    res = ctx.noise_stats(t, shift=shift, out=out, **kw)
    torch.cuda.synchronize()
    assert isinstance(res, M.NoiseStats) and res.raw.data_ptr() == out.data_ptr() and res.shift == shift
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENT).all() and (host[-GUARD:] == SENT).all(), what + ": written outside the records"
    got = host[GUARD:-GUARD].reshape(n, NR.REC_BYTES)
    if want is not None:
        _same(got, want, what)
        assert np.array_equal(res.hist.cpu().numpy().view(np.uint32), want["hist"])
        assert np.array_equal(res.nblk.cpu().numpy().view(np.uint32), want["nblk"])
        assert np.array_equal(res.nrej.cpu().numpy().view(np.uint32), want["nrej"])
    return got.copy()


def _same(got, want, what):
    exp = NR.record(want)
    if not np.array_equal(got, exp):
        g, e = got.view("<u4"), exp.view("<u4")
        bad = np.argwhere(g != e)[:5]
        raise AssertionError("%s: records differ at (frame, word) %s: got %s, want %s"
                             % (what, bad.tolist(), [int(g[tuple(b)]) for b in bad], [int(e[tuple(b)]) for b in bad]))


def _noise_images(rng, n, H, W, bits=12):
    """Smooth levels with noise of a few DN on top and a few outliers: several level bins, many energy bins."""
    yy, xx = np.mgrid[0:H, 0:W]
    top = (1 << bits) - 1
    base = (xx * (top - 200) // max(W - 1, 1) + 40 + 3 * yy)[None] + rng.integers(0, 300, size=(n, 1, 1))
    sig = rng.integers(1, 60, size=(n, 1, 1))
    img = base + np.rint(rng.standard_normal((n, H, W)) * sig).astype(np.int64)
    img[rng.random((n, H, W)) < 0.001] = top
    return np.clip(img, 0, top).astype(np.uint16)


@pytest.mark.parametrize("geom", ((16, 16), (32, 48), (48, 1040), (32, 2064), (18, 4112)))
def test_whole_frames(gpu_ctx, geom):
    """One block; a few; a partial last strip (1040 = 64 blocks + 1); two full strips and a partial one; five strips across."""
    H, W = geom
    rng = np.random.default_rng(H * 10007 + W)
    imgs = _noise_images(rng, 2, H, W)
    t = _dev16(imgs)
    sat, lo = (4095, 4000, 4095, 3900), (1, 0, 30, 1)
    want = NR.noise_stats(imgs, 7, sat, lo)
    assert int(want["nblk"].sum() + want["nrej"].sum()) == 2 * 4 * (H // 16) * (W // 16)
    _run(gpu_ctx, t, 2, 7, want, "%d x %d" % geom, sat=sat, lo=lo)
    assert np.array_equal(_np(t), imgs), "the input was written"
    # a single (H, W) mosaic drops N; the default shift keeps max(sat) below level bin 32
    one = gpu_ctx.noise_stats(t[1], sat=sat, lo=lo)
    torch.cuda.synchronize()
    assert one.shift == 7 and tuple(one.raw.shape) == (NR.REC_BYTES,) and tuple(one.hist.shape) == (4, 32, 128)
    _same(one.raw.cpu().numpy()[None], NR.noise_stats(imgs[1:], 7, sat, lo), "single")


def test_window_with_partial_blocks(gpu_ctx):
    """272 x 48 with the window (2, 2, 260, 40): blocks off the 16-byte grid, 4 rows and 8 columns that belong to no block.  Those
    and everything outside the window hold 65535, which would reject every block that read it."""
    rng = np.random.default_rng(3)
    H, W, roi = 272, 48, (2, 2, 260, 40)
    imgs = _noise_images(rng, 3, H, W)
    keep = np.zeros((H, W), bool)
    keep[2:2 + 256, 2:2 + 32] = True
    imgs[:, ~keep] = 65535
    want = NR.noise_stats(imgs, 7, 4096, 0, roi)
    assert (want["nblk"] > 0).all() and int((want["nblk"] + want["nrej"])[0, 0]) == 16 * 2
    _run(gpu_ctx, _dev16(imgs), 3, 7, want, "roi", sat=4096, roi=roi)


def test_unaligned_and_strided_views(gpu_ctx):
    """A base 2 bytes off the 16-byte grid with an odd pitch (the unaligned 16-byte loads), and a view with strided rows and frames."""
    rng = np.random.default_rng(4)
    n, H, W = 3, 34, 100
    imgs = _noise_images(rng, n, H, W)
    want = NR.noise_stats(imgs, 7, 4095, 1)
    pitch, fstride = W + 3, (W + 3) * H + 11
    flat = torch.zeros((1 + n * fstride + 16,), dtype=torch.int16, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = torch.as_strided(flat, (n, H, W), (fstride, pitch, 1), 1)
    view.copy_(torch.from_numpy(imgs.view(np.int16)).to(DEV))
    before = flat.clone()
    _run(gpu_ctx, view.view(torch.uint16), n, 7, want, "odd base and pitch", sat=4095, lo=1)
    assert torch.equal(flat, before), "the input was written"
    big = _dev16(np.zeros((2 * n, H + 5, W + 28), np.uint16))
    sub = big[::2, 2:2 + H, 8:8 + W]
    sub.copy_(_dev16(imgs))
    _run(gpu_ctx, sub, n, 7, want, "strided view", sat=4095, lo=1)


def test_flat_extreme_and_rejected_frames(gpu_ctx):
    H, W = 48, 80
    flat = np.full((1, H, W), 1234, np.uint16)
    want = NR.noise_stats(flat, 7, 65535, 0)
    assert int(want["hist"][0, :, 1234 >> 7, 0].sum()) == 4 * 15 == int(want["hist"].sum())  # every lane on one counter per position
    _run(gpu_ctx, _dev16(flat), 1, 7, want, "flat")
    # samples alternating 0 / 65535 along both axes of every plane: the largest T, 64-bit sums, the last energy bin
    yy, xx = np.mgrid[0:H, 0:W]
    ext = ((((yy >> 1) + (xx >> 1)) & 1) * 65535).astype(np.uint16)[None]
    want = NR.noise_stats(ext, 11, 0, 0)
    assert int(want["nrej"].sum()) == 60 and int(want["hist"].sum()) == 0  # sat = 0 rejects everything
    _run(gpu_ctx, _dev16(ext), 1, 11, want, "sat 0", sat=0)
    want = NR.noise_stats(ext, 11, (65535, 65535, 0, 65535), 0)  # ... 65535 itself is >= sat: every block again
    assert int(want["nrej"].sum()) == 60
    _run(gpu_ctx, _dev16(ext), 1, 11, want, "sat 65535", sat=(65535, 65535, 0, 65535))
    ext2 = (ext // 65535 * 65534).astype(np.uint16)
    want = NR.noise_stats(ext2, 11, 65535, 0)
    assert int(want["hist"][..., 127].sum()) == 60 and int(want["nblk"].sum()) == 60
    _run(gpu_ctx, _dev16(ext2), 1, 11, want, "extreme")
    # lo rejects the darker half of the frame
    rng = np.random.default_rng(6)
    img = _noise_images(rng, 1, 64, 64)
    img[:, :, :32] = np.minimum(img[:, :, :32], 90)
    img[:, :, 32:] = np.maximum(img[:, :, 32:], 100)
    want = NR.noise_stats(img, 7, 65535, 100)
    assert (want["nrej"] == 8).all() and (want["nblk"] == 8).all()
    _run(gpu_ctx, _dev16(img), 1, 7, want, "lo", lo=100)


def test_many_frames_accumulate_and_repeat(gpu_ctx):
    """35 frames of 64 x 272 with contents of their own: several frames per launch, a workgroup per frame that walks its four strips
    in two rounds.  Then twice with accumulate=True (the sum), and a repeated call (the same bytes)."""
    rng = np.random.default_rng(7)
    n, H, W = 35, 64, 272
    imgs = _noise_images(rng, n, H, W)
    imgs[5] = 777
    t = _dev16(imgs)
    want = NR.noise_stats(imgs, 7, 4095, 1)
    assert len({want["hist"][f].tobytes() for f in range(n)}) == n
    first = _run(gpu_ctx, t, n, 7, want, "35 frames", sat=4095, lo=1)
    again = _run(gpu_ctx, t, n, 7, None, sat=4095, lo=1)
    assert np.array_equal(first, again)
    acc = torch.from_numpy(first).to(DEV)
    other = np.ascontiguousarray(imgs[::-1])
    for src in (t, _dev16(other)):
        res = gpu_ctx.noise_stats(src, shift=7, sat=4095, lo=1, out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert res.raw.data_ptr() == acc.data_ptr()
    _same(acc.cpu().numpy(), NR.add(NR.add(want, want), NR.noise_stats(other, 7, 4095, 1)), "accumulate")
    with pytest.raises(ValueError):
        gpu_ctx.noise_stats(t, accumulate=True)
    for roi in ((1, 0, 32, 32), (0, 2, 15, 32), (0, 0, 64, 274)):
        with pytest.raises(ValueError):
            gpu_ctx.noise_stats(t, roi=roi)


@pytest.mark.parametrize("typ", (7, 6))
def test_decode_noise_stats(gpu_ctx, typ):
    w, h = 512, 96
    items = []
    for seed in (1, 2, 3):
        img = L.natural_image_np(w, h, 12, 12.0, seed + 10 * typ)
        buf = L.encode7(img) if typ == 7 else L.encode6(img)
        items.append((buf, img))
    ins = [torch.from_numpy(b).to(DEV) for b, _ in items]
    imgs = np.stack([im for _, im in items])
    kw = dict(sat=(4095, 4000, 4095, 3000), lo=2, roi=(2, 6, h - 2, w - 8))
    s0 = gpu_ctx.last_serial()
    res = gpu_ctx.decode_noise_stats(ins, w, h, typ, **kw)
    torch.cuda.synchronize()
    assert res.shift == 7
    _same(res.raw.cpu().numpy(), NR.noise_stats(imgs, 7, kw["sat"], kw["lo"], kw["roi"]), "decode_noise_stats")
    # ... and equals decode_batch + noise_stats, which takes no serial
    outs = [torch.zeros(w * h, dtype=torch.int16, device=DEV) for _ in ins]
    frames = M.Context.make_frames([(i.data_ptr(), i.numel(), w, h, typ, o.data_ptr(), w * h * 2) for i, o in zip(ins, outs)])
    written, status = gpu_ctx.decode_batch(frames)
    assert status == [0, 0, 0]
    s1 = gpu_ctx.last_serial()
    direct = gpu_ctx.noise_stats(torch.stack(outs).view(torch.uint16).view(3, h, w), **kw)
    torch.cuda.synchronize()
    assert torch.equal(direct.raw, res.raw) and gpu_ctx.last_serial() == s1 > s0


def test_estimate_noise_feeds_denoise(gpu_ctx):
    """8 noisy 256 x 512 frames of a ramp over eleven level bins with a known profile: the estimate is exactly what noise_fit makes
    of the numpy statement's records (how close that is to the truth: tests/test_noise_fit.py), and its table is one that
    denoise() takes and that does not make the frames worse."""
    rng = np.random.default_rng(8)
    black, white, a, b = 64, 4095, 0.5, 4.0
    clean = black + 100 + np.mgrid[0:256, 0:512][1] * (1400.0 / 512)
    imgs = np.stack([NR.noisy(clean, a, b, black, rng) for _ in range(8)])
    t = _dev16(imgs)
    S, O = gpu_ctx.estimate_noise(t, black, white)
    ref = NR.noise_stats(imgs, 7, white, 1)
    ref["shift"] = 7
    S2, O2 = M.noise_fit(ref, black, white)
    assert S.shape == O.shape == (4,) and np.array_equal(S, S2) and np.array_equal(O, O2)
    assert (S > 0).all() and (O >= 0).all()
    lut, shift = M.noise_lut(S, O, black, white)
    out = gpu_ctx.denoise(t, lut, shift)
    torch.cuda.synchronize()
    got = _np(out).astype(np.float64)
    assert got.shape == imgs.shape and np.abs(got - clean).mean() < np.abs(imgs - clean).mean()


def test_one_strip_per_workgroup(tmp_path_factory):
    """A build that holds a workgroup to one strip (build.NOISE_STRIP_FLAGS), in a child process: as many workgroups as strips add
    their counters to a frame's record."""
    res = PH.run_child(__name__, "strips1", os.path.join(ROOT, "tests", "_noise_strip_child.py"), [], B.NOISE_STRIP_FLAGS,
                       "libmcraw_noise_strip.so", 120, tmp_path_factory)
    assert res["errors"] == [] and res["calls"] == 3 and res["strips"] == [6, 34, 6]
