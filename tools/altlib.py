"""A second build of the library beside the product's, for the benches' --alt-lib (bench_shade / stats / fixpix / denoise /
merge / align / rgb / display / yuv .py): python -m motioncam_decoder_amd.build variant PATH -D... makes one, and so does a build of
another commit.  AltLib loads it with ctypes, makes a context of its own in it, and has one method per stage entry point, each
taking contiguous (N, H, W) uint16 CUDA tensors and the torch stream to queue on.  Also what the demosaic benches build alike:
their images and device inputs."""
import ctypes as C
import os
import sys

import numpy as np
import torch

import motioncam_decoder_amd as M

_MOSAIC_IN = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int]  # in, pitch, frame stride, width, height, n
_MOSAIC_OUT = [C.c_void_p, C.c_size_t, C.c_size_t]                            # out, pitch, frame stride
_DEMOSAIC = [C.POINTER(M.RgbColor), C.c_int] + _MOSAIC_IN + [C.c_void_p, C.c_size_t, C.c_void_p]  # colours, in, out, bytes, stream


def turn_order(forms, rep):
    """The forms of rep `rep`: on odd reps every *_alt form runs in front of its counterpart instead of behind it, so that neither
    build always follows a run of the same kernel on the same buffers (warm TLBs, a settled clock)."""
    if rep % 2 == 0:
        return list(forms)
    order = []
    for f in forms:
        if f.endswith("_alt"):
            order.insert(len(order) - 1, f)
        else:
            order.append(f)
    return order


def bench_images(content, w, h, distinct, rng):
    """The `distinct` 12-bit images of a demosaic bench: "smooth" (natural images) or "noise"."""
    import _libs as L
    if content == "smooth":
        return [L.natural_image_np(w, h, 12, 12.0, 100 + s) for s in range(distinct)]
    return [rng.integers(0, 4096, size=(h, w), dtype=np.uint16) for _ in range(distinct)]


def bench_mosaics(dev, imgs, n):
    """`imgs` in turn as an (n, H, W) uint16 tensor on `dev`."""
    h, w = imgs[0].shape
    mos = torch.empty((n, h, w), dtype=torch.uint16, device=dev)
    for i in range(n):
        mos.view(torch.int16)[i].copy_(torch.from_numpy(imgs[i % len(imgs)].view(np.int16)))
    return mos


def bench_encoded(dev, imgs, n, encode):
    """`imgs` in turn, encoded, resident on `dev`: (the tensor that holds them, [(pointer, length)], lengths)."""
    bufs = [encode(im) for im in imgs]
    ins = torch.zeros((n, max(len(b) for b in bufs) + 256), dtype=torch.uint8, device=dev)
    lens = []
    for i in range(n):
        b = bufs[i % len(bufs)]
        ins[i, :len(b)].copy_(torch.from_numpy(b))
        lens.append(len(b))
    return ins, [(ins[i].data_ptr(), lens[i]) for i in range(n)], lens


class AltLib:
    def __init__(self, path):
        self.name = os.path.basename(path)
        self.lib = C.CDLL(path)
        self.lib.mcraw_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        self.lib.mcraw_ctx_destroy.argtypes = [C.c_void_p]
        self.lib.mcraw_last_error.restype = C.c_char_p
        for fn, struct in (("mcraw_shade_batch", M.Shade), ("mcraw_fixpix_batch", M.FixPix), ("mcraw_denoise_batch", M.Denoise),
                           ("mcraw_merge_batch", M.Merge)):
            getattr(self.lib, fn).argtypes = [C.c_void_p, C.POINTER(struct)] + _MOSAIC_IN + _MOSAIC_OUT + [C.c_void_p]
        self.lib.mcraw_stats_batch.argtypes = [C.c_void_p, C.POINTER(M.Stats)] + _MOSAIC_IN + [C.c_void_p, C.c_size_t, C.c_void_p]
        if hasattr(self.lib, "mcraw_align_batch"):  # (a build of a commit in front of the stage has none)
            self.lib.mcraw_align_batch.argtypes = [C.c_void_p, C.POINTER(M.Align)] + _MOSAIC_IN + [C.c_void_p]
        if hasattr(self.lib, "mcraw_merge_cells_batch"):  # (likewise)
            self.lib.mcraw_merge_cells_batch.argtypes = [C.c_void_p, C.POINTER(M.Merge), C.POINTER(M.Cells)] + _MOSAIC_IN + _MOSAIC_OUT + [C.c_void_p]
        self.lib.mcraw_demosaic_batch.argtypes = [C.c_void_p, C.POINTER(M.RgbParams)] + _DEMOSAIC
        self.lib.mcraw_demosaic_display_batch.argtypes = [C.c_void_p, C.POINTER(M.RgbParams), C.POINTER(M.Display)] + _DEMOSAIC
        self.lib.mcraw_demosaic_yuv_batch.argtypes = [C.c_void_p, C.POINTER(M.RgbParams), C.POINTER(M.Yuv)] + _DEMOSAIC
        self.lib.mcraw_ctx_profile.argtypes = [C.c_void_p, C.c_int]
        self.lib.mcraw_ctx_kernel_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]
        self.h = C.c_void_p()
        if self.lib.mcraw_ctx_create(0, C.byref(self.h)) != 0:
            sys.exit("alt-lib: %s" % self.lib.mcraw_last_error().decode())

    def _mosaic_call(self, fn, s, mos, out, stream):
        n, h, w = mos.shape
        rc = getattr(self.lib, fn)(self.h, C.byref(s), C.c_void_p(mos.data_ptr()), w, h * w, w, h, n, C.c_void_p(out.data_ptr()),
                                   w, h * w, C.c_void_p(stream.cuda_stream))
        assert rc == 0, self.lib.mcraw_last_error().decode()

    def shade(self, mos, dmap, out, stream, gw, gh, top, black):
        s = M.Shade()
        s.map_w, s.map_h, s.nmaps, s.top = gw, gh, 1, top
        for i in range(4):
            s.black[i] = black[i]
        s.map = dmap.data_ptr()
        self._mosaic_call("mcraw_shade_batch", s, mos, out, stream)

    def fix(self, mos, out, stream, black, abs_thr, rel):
        s = M.FixPix()
        s.flags, s.rank, s.rel_thr, s.nlist = 3, 2, rel, 0
        for i in range(4):
            s.black[i], s.abs_thr[i] = black[i], abs_thr[i]
        self._mosaic_call("mcraw_fixpix_batch", s, mos, out, stream)

    def denoise(self, mos, out, stream, lut, shift, radius):
        s = M.Denoise()
        s.radius, s.amount, s.lut_log2, s.shift, s.nluts = radius, 256, int(lut.shape[-1]).bit_length() - 1, shift, 1
        s.lut = lut.data_ptr()
        self._mosaic_call("mcraw_denoise_batch", s, mos, out, stream)

    def merge(self, mos, out, stream, lut, shift, T, support):
        s = M.Merge()
        s.before, s.after, s.first, s.count, s.support, s.amount = T, T, 0, int(mos.shape[0]), support, 256
        s.lut_log2, s.shift, s.nluts, s.reserved = int(lut.shape[-1]).bit_length() - 1, shift, 1, 0
        s.lut, s.pos = lut.data_ptr(), None
        self._mosaic_call("mcraw_merge_batch", s, mos, out, stream)

    def merge_cells(self, mos, out, stream, lut, shift, T, support, field, cell, amount=256):
        """mcraw_merge_cells_batch: field, a contiguous (N, Cy, Cx, 2) int16 tensor for cells of cell = (cell_h, cell_w)."""
        s = M.Merge()
        s.before, s.after, s.first, s.count, s.support, s.amount = T, T, 0, int(mos.shape[0]), support, amount
        s.lut_log2, s.shift, s.nluts, s.reserved = int(lut.shape[-1]).bit_length() - 1, shift, 1, 0
        s.lut, s.pos = lut.data_ptr(), None
        g = M.Cells()
        g.cell_h, g.cell_w, g.cells_y, g.cells_x, g.reserved, g.pos = cell[0], cell[1], int(field.shape[1]), int(field.shape[2]), 0, field.data_ptr()
        n, h, w = mos.shape
        rc = self.lib.mcraw_merge_cells_batch(self.h, C.byref(s), C.byref(g), C.c_void_p(mos.data_ptr()), w, h * w, w, h, n,
                                              C.c_void_p(out.data_ptr()), w, h * w, C.c_void_p(stream.cuda_stream))
        assert rc == 0, self.lib.mcraw_last_error().decode()

    def align(self, mos, pos, work, stream, levels, radius, black, ref=-1):
        """Positions into `pos` (a contiguous (N, 2) int16 tensor); work: a uint8 tensor of mcraw_align_work_bytes bytes."""
        n, h, w = mos.shape
        a = M.Align()
        a.levels, a.radius, a.ref, a.reserved = levels, radius, ref, 0
        for i in range(4):
            a.black[i] = black[i]
        a.pos, a.sad, a.work, a.work_bytes = pos.data_ptr(), None, work.data_ptr(), work.numel()
        rc = self.lib.mcraw_align_batch(self.h, C.byref(a), C.c_void_p(mos.data_ptr()), w, h * w, w, h, n, C.c_void_p(stream.cuda_stream))
        assert rc == 0, self.lib.mcraw_last_error().decode()

    def stats(self, mos, recs, stream, bins, shift, sat, roi=None):
        """Records into `recs` (a contiguous (N, 16 * bins + 96) uint8 tensor); returns a FrameStats over it."""
        n, h, w = mos.shape
        s = M.Stats()
        y0, x0, rh, rw = (0, 0, h, w) if roi is None else roi
        s.bins_log2, s.shift, s.x0, s.y0, s.w, s.h = bins.bit_length() - 1, shift, x0, y0, rw, rh
        for i in range(4):
            s.sat[i] = sat
        s.flags, s.reserved = 0, 0
        rc = self.lib.mcraw_stats_batch(self.h, C.byref(s), C.c_void_p(mos.data_ptr()), w, h * w, w, h, n, C.c_void_p(recs.data_ptr()),
                                        recs.numel(), C.c_void_p(stream.cuda_stream))
        assert rc == 0, self.lib.mcraw_last_error().decode()
        return M.FrameStats(recs, bins, shift)

    def _demosaic_call(self, fn, prm, stage, mos, out, stream, gain, matrix):
        n, h, w = mos.shape
        cols, nc = M._rgb_colors(gain, matrix, n, fn)
        structs = (C.byref(prm),) if stage is None else (C.byref(prm), C.byref(stage))
        rc = getattr(self.lib, fn)(self.h, *structs, cols, nc, C.c_void_p(mos.data_ptr()), w, h * w, w, h, n,
                                   C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), C.c_void_p(stream.cuda_stream))
        assert rc == 0, self.lib.mcraw_last_error().decode()

    def demosaic(self, mos, out, stream, algo, dtype, white, black, gain=None, matrix=None, cfa="rggb", clip=False):
        prm = M._rgb_params(algo, M._float_code(dtype), M.FLOAT_CLIP if clip else 0, cfa, white, black)
        self._demosaic_call("mcraw_demosaic_batch", prm, None, mos, out, stream, gain, matrix)

    def demosaic_display(self, mos, out, stream, algo, lut, layout, white, black, gain=None, matrix=None, cfa="rggb"):
        """lut: a 1-D uint16 CUDA tensor; out's dtype (uint8 / uint16) decides the display dtype."""
        d = M.Display()
        d.dtype, d.layout = (M.DISP_U8 if out.dtype == torch.uint8 else M.DISP_U16), M._DISP_LAYOUTS[layout]
        d.lut_log2, d.reserved, d.lut = int(lut.numel()).bit_length() - 1, 0, lut.data_ptr()
        self._demosaic_call("mcraw_demosaic_display_batch", M._rgb_params(algo, 0, 0, cfa, white, black), d, mos, out, stream, gain, matrix)

    def demosaic_yuv(self, mos, out, stream, algo, lut, fmt, in_bits, white, black, gain=None, matrix=None, cfa="rggb",
                     standard="bt709", range="limited"):
        """lut: a 1-D uint16 CUDA tensor of in_bits entries' width."""
        fcode, bits, _ = M._YUV_FORMATS[fmt]
        cy, cb, cr, sh, y_off, c_off = M.yuv_matrix(standard, range, bits, in_bits)
        y = M.Yuv()
        y.format, y.lut_log2, y.in_bits, y.sh, y.y_off, y.c_off = fcode, int(lut.numel()).bit_length() - 1, in_bits, sh, y_off, c_off
        for i in (0, 1, 2):
            y.cy[i], y.cb[i], y.cr[i] = cy[i], cb[i], cr[i]
        y.reserved, y.lut = 0, lut.data_ptr()
        self._demosaic_call("mcraw_demosaic_yuv_batch", M._rgb_params(algo, 0, 0, cfa, white, black), y, mos, out, stream, gain, matrix)

    def profile(self, only):
        """Bracket the launches of the kernels named in `only` with events (none: off), as Context.profile."""
        mode = 0
        for name in only:
            mode |= 2 << M._kernel_id(name)
        self.lib.mcraw_ctx_profile(self.h, mode)

    def kernel_ms(self, name, reset=False):
        ms, n = C.c_double(), C.c_int()
        rc = self.lib.mcraw_ctx_kernel_ms(self.h, M._kernel_id(name), C.byref(ms), C.byref(n), 1 if reset else 0)
        assert rc == 0, rc
        return ms.value, n.value

    def close(self):
        self.lib.mcraw_ctx_destroy(self.h)
