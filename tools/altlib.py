"""A second build of the library beside the product's, for the stage benches' --alt-lib (bench_shade / stats / fixpix / denoise /
merge .py): python -m motioncam_decoder_amd.build variant PATH -D... makes one, and so does a build of another commit.  AltLib
loads it with ctypes, makes a context of its own in it, and has one method per stage entry point, each taking contiguous
(N, H, W) uint16 CUDA tensors and the torch stream to queue on."""
import ctypes as C
import os
import sys

import motioncam_decoder_amd as M

_MOSAIC_IN = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int]  # in, pitch, frame stride, width, height, n
_MOSAIC_OUT = [C.c_void_p, C.c_size_t, C.c_size_t]                            # out, pitch, frame stride


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

    def close(self):
        self.lib.mcraw_ctx_destroy(self.h)
