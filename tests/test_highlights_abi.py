"""The highlight stage's C ABI (mcraw_highlights_batch, mcraw_highlights_measure_batch) without a GPU: symbols, macros, the
struct's layout, and every rejection driven through the library with host memory -- a rejected call is decided from the
arguments alone, says why under its own name and writes nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5A5
APPLY, MEASURE = "mcraw_highlights_batch", "mcraw_highlights_measure_batch"


def _hdr():
    return open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()


def test_symbols_macros_and_contract():
    hdr, lib = _hdr(), M.load()
    for name in (APPLY, MEASURE):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in M.ABI_SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define MCRAW_HL_CLIP\s+0u\b", hdr) and M.HL_CLIP == 0
    assert re.search(r"#define MCRAW_HL_REBUILD\s+1u\b", hdr) and M.HL_REBUILD == 1
    assert re.search(r"#define MCRAW_HL_ACCUMULATE\s+1u\b", hdr) and M.HL_ACCUMULATE == 1
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)  # no kernel id of its own
    for name in ("Highlights", "HighlightChroma", "HL_CLIP", "HL_REBUILD", "HL_ACCUMULATE", "highlight_gains"):
        assert name in M.__all__
    for line in ("inv[p] = ((1 << 24) + gain[p] / 2) / gain[p]", "d = max(s - black[q], 0);   v = (d * gain[q] + 2048) >> 12",
                 "Hm = (left + right + 1) >> 1;   Vm = (up + down + 1) >> 1;   Dm = (the four diagonals + 2) >> 2",
                 "cap[p] = black[p] + ((m * inv[p] + 2048) >> 12)", "out = max(s, min(black[p] + ((cand * inv[p] + 2048) >> 12), top))",
                 "-1 -> 1 and n -> n - 2", "int64 sum[4]; uint32 cnt[4]; uint32 pad[4]"):
        assert line in hdr, line
    code = open(M.lib_path(), "rb").read()
    for k in (b"khl_apply", b"khl_measure", b"khl_clip", b"khl_init"):
        assert k in code


def test_struct_layout():
    assert C.sizeof(M.Highlights) == 64
    names = ("mode", "cfa", "flags", "top", "black", "sat", "gain", "lo", "rec", "nrec", "reserved")
    assert [getattr(M.Highlights, f).offset for f in names] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 60]
    m = re.search(r"\}\s*mcraw_highlights;\s*/\*\s*sizeof (\d+); cfa (\d+), flags (\d+), top (\d+), black (\d+), sat (\d+), gain (\d+), "
                  r"lo (\d+), rec (\d+), nrec (\d+), reserved (\d+)", _hdr())
    assert m and [int(v) for v in m.groups()] == [C.sizeof(M.Highlights)] + [getattr(M.Highlights, f).offset for f in names[1:]]


class _Mem:
    """Host memory that stands in for `in`, `out` and the records: a rejected call never looks behind the addresses.  The context
    is a dummy block that such a call (and an empty batch) never looks into either."""

    def __init__(self):
        self.buf = np.full(16384, SENT, np.uint16)
        self.ctx = C.create_string_buffer(4096)
        base = self.buf.ctypes.data
        base += -base % 64
        self.inp, self.out, self.rec = base, base + 8192, base + 16384  # 24 x 10 x 2 frames are 960 bytes each

    def untouched(self):
        return bool((self.buf == SENT).all())


def _struct(rec, nrec, **kw):
    s = M.Highlights()
    s.mode, s.cfa, s.flags, s.top = M.HL_REBUILD, 0, 0, 65535
    for i, g in enumerate((8192, 4096, 4096, 6554)):
        s.black[i], s.sat[i], s.gain[i], s.lo[i] = 64, 4095, g, 2079
    s.rec, s.nrec, s.reserved = rec or None, nrec, 0
    for k, v in kw.items():
        if isinstance(v, tuple):  # (index, value) of one of the arrays
            getattr(s, k)[v[0]] = v[1]
        else:
            setattr(s, k, v)
    return s


def _call(mem, which, st="default", **kw):
    a = dict(ctx=C.addressof(mem.ctx), inp=mem.inp, ip=24, ifs=240, w=24, h=10, n=2, out=mem.out, op=24, ofs=240)
    a.update(kw)
    lib = M.load()
    if isinstance(st, str):
        st = _struct(mem.rec, 2)
    ref = C.byref(st) if st is not None else None
    if which == MEASURE:
        rc = lib.mcraw_highlights_measure_batch(a["ctx"], ref, C.c_void_p(a["inp"]), a["ip"], a["ifs"], a["w"], a["h"], a["n"], None)
    else:
        rc = lib.mcraw_highlights_batch(a["ctx"], ref, C.c_void_p(a["inp"]), a["ip"], a["ifs"], a["w"], a["h"], a["n"],
                                        C.c_void_p(a["out"]), a["op"], a["ofs"], None)
    return rc, lib.mcraw_last_error().decode()


def _cases(mem, which):
    S = lambda **kw: _struct(mem.rec, 2, **kw)
    cases = [
        ("no context", dict(ctx=None)), ("no struct", dict(st=None)), ("negative n", dict(n=-1)),
        ("NULL in", dict(inp=0)), ("odd in", dict(inp=mem.inp + 1)),
        ("width 1", dict(w=1)), ("height 1", dict(h=1)), ("width 0", dict(w=0)), ("negative height", dict(h=-3)),
        ("width 65537", dict(w=65537, ip=65537, op=65537, n=1, st=_struct(mem.rec, 1))), ("height 65537", dict(h=65537, n=1, st=_struct(mem.rec, 1))),
        ("in pitch below width", dict(ip=23)), ("in frame stride too small", dict(ifs=239)),
        ("unknown mode", dict(st=S(mode=2))), ("unknown cfa", dict(st=S(cfa=4))), ("unknown flag", dict(st=S(flags=2))),
        ("unknown flag beside the known one", dict(st=S(flags=1 | 0x80000000))),
        ("top 0", dict(st=S(top=0))), ("top 65536", dict(st=S(top=65536))), ("reserved", dict(st=S(reserved=1))),
        ("nrec 3", dict(st=_struct(mem.rec, 3))), ("rec NULL with nrec", dict(st=_struct(0, 2))),
        ("rec misaligned", dict(st=_struct(mem.rec + 4, 2))), ("rec odd", dict(st=_struct(mem.rec + 1, 2))),
        ("rec inside in", dict(st=_struct(mem.inp + 64, 2))), ("rec ends inside in", dict(st=_struct(mem.inp - 120, 2))),
    ]
    for p in range(4):
        cases += [("gain[%d] 255" % p, dict(st=S(gain=(p, 255)))), ("sat[%d] == black" % p, dict(st=S(sat=(p, 64)))),
                  ("sat[%d] < black" % p, dict(st=S(sat=(p, 63))))]
    if which == APPLY:
        cases += [("NULL out", dict(out=0)), ("odd out", dict(out=mem.out + 1)), ("out pitch below width", dict(op=23)),
                  ("out frame stride too small", dict(ofs=239)), ("in place", dict(out=mem.inp)), ("in place, one frame", dict(out=mem.inp, n=1, st=_struct(mem.rec, 1))),
                  ("out inside in", dict(out=mem.inp + 16)), ("out ends inside in", dict(inp=mem.out + 2 * (2 * 240 - 8))),
                  ("same base, other pitch", dict(out=mem.inp, op=32, ofs=320)),
                  ("rec with nrec 0", dict(st=_struct(mem.rec, 0))),
                  ("rec inside out", dict(st=_struct(mem.out + 2 * 480 - 8, 2))), ("rec ends inside out", dict(st=_struct(mem.out - 64, 2)))]
    else:
        cases += [("nrec 0", dict(st=_struct(0, 0)))]
    return cases


@pytest.mark.parametrize("which", (APPLY, MEASURE))
def test_every_rejection_says_why_and_writes_nothing(which):
    mem = _Mem()
    for name, kw in _cases(mem, which):
        rc, msg = _call(mem, which, **kw)
        assert rc < 0, (which, name)
        assert msg.startswith(which + ": ") and len(msg) > len(which) + 2, (which, name, msg)
        assert mem.untouched(), (which, name)
    # words for the issue's list, so that a check answers to its own question
    for name, kw, word in (("width 1", dict(w=1), "2 .. 65536"), ("unknown mode", dict(st=_struct(mem.rec, 2, mode=7)), "mode"),
                           ("gain", dict(st=_struct(mem.rec, 2, gain=(2, 100))), "gain"), ("sat", dict(st=_struct(mem.rec, 2, sat=(1, 10))), "sat"),
                           ("top", dict(st=_struct(mem.rec, 2, top=0)), "top"), ("nrec", dict(st=_struct(mem.rec, 5)), "nrec"),
                           ("rec", dict(st=_struct(mem.inp, 2)), "overlaps")):
        rc, msg = _call(mem, which, **kw)
        assert rc < 0 and word in msg, (which, name, msg)
    # n == 0 is a no-op, whatever else the call says
    assert _call(mem, which, n=0)[0] == 0 and _call(mem, which, n=0, inp=0, st=_struct(0, 7, mode=9))[0] == 0
    assert mem.untouched()


def test_a_good_call_passes_every_check():
    """Nothing here may reach the device (the context is a dummy): the neighbours of the rejected values pass every check of
    hl_check, which tests/cpp/highlights_args_check.cpp drives; here the last question of the apply call -- do the records overlap
    the output -- is answered with its own words for records that end one byte inside it, behind every other check."""
    mem = _Mem()
    rc, msg = _call(mem, APPLY, st=_struct(mem.out - 2 * 64 + 8, 2, mode=M.HL_CLIP, flags=M.HL_ACCUMULATE, top=1, gain=(0, 256), sat=(3, 65)))
    assert rc < 0 and msg == APPLY + ": rec overlaps the input or the output"
    rc, msg = _call(mem, MEASURE, st=_struct(mem.inp + 2 * 480 - 8, 1, flags=M.HL_ACCUMULATE, gain=(1, 65535), cfa=3))
    assert rc < 0 and msg == MEASURE + ": rec overlaps the input"
    assert mem.untouched()
