"""The noise measurement's C ABI (mcraw_noise_batch, mcraw_noise_record_bytes, mcraw_noise_energy_bin) without a GPU: symbols, the
macro, the struct's layout as a C compiler and ctypes see it, and every rejection driven through the library with host memory -- a
rejected call is decided from the arguments alone, says why under its own name and writes nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5A5
FN = "mcraw_noise_batch"
FIELDS = ("shift", "x0", "y0", "w", "h", "sat", "lo", "flags", "reserved")


def _hdr():
    return open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()


def test_symbols_macro_and_contract():
    hdr, lib = _hdr(), M.load()
    for name in (FN, "mcraw_noise_record_bytes", "mcraw_noise_energy_bin"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in M.ABI_SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define MCRAW_NOISE_ACCUMULATE\s+1u\b", hdr) and M.NOISE_ACCUMULATE == 1
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)  # no kernel id of its own
    assert lib.mcraw_noise_record_bytes() == 65568 == M.NOISE_RECORD_BYTES
    for name in ("Noise", "NoiseStats", "NOISE_ACCUMULATE", "noise_fit", "noise_quantile_gain"):
        assert name in M.__all__
    for line in ("l  = min((s >> 6) >> shift, 31)", "vb = min(4 * (e - 4) + f + 1, 127)",
                 "uint32 hist[4][32][128];  uint32 nblk[4];  uint32 nrej[4]", "E[T] = 576 sigma^2"):
        assert line in hdr, line
    code = open(M.lib_path(), "rb").read()
    for k in (b"knoise", b"knoise_init"):
        assert k in code
    # the exported bin formula at a few edges (all of them: tests/test_noise_ref.py)
    assert [lib.mcraw_noise_energy_bin(t) for t in (0, 15, 16, 19, 20, (3 << 34) - 1, 3 << 34, (1 << 64) - 1)] == [0, 0, 1, 1, 2, 126, 127, 127]


def test_struct_layout(tmp_path):
    """sizeof and offsetof as a C compiler sees the header, against ctypes and against the header's own comment."""
    src = tmp_path / "noise_probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mcraw_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(mcraw_noise));\n'
                   + "".join('    printf(" %%zu", offsetof(mcraw_noise, %s));\n' % f for f in FIELDS)
                   + '    printf(" %zu\\n", sizeof(((mcraw_noise *)0)->sat));\n    return 0;\n}\n')
    exe = str(tmp_path / "noise_probe")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [44, 0, 4, 8, 12, 16, 20, 28, 36, 40, 8]
    assert C.sizeof(M.Noise) == got[0] and [getattr(M.Noise, f).offset for f in FIELDS] == got[1:10]
    m = re.search(r"\}\s*mcraw_noise;\s*/\*\s*sizeof (\d+); x0 (\d+), sat (\d+), lo (\d+), flags (\d+), reserved (\d+)", _hdr())
    assert m and [int(v) for v in m.groups()] == [44, 4, 20, 28, 36, 40]


class _Mem:
    """Host memory that stands in for `in` and `out`: a rejected call never looks behind the addresses.  The context is a dummy
    block that such a call (and an empty batch) never looks into either."""

    def __init__(self):
        self.buf = np.full(4096 + 2 * 65568 // 2 + 4096, SENT, np.uint16)
        self.ctx = C.create_string_buffer(4096)
        base = self.buf.ctypes.data
        base += -base % 64
        self.inp, self.out = base, base + 4096  # 2 frames of 40 x 24 are 1920 bytes each

    def untouched(self):
        return bool((self.buf == SENT).all())


def _struct(**kw):
    s = M.Noise()
    s.shift, s.x0, s.y0, s.w, s.h, s.flags, s.reserved = 7, 2, 4, 32, 16, 0, 0
    for i in range(4):
        s.sat[i], s.lo[i] = 4095, 1
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _call(mem, st="default", **kw):
    a = dict(ctx=C.addressof(mem.ctx), inp=mem.inp, ip=40, ifs=960, w=40, h=24, n=2, out=mem.out, ob=2 * 65568)
    a.update(kw)
    lib = M.load()
    if isinstance(st, str):
        st = _struct()
    rc = lib.mcraw_noise_batch(a["ctx"], C.byref(st) if st is not None else None, C.c_void_p(a["inp"]), a["ip"], a["ifs"], a["w"],
                               a["h"], a["n"], C.c_void_p(a["out"]), a["ob"], None)
    return rc, lib.mcraw_last_error().decode()


def test_every_rejection_says_why_and_writes_nothing():
    mem = _Mem()
    cases = [
        ("no context", dict(ctx=None), "bad arguments"), ("no struct", dict(st=None), "bad arguments"),
        ("negative n", dict(n=-1), "bad arguments"),
        ("NULL in", dict(inp=0), "in or out missing"), ("NULL out", dict(out=0), "in or out missing"),
        ("odd in", dict(inp=mem.inp + 1), "in not aligned to uint16"),
        ("out misaligned", dict(out=mem.out + 4), "out not 8-byte aligned"), ("out odd", dict(out=mem.out + 1), "out not 8-byte aligned"),
        ("width 0", dict(w=0), "width and height must be 1 .. 65536"), ("negative height", dict(h=-3), "width and height must be 1 .. 65536"),
        ("width 65537", dict(w=65537, ip=65537, n=1), "width and height must be 1 .. 65536"),
        ("height 65537", dict(h=65537, n=1), "width and height must be 1 .. 65536"),
        ("pitch below width", dict(ip=39), "pitch below width"),
        ("frame stride too small", dict(ifs=23 * 40 + 39), "frame stride too small for the frames not to overlap"),
        ("shift 16", dict(st=_struct(shift=16)), "shift must be 0 .. 15"),
        ("odd x0", dict(st=_struct(x0=3)), "x0 and y0 must be even"), ("odd y0", dict(st=_struct(y0=1)), "x0 and y0 must be even"),
        ("w 15", dict(st=_struct(w=15)), "w and h must be at least 16"), ("h 0", dict(st=_struct(h=0)), "w and h must be at least 16"),
        ("window too wide", dict(st=_struct(w=39)), "the window leaves the frame"),
        ("window too high", dict(st=_struct(h=21)), "the window leaves the frame"),
        ("x0 outside", dict(st=_struct(x0=40)), "the window leaves the frame"),
        ("x0 + w wraps", dict(st=_struct(x0=0xFFFFFFF0, w=32)), "the window leaves the frame"),
        ("y0 + h wraps", dict(st=_struct(y0=0xFFFFFFF0, h=32)), "the window leaves the frame"),
        ("unknown flag", dict(st=_struct(flags=2)), "unknown flag"),
        ("unknown flag beside the known one", dict(st=_struct(flags=1 | 0x80000000)), "unknown flag"),
        ("reserved", dict(st=_struct(reserved=1)), "reserved must be 0"),
        ("out_bytes one short", dict(ob=2 * 65568 - 1), "out_bytes below n * mcraw_noise_record_bytes()"),
        ("out inside in", dict(out=mem.inp + 64), "out overlaps the input"),
        ("out ends inside in", dict(inp=mem.out + 2 * 65568 - 8), "out overlaps the input"),
        ("out begins at the input's last sample", dict(out=mem.inp + 2 * (960 + 23 * 40 + 39) - 6, inp=mem.inp + 2), "out overlaps the input"),
    ]
    for name, kw, why in cases:
        rc, msg = _call(mem, **kw)
        assert rc < 0, name
        assert msg == FN + ": " + why, (name, msg)
        assert mem.untouched(), name
    # n == 0 is a no-op, whatever else the call says
    assert _call(mem, n=0)[0] == 0 and _call(mem, n=0, inp=0, out=0, st=_struct(shift=99, reserved=7))[0] == 0
    assert mem.untouched()


def test_a_good_call_passes_every_check():
    """Nothing here may reach the device (the context is a dummy): the neighbours of the rejected values pass every check up to
    the last one -- does `out` overlap the input --, which answers with its own words for records that end one byte inside it."""
    mem = _Mem()
    st = _struct(shift=15, x0=8, y0=8, w=32, h=16, flags=M.NOISE_ACCUMULATE)
    st.sat[0], st.lo[3] = 0, 65535
    rc, msg = _call(mem, st=st, inp=mem.out + 2 * 65568 - 8, ob=2 * 65568)
    assert rc < 0 and msg == FN + ": out overlaps the input"
    rc, msg = _call(mem, st=_struct(x0=0, y0=0, w=40, h=24), inp=mem.out + 65568 - 8, n=1, ifs=0, ob=65568)
    assert rc < 0 and msg == FN + ": out overlaps the input"
    assert mem.untouched()
