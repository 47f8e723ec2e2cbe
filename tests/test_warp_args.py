"""CPU: what mcraw_demosaic_warp_batch decides about a call (csrc/mcraw_warp_args.h: accept / reject / no-op, the phase tables,
the position arithmetic, the plan of the launch and a tile's source window) is plain C++ and needs neither a GPU nor HIP.
tests/cpp/warp_args_check.cpp includes that header and compares its decisions against a transcription of the contract."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                         ids=("plain", "asan_ubsan"))
def test_warp_args_without_hip(tmp_path, flags):
    """The two tables against the formula (4096 in all, the mirror, the named phases, sum |w| <= 5120, the smallest weight -303),
    every rule one defect at a time, maps at and just beyond every bound of the linear part and of the four corners with the
    frame named, and for every accepted map of the sweep (the 81 combinations of the linear part's extremes in every corner of
    the frame, and seeded ones) the plan's invariants: the tiles cover the output, every tap of every pixel of every tile lies in
    the tile's planned window, and the window in the workgroup's LDS arrays.  A stand-alone host program, once plain and once
    under ASan and UBSan."""
    exe = str(tmp_path / "warp_args_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "warp_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"cases (\d+)", lines[-2]).group(1)) >= 300000, lines[-2]
    acc, rej = (int(v) for v in re.match(r"accepted (\d+) rejected (\d+)", lines[-3]).groups())
    assert acc >= 1000 and rej >= 1000, lines[-3]  # (both decisions are exercised)
    sabs, wmin = (int(v) for v in re.match(r"tables: max sum \|w\| (\d+)  min w (-?\d+)", lines[0]).groups())
    assert 4096 < sabs <= 5120 and wmin == -303, lines[0]
