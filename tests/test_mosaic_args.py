"""CPU: the checks that the five mosaic stages share (csrc/mcraw_mosaic_args.h: one strided batch of mosaics, its extent, the
16-byte grid, the overlap of two batches) are plain C++ and need neither a GPU nor HIP.  tests/cpp/mosaic_args_check.cpp includes
that header alone and compares what the entry points decide with it against transcriptions of the check sequences they carried
before."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")


def test_mosaic_args_without_hip(tmp_path):
    """Accept / reject, the extents of `in` and `out` and the on-grid flags for shade, stats, fixpix, denoise and merge: every
    combination of W, H in {1, 2, 7, 8, 9, 65536, 65537, 0, -4}, pitch W - 1 / W / W + 1 / W + 8, frame stride one below / at /
    above the minimum, n 0 .. 2 and addresses odd / 2-byte / 16-byte aligned for both batches; the overlap layouts of the GPU
    tests (in place, out inside in, out ending inside in, the same base with another pitch or frame stride) and their
    neighbours; 200 000 seeded tuples.  Host code only, under ASan and UBSan."""
    exe = str(tmp_path / "mosaic_args_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "mosaic_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"cases (\d+)", lines[-2]).group(1)) >= 1000, lines[-2]
    acc, rej = (int(v) for v in re.match(r"accepted (\d+) rejected (\d+)", lines[-3]).groups())
    assert acc >= 1000 and rej >= 1000, lines[-3]  # (both decisions are exercised)
