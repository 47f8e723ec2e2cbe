"""CPU: what the three demosaic entry points decide about a call before anything is launched (csrc/mcraw_rgb_args.h: accept,
no-op or reject, and the launch plan -- output sizes, the 16-byte grid, launch geometry, CFA role shift, kernel kind) is plain
C++ and needs neither a GPU nor HIP.  tests/cpp/rgb_args_check.cpp includes that header alone and compares its decisions and
every plan field against a transcription of the check sequence and arithmetic that demosaic_launch carried before."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")


def test_rgb_args_without_hip(tmp_path):
    """From a good call of every kind (float f32 / f16 / bf16, display u8 / u16 x CHW / HWC, NV12 / P010) x algo: one field at a
    time -- width and height in {-4, 0, 2, 4, 6, 14, 15, 16, 65536, 65538}, pitch W - 1 / W / W + 8, frame stride one below / at
    / 8 above the minimum, n in {-1, 0, 1, 2, 35}, `in` missing / odd / 2-byte / 16-byte aligned, `out` missing and off by 1, 2,
    4 bytes, out_bytes one below / at / one above the need, algo 0 .. 3, cfa 0 .. 4, dtype 0 .. 4, flags 0 .. 2, white NaN / inf
    / at / above the mean black, ncolors 0 / 1 / n / 3, colours missing, a NaN gain and an inf matrix entry inside and behind
    the colours in use, display dtype, layout and YUV format one past, reserved 1, the LUT missing / 8 bytes off / good,
    lut_log2 and in_bits and sh at and past their ends, offsets at and past theirs for both formats, the overflow rule at
    (2^31 - 5) / (4 * 255) and one above for each row --, the geometry fields all together, the 4:2:0 evenness sizes of the GPU
    test, and 200 000 seeded tuples of zero to two such changes.  Host code only, under ASan and UBSan."""
    exe = str(tmp_path / "rgb_args_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "rgb_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"cases (\d+)", lines[-2]).group(1)) >= 1000, lines[-2]
    acc, rej = (int(v) for v in re.match(r"accepted (\d+) rejected (\d+)", lines[-3]).groups())
    assert acc >= 1000 and rej >= 1000, lines[-3]  # (both decisions are exercised)
