"""Build the native parts of the MCRAW decode path, in-tree.

    python -m motioncam_decoder_amd.build            # everything
    python -m motioncam_decoder_amd.build hip synth  # selected targets
    python -m motioncam_decoder_amd.build variant /tmp/libx.so -DMCRAW_DIAG   # another build of the HIP sources (tests, tools)

Targets
  hip    motioncam_decoder_amd/lib/libmcraw_hip.so      gfx950 kernels + C ABI (hipcc)
  synth  motioncam_decoder_amd/synth/libmcraw_synth.so  encoder / image generator (gcc, CPU)
  host   motioncam_decoder_amd/lib/libmotioncam_decoder.so + mcraw_export   C++ facade (g++)

hipcc cross-compiles for gfx950 without a GPU.  The .so files are git-ignored
but travel to the GPU box with the snapshot.
"""
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
LIB = os.path.join(PKG, "lib")
CSRC = os.path.join(PKG, "csrc")
SYNTH = os.path.join(PKG, "synth")
HOST = os.path.join(PKG, "host")

HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ARCH = "gfx950"


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


# The gfx950 library: kernels (mcraw_type7 / mcraw_type6, the encoder mcraw_encode7, the demosaic mcraw_rgb, the lens-shading stage mcraw_shade, the statistics mcraw_stats, the defective-pixel stage mcraw_fixpix, the denoiser mcraw_denoise, the temporal merge mcraw_merge, the shift estimate mcraw_align and its cell-wise form mcraw_cells, the area-average demosaic mcraw_area, the resampling demosaic mcraw_resample, the affine warp mcraw_warp and the mesh warp mcraw_mesh, the edge-directed demosaic mcraw_ha, the highlight stage mcraw_highlights, the noise measurement mcraw_noise), the host side of the C ABI in its units (csrc/mcraw_host.h) and the device pool.
HIP_SOURCES = ("mcraw_abi.hip", "mcraw_submit.hip", "mcraw_tune.hip", "mcraw_device.hip", "mcraw_hostmem.hip", "mcraw_pool.hip",
               "mcraw_type7.hip", "mcraw_type6.hip", "mcraw_encode7.hip", "mcraw_rgb.hip", "mcraw_shade.hip", "mcraw_stats.hip",
               "mcraw_fixpix.hip", "mcraw_denoise.hip", "mcraw_merge.hip", "mcraw_align.hip", "mcraw_area.hip", "mcraw_resample.hip", "mcraw_cells.hip", "mcraw_warp.hip", "mcraw_ha.hip",
               "mcraw_highlights.hip", "mcraw_mesh.hip", "mcraw_noise.hip")
HIP_HEADERS = ("mcraw_plan.h", "mcraw_dev.h", "mcraw_host.h", "mcraw_race.h", "mcraw_mosaic.h", "mcraw_mosaic_args.h",
               "mcraw_rgb_args.h", "mcraw_align_args.h", "mcraw_area_args.h", "mcraw_rgb_dev.h", "mcraw_rgb_launch.h",
               "mcraw_resample_args.h", "mcraw_rgb_paths.h", "mcraw_align_pyr.h", "mcraw_cells_args.h", "mcraw_warp_args.h", "mcraw_ha_args.h",
               "mcraw_highlights_args.h", "mcraw_warp_dev.h", "mcraw_mesh_args.h", "mcraw_mosaic_paths.h", "mcraw_noise_args.h", "mcraw_est_paths.h", "mcraw_census.h")
HIP_FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc"]


def hip_sources():
    return [os.path.join(CSRC, f) for f in HIP_SOURCES]


def _objects(flags=(), tag="", force=False, only=None):
    """One object per source under lib/obj/ (rebuilt when the source or a header is newer), compiled side by side."""
    obj = os.path.join(LIB, "obj")
    os.makedirs(obj, exist_ok=True)
    hdrs = [os.path.join(CSRC, f) for f in HIP_HEADERS] + [os.path.join(ROOT, "include", "mcraw_hip.h")]
    objs, jobs = [], []
    for src in hip_sources():
        if only is not None and src not in only:
            continue
        o = os.path.join(obj, os.path.basename(src)[:-4] + tag + ".o")
        objs.append(o)
        if force or _newer(o, [src] + hdrs):
            cmd = [HIPCC] + HIP_FLAGS + ["-Wall", "-Wno-unused-function"] + list(flags) + ["-c", "-o", o, src]
            print("+", " ".join(cmd), flush=True)
            jobs.append((subprocess.Popen(cmd), cmd))
    for pr, cmd in jobs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    return objs, bool(jobs)


def _link(out, objs):
    _run([HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-fno-gpu-rdc", "-o", out] + objs + ["-lpthread"])


def build_variant(out, flags=()):
    """Another build of the same sources (tests and tools: fault injection, forced paths, diagnostics).  Only the sources that a
    flag can reach are compiled again -- those that mention a -D name themselves, all of them when a header does or when a flag
    is no -D --; the others' objects are the product library's."""
    import hashlib
    import re
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    names = [re.sub(r"^-D([A-Za-z0-9_]+).*$", r"\1", f) for f in flags if f.startswith("-D")]
    def mentions(path):  # (whole names: MCRAW_INJECT_LOST is not in a file that only has MCRAW_INJECT_LOSTE)
        text = open(path).read()
        return any(re.search(r"\b%s\b" % n, text) for n in names)
    everything = len(names) != len(flags) or any(mentions(os.path.join(CSRC, h)) for h in HIP_HEADERS)
    touched = [s for s in hip_sources() if everything or mentions(s)]
    tag = ".v" + hashlib.sha1(" ".join(flags).encode()).hexdigest()[:10]
    plain, _ = _objects(only=[s for s in hip_sources() if s not in touched])
    special, _ = _objects(flags, tag, only=touched)
    _link(out, plain + special)
    return out


# k6_decode with one of its rare paths forced and every path counted (tests/test_gpu_k6_paths.py; the switches: csrc/mcraw_type6.hip).
# Every name below occurs in mcraw_type6.hip alone, so a variant compiles that one source.
K6_PATH_VARIANTS = {
    "census": ["-DMCRAW_PATHS6"],
    "polls0": ["-DMCRAW_PATHS6", "-DMCRAW_SCALAR_POLLS6=0"],
    "polls1": ["-DMCRAW_PATHS6", "-DMCRAW_SCALAR_POLLS6=1"],
    "slowprefix": ["-DMCRAW_PATHS6", "-DMCRAW_INJECT_SLOWPREFIX6"],
    "careful": ["-DMCRAW_PATHS6", "-DMCRAW_FORCE_CAREFUL6"],
    "latefront": ["-DMCRAW_PATHS6", "-DMCRAW_FORCE_LATEFRONT6"],
    "nofront": ["-DMCRAW_PATHS6", "-DMCRAW_FORCE_NOFRONT6"],
    "nolean": ["-DMCRAW_PATHS6", "-DMCRAW_FORCE_NOLEAN6"],
    "pairmode": ["-DMCRAW_PATHS6", "-DMCRAW_FORCE_PAIRMODE6"],
    "warm64": ["-DMCRAW_PATHS6", "-DMCRAW_WARM6=64"],
    "poison": ["-DMCRAW_PATHS6", "-DMCRAW_POISON_FRONT6"],
}

# k7_side with one way of its chain walk forced and every way counted (tests/test_gpu_k7_paths.py; the switches and why each is
# valid for every input: csrc/mcraw_type7.hip).  Every name below occurs in mcraw_type7.hip alone, so a variant compiles that one source.
#   earlyswitch  MCRAW_SEGW_RATIO=65: a unit lists at most SIDE_LCAP = 512 records, so from its 8th pass on 65 * passes >= 520 is
#                above its count: every unit that reaches an 8th pass with the chain still in the piece hands over.  The model
#                (tests/_side7_corpus.py, Stream.walk(ratio=65)) finds such a unit in every corpus stream of eight and more passes.
#   coldspec     MCRAW_SPEC_WARM=4: a speculative count starts 8 bytes in front of its pieces.  The model's chain from there has
#                not joined the true one at the part's first piece for the middle part of the refs stream of both natural frames
#                (four parts; tests/test_side7_corpus.py asserts it).
#   shortunits   MCRAW_SIDE_LCAP=256: the smallest the static_asserts allow (whole passes of 512 items in the offset scan).
#   smallpieces  MCRAW_SIDE_LPT=1: pieces of 8 KiB, and with them MCRAW_SPEC_WARM=2048 -- half a piece, as in the product: a speculative
#                count starts inside the piece in front (the kernel's static_assert).  Nothing outside #ifdefs had to change for it.
K7_PATH_VARIANTS = {
    "census": ["-DMCRAW_PATHS7"],
    "segw": ["-DMCRAW_PATHS7", "-DMCRAW_FORCE_SEGW"],
    "noswitch": ["-DMCRAW_PATHS7", "-DMCRAW_SEGW_RATIO=0u"],
    "earlyswitch": ["-DMCRAW_PATHS7", "-DMCRAW_SEGW_RATIO=65u"],
    "warm1": ["-DMCRAW_PATHS7", "-DMCRAW_FORCE_SEGW", "-DMCRAW_WARM_SEGS=1"],
    "coldspec": ["-DMCRAW_PATHS7", "-DMCRAW_SPEC_WARM=4"],
    "mute": ["-DMCRAW_PATHS7", "-DMCRAW_INJECT_MUTE7"],
    "shortunits": ["-DMCRAW_PATHS7", "-DMCRAW_SIDE_LCAP=256"],
    "smallpieces": ["-DMCRAW_PATHS7", "-DMCRAW_SIDE_LPT=1", "-DMCRAW_SPEC_WARM=2048"],
    "poison": ["-DMCRAW_PATHS7", "-DMCRAW_POISON_STRIDES7"],
}

# The encoder's two kernels with every path counted and one forced or injected (tests/test_gpu_enc7_paths.py; the switches and why
# each is valid for every input: csrc/mcraw_encode7.hip).  Every name below occurs in mcraw_encode7.hip alone, so a variant
# compiles that one source.
#   wrap  MCRAW_EPOCH0E=0xFFFFFFFD: the epoch of a context's third encode batch wraps to 1.
ENC7_PATH_VARIANTS = {
    "census": ["-DMCRAW_PATHSE"],
    "refetch": ["-DMCRAW_PATHSE", "-DMCRAW_FORCE_REFETCHE"],
    "aggonly": ["-DMCRAW_PATHSE", "-DMCRAW_FORCE_AGGONLYE"],
    "slow": ["-DMCRAW_PATHSE", "-DMCRAW_INJECT_SLOWE"],
    "lost": ["-DMCRAW_PATHSE", "-DMCRAW_INJECT_LOSTE"],
    "wrap": ["-DMCRAW_PATHSE", "-DMCRAW_EPOCH0E=0xFFFFFFFDu"],
}

# k7_tiles with every item, block, lean and store path counted and one forced (tests/test_gpu_k7t_paths.py; the switches and why
# each is valid for every input: the head of csrc/mcraw_type7.hip).  Every name below occurs in mcraw_type7.hip alone -- the store
# helpers of mcraw_dev.h count through a hook that only that source defines --, so a variant compiles that one source.
K7T_PATH_VARIANTS = {
    "census": ["-DMCRAW_PATHST"],
    "nolean": ["-DMCRAW_PATHST", "-DMCRAW_FORCE_NOLEANT"],
    "slowstore": ["-DMCRAW_PATHST", "-DMCRAW_FORCE_SLOWSTORET"],
    "nomerge": ["-DMCRAW_PATHST", "-DMCRAW_FORCE_NOMERGET"],
    "poison": ["-DMCRAW_PATHST", "-DMCRAW_POISON_PAYT"],
}

# The demosaic kernels (krgb_mhc, krgb_bin2, krgb_bin2y, krgb_area, krgb_resample, krgb_warp, krgb_mesh, krgb_ha) with every path
# counted and the persistent loop forced (tests/test_gpu_rgb_paths.py; krgb_warp: tests/test_gpu_warp_paths.py; krgb_mesh:
# tests/test_gpu_mesh_paths.py; krgb_ha: tests/test_gpu_ha_paths.py; the switches and why each is valid for every input: the head of
# csrc/mcraw_rgb.hip).  MCRAW_PATHSR and MCRAW_POISON_RGB occur in mcraw_rgb.hip, mcraw_area.hip, mcraw_resample.hip, mcraw_warp.hip,
# mcraw_mesh.hip and mcraw_ha.hip alone -- the shared headers count, cap and poison through hooks that only those sources define --,
# so a variant compiles those six sources; MCRAW_RGB_GRID_CAP occurs in the first three, and the other three take their grids'
# limit from mcraw_rgb.hip.
#   grid1  one workgroup walks every unit of every frame in order
#   grid3  successive units of a workgroup skip columns, rows and frames
RGB_PATH_VARIANTS = {
    "census": ["-DMCRAW_PATHSR"],
    "grid1": ["-DMCRAW_PATHSR", "-DMCRAW_RGB_GRID_CAP=1"],
    "grid3": ["-DMCRAW_PATHSR", "-DMCRAW_RGB_GRID_CAP=3"],
    "poison": ["-DMCRAW_PATHSR", "-DMCRAW_POISON_RGB"],
    "poison1": ["-DMCRAW_PATHSR", "-DMCRAW_RGB_GRID_CAP=1", "-DMCRAW_POISON_RGB"],
}

# The mosaic stages (kshade, kstats, kfixpix, kfixpix_list, kdenoise, kmerge, khl_apply, khl_measure, khl_clip) with every path counted
# and the guarded ones forced, and the sweep of div_round (tests/test_gpu_mosaic_paths.py; the switches and why each is valid for
# every input: the head of csrc/mcraw_mosaic_paths.h).  Every name below occurs in the stage sources alone (mcraw_shade.hip,
# mcraw_stats.hip, mcraw_fixpix.hip, mcraw_denoise.hip, mcraw_merge.hip, mcraw_highlights.hip) -- the helpers of mcraw_mosaic.h count through hooks that only those
# sources define --, so a variant compiles those sources and nothing else.
MOSAIC_PATH_VARIANTS = {
    "census": ["-DMCRAW_PATHSM"],
    "slow": ["-DMCRAW_PATHSM", "-DMCRAW_FORCE_SLOWM"],
    "poison": ["-DMCRAW_PATHSM", "-DMCRAW_POISON_M"],
    "poisonslow": ["-DMCRAW_PATHSM", "-DMCRAW_POISON_M", "-DMCRAW_FORCE_SLOWM"],
    "pieces": ["-DMCRAW_PATHSM", "-DMCRAW_MERGE_PIECE=3", "-DMCRAW_STATS_MAXTILES=2"],
    "th16": ["-DMCRAW_PATHSM", "-DMCRAW_MERGE_TH=16", "-DMCRAW_DENOISE_TH=16", "-DMCRAW_FIXPIX_TH=16"],
}
# ... and with 2 frames per launch instead of up to 65535 in every stage but kmerge (which `pieces` cuts): the second and later
# iterations of the stages' launch loops (test_gpu_mosaic_paths.py::test_mosaic_paths_frames2).  The name occurs in mcraw_shade.hip,
# mcraw_stats.hip, mcraw_fixpix.hip, mcraw_denoise.hip and mcraw_highlights.hip alone.
MOSAIC_FRAMES2_FLAGS = ["-DMCRAW_PATHSM", "-DMCRAW_STAGE_FRAMES=2"]

# The estimators (kalign_pyr, kalign_down, kalign_zero, kalign_sad<0|1>, kalign_pick, kalign_final; kcells_zero, kcells_sad<0|1>,
# kcells_pick, kcells_final; knoise) with every path counted, the launch loops split and the guarded paths forced
# (tests/test_gpu_est_paths.py; the switches and why each is valid for every input: the head of csrc/mcraw_est_paths.h).  Every name
# below occurs in mcraw_align.hip, mcraw_cells.hip and mcraw_noise.hip alone -- the shared headers count and cut the launch loops
# through hooks that only those sources define --, so a variant compiles those three sources and nothing else.
#   frames2  2 frames per launch instead of up to 65535: the second and later iterations of every launch loop
#   slow     al_refine<false> for every wave; kcells_sad adds with atomics onto kcells_zero's zeros
#   poison   0xFFFF in the SAD kernels' LDS tiles in front of staging
#   strips1  knoise with one strip per workgroup
EST_PATH_VARIANTS = {
    "census": ["-DMCRAW_PATHSA"],
    "frames2": ["-DMCRAW_PATHSA", "-DMCRAW_EST_FRAMES=2"],
    "slow": ["-DMCRAW_PATHSA", "-DMCRAW_FORCE_SLOWA"],
    "poison": ["-DMCRAW_PATHSA", "-DMCRAW_POISON_A"],
    "poisonslow": ["-DMCRAW_PATHSA", "-DMCRAW_POISON_A", "-DMCRAW_FORCE_SLOWA"],
    "strips1": ["-DMCRAW_PATHSA", "-DMCRAW_NOISE_MAXSTRIPS=1"],
}

# knoise with at most one strip per workgroup (tests/test_gpu_noise.py): as many workgroups as strips flush into a frame's record,
# and half of every workgroup idles.  The name occurs in mcraw_noise.hip alone, so the variant compiles that one source.
NOISE_STRIP_FLAGS = ["-DMCRAW_NOISE_MAXSTRIPS=1"]

# The merge with tiles of 16 rows instead of 32 (tools/bench_merge.py --alt-lib, tests/test_gpu_merge_cells.py): the name occurs in
# mcraw_merge.hip alone.
MERGE_ALT_FLAGS = ["-DMCRAW_MERGE_TH=16"]


def build_merge_alt():
    """lib/alt/libmcraw_hip_th16_<tag>.so, the MCRAW_MERGE_TH=16 build, made once per state of the sources (the tag is a hash of
    them, so a library left from other sources is never taken for this one)."""
    import hashlib
    h = hashlib.sha1()
    for f in hip_sources() + [os.path.join(CSRC, f) for f in HIP_HEADERS] + [os.path.join(ROOT, "include", "mcraw_hip.h")]:
        h.update(open(f, "rb").read())
    out = os.path.join(LIB, "alt", "libmcraw_hip_th16_%s.so" % h.hexdigest()[:12])
    if not os.path.exists(out):
        build_variant(out, MERGE_ALT_FLAGS)
    return out


# The -D builds that tests/ links on the GPU box (tests/test_gpu_split.py, test_gpu_segw.py, test_gpu_lookback_fault.py,
# test_gpu_k6_paths.py, test_gpu_k7_paths.py, test_gpu_enc7_paths.py, test_gpu_k7t_paths.py, test_gpu_rgb_paths.py,
# test_gpu_mosaic_paths.py, test_gpu_noise.py, test_gpu_est_paths.py).
PATH_VARIANTS = (K6_PATH_VARIANTS, K7_PATH_VARIANTS, ENC7_PATH_VARIANTS, K7T_PATH_VARIANTS, RGB_PATH_VARIANTS, MOSAIC_PATH_VARIANTS,
                 EST_PATH_VARIANTS)
TEST_VARIANTS = ((["-DMCRAW_FORCE_SEGW"], ["-DMCRAW_INJECT_MUTE7"], ["-DMCRAW_INJECT_LOST"], MERGE_ALT_FLAGS, NOISE_STRIP_FLAGS, MOSAIC_FRAMES2_FLAGS)
                 + tuple(flags for table in PATH_VARIANTS for flags in table.values()))


def prebuild_test_variants():
    """Compile the test variants' objects into lib/obj/ ahead of time: build_variant() on the GPU box then only links."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        for i, flags in enumerate(TEST_VARIANTS):
            build_variant(os.path.join(d, "v%d.so" % i), flags)


def build_hip(force=False):
    """lib/libmcraw_hip.so: one object per source (lib/obj/), then the link."""
    os.makedirs(LIB, exist_ok=True)
    out = os.path.join(LIB, "libmcraw_hip.so")
    if os.environ.get("MCRAW_DIAG"):  # timing-experiment kernels (tools/abl7.sh) in place of the product library
        objs, built = _objects(["-DMCRAW_DIAG"], ".diag", force)
    else:
        objs, built = _objects(force=force)
    if force or built or _newer(out, objs):
        _link(out, objs)
    return out


def build_timeline(force=False):
    """The diagnostic build of the host-memory pipeline (tools/timeline_host.sh): events with timing, one line per sub-batch when
    it is drained.  Not the product: lib/timeline/libmcraw_hip.so, picked up through LD_LIBRARY_PATH or MCRAW_LIB_PATH."""
    out = os.path.join(LIB, "timeline", "libmcraw_hip.so")
    if force or _newer(out, hip_sources() + [os.path.join(CSRC, f) for f in HIP_HEADERS]):
        build_variant(out, ["-Wall", "-Wno-unused-function", "-DMCRAW_TIMELINE"])
    return out


def build_synth(force=False):
    out = os.path.join(SYNTH, "libmcraw_synth.so")
    src = os.path.join(SYNTH, "mcraw_synth.c")
    if force or _newer(out, [src]):
        _run(["gcc", "-O3", "-march=x86-64-v3", "-fPIC", "-std=c11", "-Wall", "-Wextra", "-shared", "-o", out, src, "-lm"])
    return out


def build_host(force=False):
    """C++ facade (motioncam::Decoder over the C ABI) and the export tool."""
    os.makedirs(LIB, exist_ok=True)
    out = os.path.join(LIB, "libmotioncam_decoder.so")
    srcs = [os.path.join(HOST, f) for f in ("Decoder.cpp", "RawData.cpp", "Writer.cpp")]
    if not all(os.path.exists(s) for s in srcs):
        return None
    hdrs = [os.path.join(HOST, "include", "motioncam", f) for f in ("Decoder.hpp", "Container.hpp", "RawData.hpp", "Writer.hpp",
                                                                     "mcraw_container.h")]
    hdrs.append(os.path.join(HOST, "WorkerPool.hpp"))
    inc = ["-I" + os.path.join(HOST, "include"), "-I" + os.path.join(HOST, "thirdparty"), "-I" + os.path.join(ROOT, "include")]
    if force or _newer(out, srcs + hdrs):
        _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall"] + inc + ["-o", out] + srcs +
             ["-L" + LIB, "-lmcraw_hip", "-lpthread", "-Wl,-rpath,$ORIGIN"])
    tool = os.path.join(LIB, "mcraw_export")
    tsrc = os.path.join(HOST, "mcraw_export.cpp")
    if os.path.exists(tsrc) and (force or _newer(tool, [tsrc, out])):
        _run(["g++", "-O2", "-std=c++17", "-Wall"] + inc + ["-o", tool, tsrc, "-L" + LIB, "-lmotioncam_decoder",
             "-lmcraw_hip", "-lpthread", "-Wl,-rpath,$ORIGIN"])
    return out


def build_all(force=False, targets=("hip", "synth", "host")):
    res = {}
    if "hip" in targets:
        res["hip"] = build_hip(force)
    if "synth" in targets:
        res["synth"] = build_synth(force)
    if "host" in targets:
        res["host"] = build_host(force)
    return res


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "variant":  # python -m motioncam_decoder_amd.build variant <out.so> [compiler flags ...]
        build_variant(sys.argv[2], sys.argv[3:])
        sys.exit(0)
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    build_all(force="--force" in sys.argv, targets=tuple(args) or ("hip", "synth", "host"))
