#!/usr/bin/env python3
"""Resource report of the demosaic kernels (csrc/mcraw_rgb.hip), of the lens-shading kernel (csrc/mcraw_shade.hip), of the
statistics kernels (csrc/mcraw_stats.hip), of the defective-pixel kernels (csrc/mcraw_fixpix.hip), of the denoising kernel
(csrc/mcraw_denoise.hip), of the temporal merge (csrc/mcraw_merge.hip), of the shift estimate (csrc/mcraw_align.hip) and of the position field (csrc/mcraw_cells.hip and the merge's kmerge<..., field> instances): compiles the files for gfx950 with -Rpass-analysis=kernel-resource-usage (no GPU needed) and prints
one line per instance in the format of profiles/rgb_resources.txt / display_resources.txt / yuv_resources.txt /
shade_resources.txt / stats_resources.txt / fixpix_resources.txt / denoise_resources.txt / merge_resources.txt / align_resources.txt /
cells_resources.txt (kcells_* and kmerge<..., field>) / area_resources.txt (csrc/mcraw_area.hip: krgb_area and karea_tab) /
resample_resources.txt (csrc/mcraw_resample.hip: krgb_resample and kres_tab) / warp_resources.txt (csrc/mcraw_warp.hip: krgb_warp) /
mesh_resources.txt (csrc/mcraw_mesh.hip: krgb_mesh) / ha_resources.txt (csrc/mcraw_ha.hip: krgb_ha) / highlights_resources.txt (csrc/mcraw_highlights.hip: khl_apply, khl_clip, khl_measure, khl_init) / noise_resources.txt (csrc/mcraw_noise.hip: knoise, knoise_init).

    python tools/rgb_resources.py            # every instance
    python tools/rgb_resources.py --check    # the figures in the seventeen committed files must equal the compiler's; exit 1 if not
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motioncam_decoder_amd import build as B

KINDS = {32: "f32", 33: "f16", 34: "bf16", 48: "u8", 49: "u16", 50: "nv12", 51: "p010"}
FILES = ("rgb_resources.txt", "display_resources.txt", "yuv_resources.txt")
SHADE_FILE = "shade_resources.txt"
RGB_NAME = r"Function Name: _ZN5mcraw\d+(krgb_mhc|krgb_bin2)y?ILi(\d+)ELi(\d)EEEv"
STATS_FILE = "stats_resources.txt"
STATS_NAME = r"Function Name: _ZN5mcraw\d+(kstats_init|kstats)(?:ILi(\d+)EEEv|E)"  # kstats<bins_log2>, and the kernel that empties the records
FIXPIX_FILE = "fixpix_resources.txt"
FIXPIX_NAME = r"Function Name: _ZN5mcraw\d+(kfixpix_init|kfixpix_list|kfixpix)(?:ILb([01])EEEv|E)"  # kfixpix<NT>, the list pass, the counts' init
DENOISE_FILE = "denoise_resources.txt"
DENOISE_NAME = r"Function Name: _ZN5mcraw\d+(kdenoise)ILi([12])ELb([01])EEEv"  # kdenoise<RADIUS, NT>
MERGE_FILE = "merge_resources.txt"
MERGE_NAME = r"Function Name: _ZN5mcraw\d+(kmerge)ILi([01])ELb([01])ELb([01])ENS_\d+Mg(?:Cell)?ArgsEEEvT2_"  # kmerge<SUPPORT, NT, FIELD, ARGS>: FIELD 0, the shifts per frame (merge_resources.txt); 1, per cell (cells_resources.txt)
CELLS_FILE = "cells_resources.txt"
CELLS_NAME = r"Function Name: _ZN5mcraw\d+(kcells_[a-z]+)(?:ILi([01])EEEv|E)"  # kcells_sad<R = 1: nine candidates in registers; 0: a loop>, the others
ALIGN_FILE = "align_resources.txt"
ALIGN_NAME = r"Function Name: _ZN5mcraw\d+(kalign_[a-z]+)(?:ILi([01])EEEv|E)"  # kalign_sad<R = 1: nine candidates in registers; 0: a loop>, the others
AREA_FILE = "area_resources.txt"
AREA_NAME = r"Function Name: _ZN5mcraw\d+(krgb_area|karea_tab)(?:ILi(\d+)ELi(\d)EEEv|E)"  # krgb_area<kind, CFA shift>, and the kernel that writes the taps
RESAMPLE_FILE = "resample_resources.txt"
RESAMPLE_NAME = r"Function Name: _ZN5mcraw\d+(krgb_resample|kres_tab)(?:ILi(\d+)ELi(\d)EEEv|E)"  # krgb_resample<kind, CFA shift>, and the kernel that writes the taps
WARP_FILE = "warp_resources.txt"
WARP_NAME = r"Function Name: _ZN5mcraw\d+(krgb_warp)ILi(\d+)ELi(\d)EEEv"  # krgb_warp<kind, CFA shift>
MESH_FILE = "mesh_resources.txt"
MESH_NAME = r"Function Name: _ZN5mcraw\d+(krgb_mesh)ILi(\d+)ELi(\d)EEEv"  # krgb_mesh<kind, CFA shift>
HA_FILE = "ha_resources.txt"
HA_NAME = r"Function Name: _ZN5mcraw\d+(krgb_ha)ILi(\d+)ELi(\d)EEEv"  # krgb_ha<kind, CFA shift>
HL_FILE = "highlights_resources.txt"
HL_NAME = r"Function Name: _ZN5mcraw\d+(khl_init|khl_measure|khl_apply|khl_clip)(?:ILb([01])EEEv|E)"  # khl_apply<NT>, khl_clip<NT>, the measure kernel, the records' init
NOISE_FILE = "noise_resources.txt"
NOISE_NAME = r"Function Name: _ZN5mcraw\d+(knoise_init|knoise)E"  # the measuring kernel, the records' init
SHADE_NAME = r"Function Name: _ZN5mcraw\d+(kshade)ILb([01])EEEv"  # kshade<NT>: `sc1 nt` streaming stores or plain ones


def _label(m):
    if m.group(1) == "kstats_init":
        return "kstats_init"
    if m.group(1) == "kstats":
        return "kstats<B=%d>" % (1 << int(m.group(2)))
    if m.group(1) in ("kfixpix_init", "kfixpix_list"):
        return m.group(1)
    if m.group(1) == "kfixpix":
        return "kfixpix<%s>" % ("stream" if m.group(2) == "1" else "plain")
    if m.group(1) == "kdenoise":
        return "kdenoise<R=%s,%s>" % (m.group(2), "stream" if m.group(3) == "1" else "plain")
    if m.group(1) == "kmerge":
        return "kmerge<S=%s,%s%s>" % (m.group(2), "stream" if m.group(3) == "1" else "plain", ",field" if m.group(4) == "1" else "")
    if m.group(1) == "kcells_sad":
        return "kcells_sad<%s>" % ("refine" if m.group(2) == "1" else "coarse")
    if m.group(1).startswith("kcells_"):
        return m.group(1)
    if m.group(1) == "kalign_sad":
        return "kalign_sad<%s>" % ("refine" if m.group(2) == "1" else "coarse")
    if m.group(1).startswith("kalign_"):
        return m.group(1)
    if m.group(1) in ("karea_tab", "kres_tab"):
        return m.group(1)
    if m.group(1) in ("khl_init", "khl_measure", "knoise", "knoise_init"):
        return m.group(1)
    if m.group(1) in ("khl_apply", "khl_clip"):
        return "%s<%s>" % (m.group(1), "stream" if m.group(2) == "1" else "plain")
    if m.group(1) == "kshade":
        return "kshade<%s>" % ("stream" if m.group(2) == "1" else "plain")
    return "%s<%s,S=%s>" % (m.group(1), KINDS[int(m.group(2))], m.group(3))


def report(source="mcraw_rgb.hip", name=RGB_NAME):
    src = os.path.join(B.CSRC, source)
    with tempfile.TemporaryDirectory() as d:
        cmd = [B.HIPCC] + B.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                                         os.path.join(d, "x.o"), src]
        err = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
    rows, cur = {}, None
    for line in err.splitlines():
        m = re.search(name, line)
        if m:
            cur = _label(m)
            rows[cur] = {}
            continue
        if "Function Name:" in line:  # an instance that this report does not list: its figures belong to no row
            cur = None
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            rows[cur][m.group(1).strip()] = int(m.group(2))
    out = {}
    for k, v in rows.items():
        out[k] = "%-24s %6d %5d %8d %12d %7d" % (k, v["VGPRs"], v["TotalSGPRs"], v["ScratchSize"], v["Occupancy"], v["LDS Size"])
    return out


def _check(files, rep, prefix):
    bad, seen = 0, 0
    for f in files:
        for line in open(os.path.join(ROOT, "profiles", f)) if os.path.exists(os.path.join(ROOT, "profiles", f)) else ():
            if not line.startswith(prefix):
                continue
            seen += 1
            if rep.get(line.split()[0], "").split() != line.split():  # (the files differ in column spacing)
                bad += 1
                print("%s: committed  %s\n%s  compiler   %s" % (f, line.rstrip("\n"), " " * len(f), rep.get(line.split()[0])))
    print("%d committed lines, %d differ, %d instances compiled" % (seen, bad, len(rep)))
    return 1 if bad or seen != len(rep) else 0


def main():
    rep, shade, stats = report(), report("mcraw_shade.hip", SHADE_NAME), report("mcraw_stats.hip", STATS_NAME)
    fixpix, denoise = report("mcraw_fixpix.hip", FIXPIX_NAME), report("mcraw_denoise.hip", DENOISE_NAME)
    both, align = report("mcraw_merge.hip", MERGE_NAME), report("mcraw_align.hip", ALIGN_NAME)
    merge = {k: v for k, v in both.items() if not k.endswith(",field>")}
    area = report("mcraw_area.hip", AREA_NAME)
    cells = dict(report("mcraw_cells.hip", CELLS_NAME), **{k: v for k, v in both.items() if k.endswith(",field>")})
    resample = report("mcraw_resample.hip", RESAMPLE_NAME)
    warp = report("mcraw_warp.hip", WARP_NAME)
    ha = report("mcraw_ha.hip", HA_NAME)
    mesh = report("mcraw_mesh.hip", MESH_NAME)
    hl = report("mcraw_highlights.hip", HL_NAME)
    noise = report("mcraw_noise.hip", NOISE_NAME)
    if "--check" not in sys.argv:
        for line in list(rep.values()) + list(shade.values()) + list(stats.values()) + list(fixpix.values()) + list(denoise.values()) + \
                list(merge.values()) + list(align.values()) + list(area.values()) + list(resample.values()) + list(cells.values()) + list(warp.values()) + list(ha.values()) + list(hl.values()) + list(mesh.values()) + list(noise.values()):
            print(line)
        return 0
    return _check(FILES, rep, "krgb_") | _check((SHADE_FILE,), shade, "kshade") | _check((STATS_FILE,), stats, "kstats") | \
        _check((FIXPIX_FILE,), fixpix, "kfixpix") | _check((DENOISE_FILE,), denoise, "kdenoise") | _check((MERGE_FILE,), merge, "kmerge") | \
        _check((ALIGN_FILE,), align, "kalign") | _check((AREA_FILE,), area, ("krgb_area", "karea_tab")) | \
        _check((RESAMPLE_FILE,), resample, ("krgb_resample", "kres_tab")) | _check((CELLS_FILE,), cells, ("kcells_", "kmerge<")) | \
        _check((WARP_FILE,), warp, "krgb_warp") | _check((HA_FILE,), ha, "krgb_ha") | \
        _check((HL_FILE,), hl, "khl_") | _check((MESH_FILE,), mesh, "krgb_mesh") | _check((NOISE_FILE,), noise, "knoise")


if __name__ == "__main__":
    sys.exit(main())
