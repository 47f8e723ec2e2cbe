"""GPU: mcraw_export --transcode decodes every frame of a clip (legacy or current encoding) on the GPU, encodes it again on
the GPU as type 7 and writes the container with the camera metadata and the audio unchanged.  Every output frame says
compressionType 7, holds exactly synthlib.encode7 of its source image, and decodes -- through the product's Decoder and
through the reference decoder -- to what the source frame decodes to."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import _libs as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "motioncam_decoder_amd", "lib")
EXPORT = os.path.join(LIB, "mcraw_export")
BUFFER, METADATA, AUDIO_DATA, AUDIO_DATA_METADATA = 2, 3, 5, 6


def read_container(path):
    """(camera json, [(payload, frame json)], [(pcm bytes, timestamp or None)]) in file order."""
    raw = open(path, "rb").read()
    assert raw[:7] == b"MOTION "
    pos, camera, frames, audio, last = 8, None, [], [], None
    while pos + 8 <= len(raw):
        kind, size = struct.unpack_from("<II", raw, pos)
        body = raw[pos + 8: pos + 8 + size]
        pos += 8 + size
        if kind == METADATA:
            if camera is None:
                camera = json.loads(body)
            else:
                frames.append((last, json.loads(body)))
        elif kind == BUFFER:
            last = np.frombuffer(body, dtype=np.uint8)
        elif kind == AUDIO_DATA:
            audio.append([body, None])
        elif kind == AUDIO_DATA_METADATA:
            audio[-1][1] = struct.unpack("<q", body)[0]
    return camera, frames, [tuple(a) for a in audio]


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from motioncam_decoder_amd import build
    build.build_hip()
    build.build_host()
    d = tmp_path_factory.mktemp("transcode")
    specs = [(3000, 6, 256, 32, 12, 12.0), (1000, 7, 320, 24, 10, 4.0), (2000, 6, 160, 20, 14, 40.0), (4000, 6, 100, 6, 10, 3.0),
             (5000, 7, 200, 100, 12, 8.0), (6000, 6, 4032, 64, 12, 12.0)]
    images, frames = {}, []
    for ts, typ, w, h, nb, sig in specs:
        img = L.natural_image_np(w, h, nb, sig, ts)
        images[ts] = img
        frames.append((ts, typ, w, h, L.encode7(img) if typ == 7 else L.encode6(img)))
    audio = [(111, np.arange(960, dtype=np.int16)), (None, (np.arange(960, dtype=np.int16) * 3).astype(np.int16)),
             (333, (np.arange(960, dtype=np.int16) * 5).astype(np.int16))]
    src = L.write_mcraw(str(d / "src.mcraw"), frames, audio, camera_extra={"note": "transcode"})
    return d, src, images, {ts: (typ, buf) for ts, typ, _, _, buf in frames}


def test_transcode_clip(clips):
    d, src, images, source = clips
    out = str(d / "out.mcraw")
    r = subprocess.run([EXPORT, src, "--transcode", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "transcoded %d frames" % len(images) in r.stdout, r.stdout
    cam_in, frames_in, audio_in = read_container(src)
    cam_out, frames_out, audio_out = read_container(out)
    assert cam_out == cam_in
    assert sorted(audio_out, key=repr) == sorted(audio_in, key=repr)
    assert len(frames_out) == len(frames_in)
    ref_ok = L.ref_path() is not None
    by_ts = {int(m["timestamp"]): (p, m) for p, m in frames_in}
    for payload, meta in frames_out:
        ts = int(meta["timestamp"])
        img = images[ts]
        h, w = img.shape
        assert meta["compressionType"] == 7
        src_meta = dict(by_ts[ts][1])
        src_meta["compressionType"] = 7
        assert meta == src_meta
        assert np.array_equal(payload, L.encode7(img)), ts
        typ, buf = source[ts]
        _, want = (L.oracle_decode7 if typ == 7 else L.oracle_decode6)(buf, w, h)
        ret, got = L.oracle_decode7(payload.copy(), w, h)
        assert ret == w * h and np.array_equal(got, want)
        if ref_ok and h % 4 == 0:  # (the reference writes width * encodedHeight samples)
            ret, got = L.ref_decode7(payload.copy(), w, h)  # (rows h .. h + 3: the reference's spare rows)
            assert ret == w * h and np.array_equal(got[:h], want)


def test_transcoded_clip_decodes_through_the_product(clips, tmp_path):
    d, src, images, _ = clips
    out = str(d / "out2.mcraw")
    r = subprocess.run([EXPORT, src, "--transcode", out, "-n", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "transcoded 4 frames" in r.stdout, r.stdout + r.stderr
    dump_src, dump_out = tmp_path / "a", tmp_path / "b"
    dump_src.mkdir()
    dump_out.mkdir()
    ra = subprocess.run([EXPORT, src, "-n", "4", "-o", str(dump_src)], capture_output=True, text=True, timeout=300)
    rb = subprocess.run([EXPORT, out, "-o", str(dump_out)], capture_output=True, text=True, timeout=300)
    assert ra.returncode == 0 and rb.returncode == 0, ra.stdout + ra.stderr + rb.stdout + rb.stderr
    la = [ln for ln in ra.stdout.splitlines() if ln.startswith("frame ")]
    lb = [ln for ln in rb.stdout.splitlines() if ln.startswith("frame ")]
    assert len(la) == len(lb) == 4
    for a, b in zip(la, lb):  # same geometry and pixel checksum, only the type changes
        assert b.split(" type ")[0] == a.split(" type ")[0] and b.split("crc32")[1] == a.split("crc32")[1]
        assert " type 7 " in b
    for name in sorted(os.listdir(dump_src)):
        if name.startswith("frame_"):
            assert open(dump_src / name, "rb").read() == open(dump_out / name, "rb").read(), name
