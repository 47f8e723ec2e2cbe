"""CPU: the model of the type-7 encoder's kernels (tests/_enc7_model.py) against the synthesiser, and what the GPU path test
(tests/test_gpu_enc7_paths.py) takes for granted about the corpus.

The model works out blocks, segments and side-stream records from the image alone.  Here every corpus frame goes through
synthlib.encode7, its two side streams are parsed -- record headers, and the entries through an unpack_block for every class --
and compared with the model's block classes and refs, record classes and refs, payload length and frame length.  Then the
conditions of the GPU test are checked on the reference alone: the corpus makes every content-driven counter of the census
nonzero, all 17 block classes among them, bits records of exactly the classes 0..5 and refs records of exactly 0..15."""
import numpy as np
import pytest

import _enc7_model as E
import _libs as L


def unpack_block(p, bits):
    """The 64 entries of a side-stream record stored at class `bits` (0..15): the inverse of mcraw_synth_pack_block7."""
    n = int(E.LEN7[bits])
    P = np.asarray(p[:n], np.int64).reshape(-1, 8)  # P[i, j] = byte 8 i + j
    v = np.zeros((8, 8), np.int64)                  # v[k, j] = entry 8 k + j
    if bits == 0:
        pass
    elif bits == 1:
        for k in range(8):
            v[k] = (P[0] >> k) & 1
    elif bits == 2:
        for h in range(2):
            for k in range(4):
                v[4 * h + k] = (P[h] >> (2 * k)) & 3
    elif bits == 3:
        v[0], v[1], v[2] = P[0] & 7, (P[0] >> 3) & 7, ((P[0] >> 6) & 3) | (((P[2] >> 6) & 1) << 2)
        v[3], v[4], v[5] = P[1] & 7, (P[1] >> 3) & 7, ((P[1] >> 6) & 3) | (((P[2] >> 7) & 1) << 2)
        v[6], v[7] = P[2] & 7, (P[2] >> 3) & 7
    elif bits == 4:
        for g in range(4):
            v[2 * g], v[2 * g + 1] = P[g] & 15, P[g] >> 4
    elif bits == 5:
        for i in range(5):
            v[i] = P[i] & 31
        v[5] = (P[0] >> 5) | (((P[3] >> 5) & 3) << 3)
        v[6] = (P[1] >> 5) | (((P[4] >> 5) & 3) << 3)
        v[7] = (P[2] >> 5) | ((P[3] >> 7) << 3) | ((P[4] >> 7) << 4)
    elif bits == 6:
        for i in range(6):
            v[i] = P[i] & 63
        for t in range(3):
            v[6] |= (P[t] >> 6) << (2 * t)
            v[7] |= (P[3 + t] >> 6) << (2 * t)
    elif bits in (7, 8):
        v[:] = P
    elif bits in (9, 10):
        for h in range(2):
            for i in range(4):
                v[4 * h + i] = P[5 * h + i] | (((P[5 * h + 4] >> (2 * i)) & 3) << 8)
    else:
        raw = np.asarray(p[:128], np.int64)
        return raw[0::2] | (raw[1::2] << 8)
    return v.reshape(-1)


def parse_stream(buf, off):
    """(count, [(hb, ref)], entries, end) of the side stream at `off`."""
    count = int(np.frombuffer(buf[off: off + 4].tobytes(), "<u4")[0])
    pos, heads, ent = off + 4, [], []
    for _ in range(count // 64):
        hb, ref = int(buf[pos]) >> 4, ((int(buf[pos]) & 15) << 8) | int(buf[pos + 1])
        ent.append(unpack_block(buf[pos + 2:], hb) + ref)
        heads.append((hb, ref))
        pos += 2 + int(E.LEN7[hb])
    return count, heads, np.concatenate(ent), pos


@pytest.mark.parametrize("name", [f["name"] for f in E.corpus()])
def test_model_equals_synthesiser(name):
    f = E.by_name(name)
    F = E.model_of(f["img"])
    buf = L.encode7(f["img"])
    enc_w, enc_h, boff, roff = (int(v) for v in np.frombuffer(buf[:16].tobytes(), "<u4"))
    assert (enc_w, enc_h) == (64 * F.tilesX, 4 * F.tilesY)
    assert boff == 16 + F.payload, "payload length"
    nblk = 4 * F.ntiles
    end = boff
    for s, off in enumerate((boff, roff)):
        assert off == end, "the streams follow each other"
        count, heads, ent, end = parse_stream(buf, off)
        assert count == 64 * F.R
        assert [h for h, _ in heads] == list(F.rec_hb[s]), "record classes of stream %d" % s
        assert [r for _, r in heads] == list(F.rec_ref[s]), "record refs of stream %d" % s
        assert np.array_equal(ent[:nblk], F.nb if s == 0 else F.ref), "entries of stream %d" % s
        assert not ent[nblk:].any()
    assert end == len(buf) == F.length, "frame length"
    # the payload bytes of every segment add up, and a failed frame's range lies inside the payload
    assert int(F.seg_bytes.sum()) == F.payload and len(F.seg_bytes) == F.nseg
    lo, hi = F.failed_range(min(3, F.nseg))
    assert lo == 16 and hi <= boff


def test_geometry_of_the_big_frames():
    g = E.geometry(1024, 1028)
    assert (g["ntiles"], g["nseg"], g["R"]) == (4112, 65, 257)
    g = E.geometry(1024, 2068)
    assert (g["nseg"], g["R"]) == (130, 517)
    g = E.geometry(4, 4100)
    assert (g["tilesX"], g["nseg"]) == (1, 17)
    F = E.model_of(E.by_name("nat12 4x4100")["img"])
    assert F.tile16.sum() == 0, "every load of the narrow frame is a right-edge load"
    g = E.geometry(1024, 112)
    assert g["R"] == 28 and g["tilesX"] == 16


def test_records_image_reaches_every_record_class():
    F = E.model_of(E.records_image())
    assert set(F.rec_hb[0]) == set(range(6)), sorted(set(F.rec_hb[0]))
    assert set(F.rec_hb[1]) == set(range(16)), sorted(set(F.rec_hb[1]))
    assert list(F.rec_hb[1][:16]) == list(range(16))
    # the clamp: at 4095 (not clamped), one above, far above, at the top
    assert list(F.rec_min[1][16:20]) == [4095, 4096, 50000, 65535]
    assert list(F.rec_ref[1][16:20]) == [4095] * 4 and list(F.rec_hb[1][16:20]) == [0, 1, 15, 15]
    assert list(F.rec_hb[0][20:28]) == [0, 1, 2, 3, 4, 5, 0, 3]


def test_corpus_drives_every_content_counter():
    K = E.corpus()
    c = E.census(K)
    for k in E.CONTENT:
        assert (c[k] > 0) == (k not in E.ONLY_BAD + E.UNREACHABLE), (k, c[k])
    bits = set().union(*(set(E.model_of(f["img"]).rec_hb[0]) for f in K))
    refs = set().union(*(set(E.model_of(f["img"]).rec_hb[1]) for f in K))
    assert bits == set(range(6)) and refs == set(range(16)), (sorted(bits), sorted(refs))
    # ... and the counters of rejected and failed frames in the batches made for them
    bad = dict(E.batches())["bad among good"]
    assert E.census(bad)["side_bad"] > 0 and E.census(bad)["idle"] > 0
    lost = E.lost_batches()[0][1]
    assert lost[0]["name"] == "nat12 1024x1028"
    cl, cg = E.census(lost, lost=True), E.census(lost)
    assert cl["side_fail"] > 0 and cl["headers"] == cg["headers"] - 1 and cl["lookbacks"] == cg["lookbacks"] - 1
    assert cl["rows"] < cg["rows"] and cl["live"] == cg["live"]


def test_batches_shrink_and_grow_the_strides():
    B = dict(E.batches())
    assert E.strides(B["seq big"]) == (130, 517) and E.strides(B["seq tiny"]) == (1, 1) and E.strides(B["seq big again"]) == (130, 517)
    assert E.strides(B["all"]) == (130, 517)
    c = E.census(B["all"])
    assert c["side_idle"] > 0 and c["side_chunks"] > 0 and c["idle"] > 0
    assert E.windows_aggonly(B["seq big"]) == sum((s + 63) // 64 for s in range(1, 130)) > 129  # third windows
    lo, hi = E.word_bounds(B["seq big"])
    assert (lo, hi) == (129, 130 * 129 // 2)
