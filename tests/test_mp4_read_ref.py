"""The Python reference of hbs_mp4_samples / hbs_mp4_init_read_host (tests/_mp4_read_ref.py) against two witnesses: the reader
of tests/_mp4_ref.py on this library's own fragment layout, and the general writer, which knows what it wrote."""
import struct

import numpy as np
import pytest

from tests import _mp4_ref as R
from tests import _mp4_read_ref as Q


def tables_equal(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("times", [False, True])
def test_reader_agrees_with_mp4_ref_on_own_layout(L, times):
    rng = np.random.default_rng(100 + L + 10 * times)
    stream, index, keep, nal_au, au, dts, pts = R.random_case(rng, 40, max_nal=200, times=times)
    prm = R.params(length_size=L, flags=R.CUT_AT_IRAP, track_id=5, sequence=9, max_samples=7)
    out, so, ss, frags, s = R.fragment(stream, index, keep, nal_au, au, dts, pts, prm)
    assert s["error"] == 0
    want = R.read_fragments(out)
    for segs in (None, [(int(f["out_off"]), int(f["out_bytes"])) for f in frags]):
        off, size, d, p, fl, fr, sm = Q.samples(out, segs, Q.read_params(track_id=5))
        assert sm["error"] == 0 and sm["nal_count"] == len(au) and sm["nal_found"] == len(frags) and sm["rbsp_bytes"] == s["rbsp_bytes"]
        assert np.array_equal(off, so) and np.array_equal(size, ss)
        assert np.array_equal(fr, frags)
        flat = [x for f in want for x in f["samples"]]
        assert [(int(a), int(b)) for a, b in zip(off, size)] == [(x[0], x[1]) for x in flat]
        k = 0
        for f in want:
            t = f["decode_time"]
            for _, _, dur, flg, cts in f["samples"]:
                assert (int(d[k]), int(p[k]), int(fl[k])) == (t, t + cts, flg)
                t += dur
                k += 1
        if dts is not None:
            assert np.array_equal(d, dts) and np.array_equal(p, pts)


def test_reader_inverts_the_general_writer():
    seen = set()
    for seed in range(60):
        rng = np.random.default_rng(seed)
        prm = Q.read_params(track_id=int(rng.integers(0, 3)), trex_duration=int(rng.integers(1, 9000)), trex_size=int(rng.integers(0, 30)),
                            trex_flags=int(rng.integers(0, 1 << 32)))
        buf, segs, expect, frags = Q.random_segments(rng, int(rng.integers(1, 4)), prm, lead=int(rng.integers(0, 3)) * 16)
        got = Q.samples(buf, segs, prm)
        assert got[6]["error"] == 0, (seed, got[6])
        tables_equal(got[:5], Q.expected_tables(expect))
        assert np.array_equal(got[5], frags), seed
        assert got[6] == Q.summary(0, len(expect), len(frags), sum(e[1] for e in expect), len(buf))
        # which features the cases exercised: read off the bytes by the independent reader's box walk
        for off, size in segs:
            top = Q.boxes(buf, off, off + size)
            if struct.unpack(">I", buf[top[-1][1]:top[-1][1] + 4])[0] == 0:
                seen.add("size0")
            for kind, at, p, e in top:
                if p - at == 16:
                    seen.add("large")
                if kind in Q.FOREIGN_TOP:
                    seen.add("foreign top")
                if kind != b"moof":
                    continue
                trafs = [k for k in Q.boxes(buf, p, e) if k[0] == b"traf"]
                if len(trafs) > 1:
                    seen.add("foreign traf")
                for _, _, tp, te in trafs:
                    truns = 0
                    for k2, a2, p2, e2 in Q.boxes(buf, tp, te):
                        if k2 in Q.FOREIGN_TRAF:
                            seen.add("foreign child")
                        if k2 == b"tfhd":
                            fl = Q.be(buf, p2, 4) & 0xFFFFFF
                            seen.update("tfhd %#x" % b for b in (1, 2, 8, 0x10, 0x20, 0x010000, 0x020000) if fl & b)
                        if k2 == b"tfdt":
                            seen.add("tfdt v%d" % buf[p2])
                        if k2 == b"trun":
                            truns += 1
                            fl = Q.be(buf, p2, 4) & 0xFFFFFF
                            seen.add("trun v%d" % buf[p2])
                            seen.update("trun %#x" % b for b in (1, 4, 0x100, 0x200, 0x400, 0x800) if fl & b)
                            seen.add("trun with data_offset" if fl & 1 else "trun without data_offset")
                    if truns > 1:
                        seen.add("several truns")
    want = {"size0", "large", "foreign top", "foreign traf", "foreign child", "tfdt v0", "tfdt v1", "trun v0", "trun v1", "several truns",
            "trun with data_offset", "trun without data_offset"}
    want |= {"tfhd %#x" % b for b in (1, 2, 8, 0x10, 0x20, 0x010000, 0x020000)} | {"trun %#x" % b for b in (1, 4, 0x100, 0x200, 0x400, 0x800)}
    assert want <= seen, want - seen


def good_moof(track=1, time=1000, entries=((10, 4, 0, 0), (10, 4, 0, 0)), data_offset=None, hflags=0x020000, short=0, **tf):
    """a plain moof + mdat whose samples lie in the mdat"""
    def make(off):
        return Q.box(b"moof", Q.mfhd(3) + Q.box(b"traf", Q.tfhd(track, hflags, **tf) + Q.tfdt(time) + Q.trun(0xF01, list(entries), 1, off)))
    m = make(0)
    m = make(len(m) + 8 if data_offset is None else data_offset)
    return m + Q.box(b"mdat", bytes(sum(e[1] for e in entries) - short))


def errors_of(buf, segs=None, prm=None, **kw):
    got = Q.samples(buf, segs, prm or Q.read_params(track_id=1), **kw)
    assert got[0] is None
    return got[6]["error"], got[6]["reserved"]


def test_chain_errors_at_the_segment():
    g = good_moof()
    segs = [(0, len(g)), (len(g), len(g)), (2 * len(g), len(g))]
    for bad in (g[:-1], g + b"\0\0\0", struct.pack(">I4s", 7, b"free") + g[8:], struct.pack(">I4sQ", 1, b"free", 15) + g[16:],
                struct.pack(">I4s", len(g) + 1, b"free") + g[8:], struct.pack(">I4s", 1, b"free") + g[8:15]):
        buf = g + bad + bytes(len(g) - len(bad)) if len(bad) <= len(g) else None
        if buf is None:
            buf, s2 = g + bad + g, [(0, len(g)), (len(g), len(bad)), (len(g) + len(bad), len(g))]
        else:
            s2 = [(0, len(g)), (len(g), len(bad)), (2 * len(g), 0)]
        assert errors_of(buf, s2) == (Q.E_ARG, [2, 0, 0])
    assert errors_of(g * 3, segs[:2] + [(2 * len(g), len(g) + 1)]) == (Q.E_ARG, [3, 0, 0])          # leaves the buffer
    assert Q.samples(g * 3, segs, Q.read_params(track_id=1))[6]["error"] == 0


def test_moof_errors_at_the_moof():
    g = good_moof()
    t = Q.tfhd(1) + Q.tfdt(5)
    cases = [
        Q.box(b"moof", Q.box(b"traf", t)),                                                         # no mfhd
        Q.box(b"moof", Q.full(b"mfhd", 1, 0, struct.pack(">I", 1)) + Q.box(b"traf", t)),         # mfhd version 1
        Q.box(b"moof", Q.full(b"mfhd", 0, 0, b"\0\0") + Q.box(b"traf", t)),                      # mfhd too short
        Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", Q.tfhd(1))),                                    # no tfdt
        Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", Q.tfhd(1) + Q.full(b"tfdt", 2, 0, bytes(8)))),  # tfdt version 2
        Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", Q.tfdt(5))),                                    # no tfhd
        Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", t + Q.trun(0x200, [(0, 1, 0, 0)], version=2))),  # trun version 2
        Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", t + Q.trun(0x200, [(0, 1, 0, 0)], count=2))),    # entries leave the box
        Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", Q.tfhd(2)) + Q.box(b"traf", Q.tfhd(1, 0) + Q.tfdt(5))),   # previous traf's end
        Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", t + struct.pack(">I4s", 9, b"free"))),           # a child leaves the traf
        Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", Q.full(b"tfhd", 0, 0x8, struct.pack(">I", 1)) + Q.tfdt(5))),   # tfhd short for its flags
    ]
    for c in cases:
        assert errors_of(g + c + g) == (Q.E_ARG, [0, 2, 0]), c
    # a moof without a traf of the track is a fragment of no samples, not an error
    none = Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", Q.tfhd(2) + Q.tfdt(5) + Q.trun(0x200, [(0, 1, 0, 0)])))
    got = Q.samples(g + none + g, None, Q.read_params(track_id=1))
    assert got[6]["error"] == 0 and got[5]["samples"].tolist() == [2, 0, 2] and got[5]["first_au"].tolist() == [0, 2, 2]


def test_sample_errors_at_the_sample():
    g = good_moof()
    prm = Q.read_params(track_id=1)
    assert errors_of(g + good_moof(time=(1 << 62) - 10)) == (Q.E_ARG, [0, 0, 4])                       # dts reaches 2^62 at its 2nd
    assert errors_of(g + good_moof(entries=((10, 4, 0, 0), (10, 4, 0, -1021), (1, 4, 0, 0)))) == (Q.E_ARG, [0, 0, 4])   # pts < 0
    assert errors_of(g + good_moof(time=(1 << 62) - 5, entries=((1, 4, 0, 4), (1, 4, 0, 4)))) == (Q.E_ARG, [0, 0, 4])  # pts >= 2^62
    assert errors_of(g + good_moof(short=1)) == (Q.E_ARG, [0, 0, 4])                                   # past the end
    assert errors_of(g + good_moof(data_offset=-1 - len(g))) == (Q.E_ARG, [0, 0, 3])                   # negative data begin
    assert errors_of(g + good_moof(hflags=1, base=(1 << 64) - 1)) == (Q.E_ARG, [0, 0, 3])              # base far outside
    # capacity, counted after the stage in front of it is clean
    assert Q.samples(g + g, None, prm, moof_cap=1)[6] == Q.summary(Q.E_CAPACITY, 0, 2, 0, 2 * len(g))
    assert Q.samples(g + g, None, prm, sample_cap=3)[6] == Q.summary(Q.E_CAPACITY, 4, 2, 0, 2 * len(g))
    assert Q.samples(b"", None, prm)[6] == Q.summary()
    assert Q.samples(g, [], prm)[6] == Q.summary(total=len(g))


NALS = [bytes([0x40, 0x01, 0x0C, 0x01, 0xFF, 0xFF, 0x01, 0x60] + [0] * 10), bytes([0x42, 0x01, 0x01, 0x01, 0x60] + list(range(1, 20))),
        bytes([0x44, 0x01, 0xC1, 0x72, 0xB4]), bytes([0x44, 0x01, 0xC0, 0xF7, 0xC0, 0xCC])]


@pytest.mark.parametrize("L,hev1", [(4, False), (2, True), (1, False)])
def test_init_read_inverts_init_segment(L, hev1):
    seg = R.init_segment(NALS, track_id=7, timescale=24000, width=1280, height=720, length_size=L, flags=R.HEV1 if hev1 else 0)
    for track in (0, 7):
        t, nals = Q.init_read(seg, track)
        assert (t["track_id"], t["timescale"], t["width"], t["height"], t["length_size"]) == (7, 24000, 1280, 720, L)
        assert t["entry"] == int.from_bytes(b"hev1" if hev1 else b"hvc1", "big") and t["n_nals"] == 4
        assert (t["trex_duration"], t["trex_size"], t["trex_flags"]) == (0, 0, 0)
        assert [seg[o:o + n] for o, n in nals] == NALS
        want = R.read_init(seg)
        assert seg[t["hvcc_off"]:t["hvcc_off"] + 22] == want["config"]
    with pytest.raises(Q.Malformed):
        Q.init_read(seg, 8)
    with pytest.raises(Q.Malformed):
        Q.init_read(seg[:-1], 0)


def test_library_init_read_agrees():
    import hevcbitstream_amd as hbs
    seg = R.init_segment(NALS, track_id=7, timescale=24000, width=1280, height=720, length_size=2)
    assert bytes(hbs.mp4_init(NALS, track_id=7, timescale=24000, width=1280, height=720, length_size=2)) == bytes(seg)
    for track in (0, 7):
        t, nals = hbs.mp4_init_read(seg, track)
        want, where = Q.init_read(seg, track)
        assert nals == NALS and nals == [seg[o:o + n] for o, n in where]
        for k, v in want.items():
            assert int(t[k]) == v, k
        assert t["reserved"].tolist() == [0, 0]
    for bad in (seg[:-1], seg[:200], b"", seg[:35] + b"\xff" + seg[36:]):
        with pytest.raises(hbs.HbsError):
            hbs.mp4_init_read(bad, 0)
    with pytest.raises(hbs.HbsError):
        hbs.mp4_init_read(seg, 8)
