"""The Python restatement of hbs_mp4_stbl_write and hbs_mp4_moov_host (tests/_mp4_stbl_write_ref.py) held by what already exists:
the payload packers, the reader, the finder and the writer of whole progressive files of tests/_mp4_stbl_ref.py.  On the same
inputs the library's host side -- hbs_mp4_moov_host and hbs_mp4_stbl_write_bytes_host -- must say what the restatement says.  No
GPU."""
import numpy as np
import pytest

from tests import _mp4_stbl_ref as S
from tests import _mp4_stbl_write_ref as Wr
from tests.test_mp4_read_ref import NALS


def bound_holds(c, s):
    """hbs_mp4_stbl_write_bytes_host is the restatement's bound, and no plan passes it"""
    import hevcbitstream_amd as hbs
    t = c["t"]
    flags = S.CO64 if c["params"].get("co64") else 0
    bound = hbs.mp4_stbl_write_bytes(len(t["size"]), t["pts"] is not None, t["flags"] is not None, flags)
    assert bound == Wr.bytes_bound(len(t["size"]), t["pts"] is not None, t["flags"] is not None, flags)
    assert s["error"] != 0 or s["stream_bytes"] <= bound


def reads_back(c, blob, rec):
    """S.read of the boxes gives the tables that went in: dts less dts[0], flags on the non-sync bit"""
    t, p = c["t"], c["params"]
    n = len(t["size"])
    r = rec.copy()
    r["file_bytes"] = 1 << 62
    off, size, dts, pts, fl, s = S.read(blob, r)
    assert s["error"] == 0, s
    assert off.tolist() == [o + p.get("data_offset", 0) for o in t["off"]] and size.tolist() == t["size"]
    d = t["dts"] if t["dts"] is not None else [p.get("base_time", 0) + k * p["sample_duration"] for k in range(n)]
    first = d[0] if n else 0
    assert dts.tolist() == [x - first for x in d]
    assert pts.tolist() == [x - first for x in (t["pts"] if t["pts"] is not None else d)]
    assert (fl != 0).tolist() == [bool(f & S.NON_SYNC) for f in (t["flags"] if t["flags"] is not None else [0] * n)]


@pytest.mark.parametrize("seed", range(8))
def test_boxes_are_the_payloads_of_the_reader_s_writer(seed):
    rng = np.random.default_rng(300 + seed)
    n = int(rng.integers(0, 120))
    co64 = bool(seed & 1)
    t, track, dur = Wr.random_tables(rng, n, reorder=seed % 3 != 0, constant=9 if seed == 5 else None)
    if seed == 2:
        t["flags"] = None
    c = Wr.case("random", t, sample_duration=dur, co64=co64)
    blob, rec, s = Wr.call(c)
    bound_holds(c, s)
    lens = track["chunk_lens"]
    firsts = [sum(lens[:i]) for i in range(len(lens))]
    sizes = t["size"]
    constant = sizes[0] if n and sizes[0] and len(set(sizes)) == 1 else None
    pay = S.payloads(sizes, lens, [t["off"][f] for f in firsts], track["deltas"], track["cts"], None if seed == 2 else track["sync"], co64, constant)
    for name in S.BOXES:
        at, size = int(rec[name][0][0]), int(rec[name][0][1])
        assert (blob[at:at + size] or None) == pay[name], name
        if size:
            assert int.from_bytes(blob[at - 8:at - 4], "big") == size + 8
    assert s == Wr.summary(0, n, len(lens), sum(sizes), len(blob), sum(track["deltas"]))
    reads_back(c, blob, rec)


def test_the_gpu_test_s_cases_read_back():
    for c in Wr.valid_cases():
        blob, rec, s = Wr.call(c)
        assert s["error"] == 0 and len(blob) == s["stream_bytes"] and len(blob) % 4 == 0, c["name"]
        bound_holds(c, s)
        reads_back(c, blob, rec)


def file_case(seed, moov_first, co64, gaps=5):
    rng = np.random.default_rng(400 + seed)
    n = 40 + seed
    track = S.random_track(rng, n, constant=6 if seed == 3 else None)
    track["chunk_lens"] = [c for c in track["chunk_lens"] if c]
    sizes = [len(x) for x in track["samples"]]
    want, offs = S.progressive_file(track["samples"], track["chunk_lens"], track["deltas"], track["cts"], track["sync"], nals=NALS, track_id=3,
                                    co64=co64, constant=6 if seed == 3 else None, moov_first=moov_first, gaps=gaps)
    t = Wr.tables_of(sizes, track["chunk_lens"], track["deltas"], track["cts"], track["sync"], first=gaps, gap=gaps)
    body = bytearray()
    k = 0
    for c in track["chunk_lens"]:
        body += b"\xEE" * gaps + b"".join(track["samples"][k:k + c])
        k += c
    return want, offs, t, bytes(body), track


@pytest.mark.parametrize("moov_first", (True, False))
@pytest.mark.parametrize("co64", (False, True))
def test_prefix_boxes_and_mdat_are_the_progressive_file(moov_first, co64):
    import hevcbitstream_amd as hbs
    for seed in range(4):
        want, offs, t, body, track = file_case(seed, moov_first, co64)
        dur = track["deltas"][-1]
        # the layout's two recipes: T from a plan, then the real data_offset
        _, _, plan = Wr.write(t["off"], t["size"], t["dts"], t["pts"], t["flags"], co64=co64, sample_duration=dur)
        T = plan["stream_bytes"]
        prefix = Wr.moov_prefix(NALS, 0, T, track_id=3)
        assert hbs.mp4_moov(NALS, 0, T, track_id=3) == prefix
        ftyp = int.from_bytes(prefix[:4], "big")
        data_offset = (len(prefix) + T + 8) if moov_first else ftyp + 8
        blob, rec, s = Wr.write(t["off"], t["size"], t["dts"], t["pts"], t["flags"], co64=co64, sample_duration=dur, data_offset=data_offset)
        assert s["stream_bytes"] == T and [o + data_offset for o in t["off"]] == offs
        got = Wr.assemble(prefix, blob, body, moov_first)
        assert got == want
        # the finder's record is the call's, shifted to where the boxes lie
        base = len(prefix) if moov_first else len(got) - T
        found = S.find(got, track_id=3)
        assert hbs.mp4_stbl_find(got, track_id=3).tobytes() == found.tobytes()
        for name in S.BOXES:
            shift = base if int(rec[name][0][1]) else 0
            assert found[name][0].tolist() == [int(rec[name][0][0]) + shift, int(rec[name][0][1])], name
        assert int(found["flags"][0]) == int(rec["flags"][0])
        # with a duration only the three duration fields differ
        D = s["reserved"][1]
        assert D == sum(track["deltas"])
        timed = Wr.moov_prefix(NALS, D, T, track_id=3)
        assert hbs.mp4_moov(NALS, D, T, track_id=3) == timed and len(timed) == len(prefix)
        fields = [prefix.index(b"mvhd") + 20, prefix.index(b"tkhd") + 24, prefix.index(b"mdhd") + 20]
        differ = [i for i in range(len(prefix)) if prefix[i] != timed[i]]
        assert differ and all(any(f <= i < f + 4 for f in fields) for i in differ)
        for f in fields:
            assert int.from_bytes(timed[f:f + 4], "big") == D and prefix[f:f + 4] == bytes(4)


def test_moov_refusals():
    import hevcbitstream_amd as hbs
    for kw in (dict(duration=1 << 32, tables_bytes=0), dict(duration=0, tables_bytes=6), dict(duration=0, tables_bytes=(1 << 32) - 64),
               dict(duration=0, tables_bytes=1 << 32), dict(duration=0, tables_bytes=0, track_id=0), dict(duration=0, tables_bytes=0, length_size=3)):
        assert Wr.moov_prefix(NALS, **kw) == Wr.E_ARG, kw
        with pytest.raises(hbs.HbsError):
            hbs.mp4_moov(NALS, **kw)
    with pytest.raises(hbs.HbsError):
        hbs.mp4_moov([NALS[0]], 0, 0)                     # no SPS
    # the largest tables a moov holds
    prefix = Wr.moov_prefix(NALS, 0, 0)
    moov = len(prefix) - int.from_bytes(prefix[:4], "big")
    most = (S.M32 - moov) // 4 * 4
    assert hbs.mp4_moov(NALS, (1 << 32) - 1, most) == Wr.moov_prefix(NALS, (1 << 32) - 1, most)
    assert Wr.moov_prefix(NALS, 0, most + 4) == Wr.E_ARG
    with pytest.raises(hbs.HbsError):
        hbs.mp4_moov(NALS, 0, most + 4)


def test_every_sample_error_is_reported_at_its_lowest_sample():
    seen = set()
    for c, p in Wr.error_cases():
        blob, rec, s = Wr.call(c)
        assert blob is None and rec is None
        assert s == Wr.summary(Wr.E_ARG, len(c["t"]["size"]), bad_sample=p + 1), (c["name"], p)
        bound_holds(c, s)
        seen.add(c["name"])
    assert len(seen) == 11


def test_capacity_and_the_box_size_rule():
    c = Wr.valid_cases()[3]
    blob, rec, s = Wr.call(c)
    T = len(blob)
    bound_holds(c, s)
    for cap in (0, T - 4, T - 1):
        b2, r2, s2 = Wr.call(c, out_cap=cap)
        assert b2 is None and r2 is None and s2 == dict(s, error=Wr.E_CAPACITY)
    assert Wr.call(c, out_cap=T)[0] == blob
    for i, (name, entries) in enumerate((("stts", 1 << 29), ("ctts", 1 << 29), ("stss", 1 << 30), ("stsc", 357913941), ("stsz", 1 << 30), ("stco", 1 << 30))):
        b2, _, s2 = Wr.call(c, entries_override={name: entries})
        assert b2 is None and s2 == Wr.summary(Wr.E_ARG, s["nal_count"], bad_box=i + 1), name
        assert Wr.call(c, entries_override={name: entries - 8})[2]["error"] == 0
