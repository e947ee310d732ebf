"""hbs_mp4_fragment's plain restatement (tests/_mp4_ref.py) on the CPU: the writer against the reader that knows nothing of it,
two vectors worked out by hand, and hbs_mp4_init_host / hbs_mp4_fragment_bytes_host through the binding against the writer."""
import numpy as np
import pytest

from tests import _mp4_ref as R
from tests._mp4_ref import random_case

FRAGMENT_HEX = """
00000068 6D6F6F66
  00000010 6D666864 00000000 00000007
  00000050 74726166
    00000010 74666864 00020000 00000001
    00000014 74666474 01000000 00000000 00015F90
    00000024 7472756E 01000F01 00000001 00000070
      00000BB8 00000009 02000000 00000000
00000011 6D646174
  00000005 2601AABBCC
"""
SPS = bytes.fromhex("420101 01 600000 03 00 900000 03 0000 03 00 5D A0028080")
HVCC_HEX = """
0000003A 68766343
  01  01 60000000 900000000000 5D  F000 FC FD F8 F8 0000 0F 01
  A1 0001 0016 4201010160000003009000000300000300 5DA0028080
"""
VPS = bytes.fromhex("40010C01FFFF016000000300900000030000030078959809")
PPS = bytes.fromhex("4401C172B46240")


def unhex(s):
    return bytes.fromhex("".join(s.split()))


def test_a_one_sample_fragment_by_hand():
    stream = np.frombuffer(b"\x00\x00\x01" + unhex("2601AABBCC"), dtype=np.uint8)
    out, off, size, frags, s = R.fragment(stream, R.entries([3], [8]), None, np.array([41], np.uint32), R.au_records([1]), None, None,
                                          R.params(length_size=4, sequence=7, track_id=1, sample_duration=3000, base_time=90000))
    assert out.tobytes() == unhex(FRAGMENT_HEX)
    assert off.tolist() == [112] and size.tolist() == [9] and s["stream_bytes"] == 121 == R.fragment_bytes(1, 9)
    assert frags.tolist() == [(0, 121, 0, 90000, 1, 7, 1, 0)]
    f, = R.read_fragments(out)
    assert f["samples"] == [(112, 9, 3000, 0x02000000, 0)] and (f["sequence"], f["track_id"], f["decode_time"]) == (7, 1, 90000)


def test_an_hvcc_by_hand_with_emulation_prevention_in_the_profile_bytes():
    assert R.strip_epb(SPS)[:15] == unhex("420101 01 60000000 900000000000 5D")
    seg = R.init_segment([SPS])
    assert unhex(HVCC_HEX) in seg and seg.endswith(unhex("00000028 6D766578 00000020 74726578 00000000 00000001 00000001") + bytes(12))
    got = R.read_init(seg)
    assert got["arrays"] == [(0xA1, [SPS])] and got["entry"] == b"hvc1" and got["config"] == unhex(HVCC_HEX)[8:30]


def check_against_reader(out, off, size, frags, s, stream, index, keep, nal_au, au, dts, pts, prm):
    got = R.read_fragments(out)
    assert len(got) == len(frags) == s["nal_count"]
    table = [x for f in got for x in f["samples"]]
    assert [x[0] for x in table] == off.tolist() and [x[1] for x in table] == size.tolist()
    assert [f["off"] for f in got] == frags["out_off"].tolist() and [f["bytes"] for f in got] == frags["out_bytes"].tolist()
    assert [f["sequence"] for f in got] == [(prm["sequence"] + r) & R.M32 for r in range(len(got))]
    assert all(f["track_id"] == prm["track_id"] for f in got)
    first = np.cumsum([0] + [len(f["samples"]) for f in got])[:-1]
    assert first.tolist() == frags["first_au"].tolist()
    n_aus = len(au)
    d = [int(dts[a]) if dts is not None else prm["base_time"] + a * prm["sample_duration"] for a in range(n_aus)]
    assert [f["decode_time"] for f in got] == [d[a] for a in first]
    assert [x[2] for x in table] == [d[a + 1] - d[a] for a in range(n_aus - 1)] + [prm["sample_duration"]]
    assert [x[4] for x in table] == [(int(pts[a]) - d[a]) if pts is not None else 0 for a in range(n_aus)]
    assert [x[3] for x in table] == [0x02000000 if f & 1 else 0x01010000 for f in au["flags"].tolist()]
    # the cuts
    M = prm["max_samples"]
    for f, a0 in zip(got, first):
        assert M == 0 or len(f["samples"]) <= M
    if prm["flags"] & R.CUT_AT_IRAP:
        assert {a for a in range(n_aus) if au["flags"][a] & 1} <= set(first.tolist())
    elif M == 0:
        assert len(got) == 1
    # the payloads
    rel = (nal_au.astype(np.int64) - int(nal_au[0])) & R.M32
    b = out.tobytes()
    for a, (o, z, _, _, _) in enumerate(table):
        want = [stream[int(index["start"][k]):int(index["end"][k])].tobytes() for k in np.flatnonzero(rel == a) if keep is None or keep[k]]
        assert R.samples_to_nals(b, o, z, prm["length_size"]) == want


def test_writer_against_reader():
    rng = np.random.default_rng(5)
    for case in range(120):
        L = (1, 2, 4)[case % 3]
        mode = case % 4
        prm = R.params(length_size=L, flags=R.CUT_AT_IRAP if mode in (1, 3) else 0, track_id=int(rng.integers(1, 1 << 32)),
                       sequence=int(rng.integers((1 << 32) - 3, 1 << 32)) if case % 5 == 0 else int(rng.integers(0, 1 << 32)),
                       max_samples=(0, 0, 1, 3)[mode], sample_duration=int(rng.integers(0, 1 << 32)),
                       base_time=int(rng.integers(0, 1 << 50)))
        c = random_case(rng, int(rng.integers(1, 40)), max_nal=255 if L == 1 else 400, keep_some=case % 2 == 0, times=case % 3 != 1,
                        irap_every=(None, 1, 2, 3, 4, 7)[case % 6])
        res = R.fragment(*c, prm)
        assert res[4]["error"] == 0, res[4]
        check_against_reader(*res, *c, prm)


def test_writer_errors():
    rng = np.random.default_rng(6)
    stream, index, keep, nal_au, au, dts, pts = random_case(rng, 12, keep_some=False)
    prm = R.params()
    n = len(index)

    def err(**kw):
        a = dict(stream=stream, index=index.copy(), keep=keep, nal_au=nal_au.copy(), au=au, dts=dts.copy(), pts=pts.copy())
        a.update(kw)
        return R.fragment(a["stream"], a["index"], a["keep"], a["nal_au"], a["au"], a["dts"], a["pts"], kw.get("prm", prm))[4]
    i2 = index.copy(); i2["end"][5] = len(stream) + 1
    assert err(index=i2)["reserved"][:2] == [6, 0] and err(index=i2)["error"] == R.E_ARG
    na = nal_au.copy(); na[n - 1] += 1
    assert err(nal_au=na)["reserved"][0] == n
    d2 = dts.copy(); d2[3] = (1 << 64) - 1
    assert err(dts=d2)["reserved"][:2] == [0, 3]          # AU 2's duration is out of range first
    p2 = pts.copy(); p2[0] = dts[0] + np.uint64(1 << 31)
    assert err(pts=p2)["reserved"][:2] == [0, 1]
    assert err(index=i2, pts=p2)["reserved"][:2] == [6, 1]
    assert err(prm=R.params(length_size=1), index=R.entries([0], [256]), nal_au=np.zeros(1, np.uint32), au=au[:1], dts=None, pts=None,
               stream=np.zeros(256, np.uint8))["reserved"][0] == 1
    big = R.fragment(stream, index, keep, nal_au, au, None, None, R.params(base_time=(1 << 62) - 1 - 5 * 7, sample_duration=7))[4]
    assert big["reserved"][:2] == [0, 7]


def test_init_host_against_the_writer():
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(8)
    assert hbs.mp4_init([VPS, SPS, PPS]) == R.init_segment([VPS, SPS, PPS])
    for case in range(60):
        nals = [(VPS, SPS, PPS)[int(t)] + bytes(rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8)) for t in rng.integers(0, 3, size=int(rng.integers(1, 7)))]
        nals.insert(int(rng.integers(0, len(nals) + 1)), SPS[:18 + case % 5])
        kw = dict(track_id=int(rng.integers(1, (1 << 32) - 1)), timescale=int(rng.integers(1, 1 << 32)), width=int(rng.integers(1, 65536)),
                  height=int(rng.integers(1, 65536)), length_size=(1, 2, 4)[case % 3], chroma_format_idc=case % 4,
                  bit_depth_luma=8 + case % 8, bit_depth_chroma=8 + (case // 2) % 8, flags=case & 1)
        want = R.init_segment(nals, **kw)
        assert hbs.mp4_init(nals, **kw) == want
        got = R.read_init(want)
        assert got["entry"] == (b"hev1" if case & 1 else b"hvc1") and got["track_id"] == kw["track_id"] and got["timescale"] == kw["timescale"]
        assert (got["width"], got["height"]) == (kw["width"], kw["height"])
        for head, of in got["arrays"]:
            assert head >> 7 == 1 - (case & 1) and of == [x for x in nals if (x[0] >> 1) & 0x3F == head & 0x3F]
        assert [h & 0x3F for h, _ in got["arrays"]] == sorted(h & 0x3F for h, _ in got["arrays"])
    big = SPS + bytes(65535 - len(SPS))
    assert hbs.mp4_init([big]) == R.init_segment([big])


def test_init_host_refusals():
    import hevcbitstream_amd as hbs
    ok = [VPS, SPS, PPS]
    short_sps = bytes.fromhex("420101 01 600000 03 00 900000 03 0000 03 00")          # 14 bytes once stripped
    assert len(R.strip_epb(short_sps)) == 14 and len(R.strip_epb(short_sps + b"\x5D")) == 15
    assert hbs.mp4_init([short_sps + b"\x5D"]) == R.init_segment([short_sps + b"\x5D"])
    for nals, kw in (([VPS, PPS], {}), ([short_sps], {}), ([SPS, b"\x42"], {}), ([SPS, SPS + bytes(65536 - len(SPS))], {}), ([SPS, b"\x46\x01\x50"], {}),
                     ([SPS, b"\x3E\x01\x50"], {}), ([], {}), (ok, dict(track_id=0)), (ok, dict(track_id=(1 << 32) - 1)), (ok, dict(timescale=0)),
                     (ok, dict(width=0)), (ok, dict(width=65536)), (ok, dict(height=0)), (ok, dict(height=65536)), (ok, dict(length_size=3)),
                     (ok, dict(length_size=0)), (ok, dict(chroma_format_idc=4)), (ok, dict(chroma_format_idc=-1)), (ok, dict(bit_depth_luma=7)),
                     (ok, dict(bit_depth_luma=16)), (ok, dict(bit_depth_chroma=7)), (ok, dict(bit_depth_chroma=16)), (ok, dict(flags=2))):
        assert R.init_segment(nals, **kw) == R.E_ARG, (nals, kw)
        with pytest.raises(hbs.HbsError):
            hbs.mp4_init(nals, **kw)
    # too little room: the size comes back and nothing is written
    lib = hbs.load_library()
    import ctypes as C
    prm = np.zeros(1, dtype=hbs.MP4_INIT_PARAMS)
    prm[0] = (1, 90000, 1920, 1080, 4, 1, 8, 8)
    buf = np.frombuffer(SPS, dtype=np.uint8).copy()
    ptrs, sizes = (C.c_void_p * 1)(buf.ctypes.data), np.array([len(SPS)], dtype=np.uint64)
    want = R.init_segment([SPS])
    out = np.full(len(want), 0xC3, dtype=np.uint8)
    a = (prm.ctypes.data, 0, C.cast(ptrs, C.c_void_p), sizes.ctypes.data, 1)
    assert lib.hbs_mp4_init_host(*a, out.ctypes.data, len(want) - 1) == len(want) and (out == 0xC3).all()
    assert lib.hbs_mp4_init_host(*a, out.ctypes.data, len(want)) == len(want) and out.tobytes() == want
    assert lib.hbs_mp4_init_host(None, 0, C.cast(ptrs, C.c_void_p), sizes.ctypes.data, 1, None, 0) == R.E_ARG
    assert lib.hbs_mp4_init_host(prm.ctypes.data, 0, None, sizes.ctypes.data, 1, None, 0) == R.E_ARG
    assert lib.hbs_mp4_init_host(prm.ctypes.data, 0, C.cast(ptrs, C.c_void_p), None, 1, None, 0) == R.E_ARG
    assert lib.hbs_mp4_init_host(*a, None, 10) == R.E_ARG


def test_fragment_bytes_host():
    import hevcbitstream_amd as hbs
    for S, P in ((0, 0), (1, 9), (40, 12345), (1 << 28, (1 << 32) - 9)):
        assert hbs.mp4_fragment_bytes(S, P) == R.fragment_bytes(S, P) == 96 + 16 * S + P
