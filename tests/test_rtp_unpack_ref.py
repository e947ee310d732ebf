"""hbs_rtp_unpack on the CPU side: the symbols and the record size, a fixed hand-written vector the plain restatement of the rule
(tests/_rtp_unpack_ref.py) must give, the round trip from tests/_rtp_ref.pack, a lost packet, hbs_rtp_frames_host against a
Python walk, and hbs_rtp_packet_host on the inputs of tests/test_rtp_abi.py."""
import numpy as np
import pytest

from tests import _rtp_ref as R
from tests import _rtp_unpack_ref as U


def test_symbols_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    for name in ("hbs_rtp_unpack", "hbs_rtp_frames_host"):
        assert name in declared_functions()
        assert name in EXPORTS
        assert hasattr(hbs.load_library(), name)
    assert hasattr(hbs.Context, "rtp_unpack") and hasattr(hbs.Context, "rtp_unpack_async")
    assert hbs.RTP_UNPACK_PARAMS.itemsize == 16 and hbs.RTP_UNPACK_PARAMS == U.PARAMS
    assert hbs.RTPU_MATCH_SSRC == U.MATCH_SSRC == 1
    assert callable(hbs.rtp_frames)
    assert np.array_equal(hbs.rtp_unpack_params(**U.params(flags=1)), U.params_record(U.params(flags=1)))


HEAD = "A1B2C3D4"          # the ssrc
FIXED = [
    # seq 0xFFFE, ts 0x01020304: a single NAL 40 01 AA
    bytes.fromhex("8060FFFE01020304" + HEAD + "4001AA"),
    # seq 0xFFFF, same ts, marker: an aggregation packet of 42 01 BB and 44 01 -> the second ends the AU
    bytes.fromhex("80E0FFFF01020304" + HEAD + "6001" + "0003" + "4201BB" + "0002" + "4401"),
    # seq 0, 1, 2, ts 0x01020400: three fragments of 26 01 11 22 33 44 55 (type 19), the last with the marker
    bytes.fromhex("8060000001020400" + HEAD + "620193" + "1122"),
    bytes.fromhex("8060000101020400" + HEAD + "620113" + "33"),
    bytes.fromhex("80E0000201020400" + HEAD + "620153" + "4455"),
    # seq 4 (3 was lost): an orphan last fragment, dropped; one sequence break
    bytes.fromhex("8060000401020500" + HEAD + "620153" + "99"),
]
FIXED_OUT = "00000001" + "4001AA" + "00000001" + "4201BB" + "00000001" + "4401" + "00000001" + "26011122334455"


@pytest.mark.parametrize("sc", (4, 3))
def test_the_fixed_vector(sc):
    """so that the reference is not its own judge"""
    data, off, size = U.lay_out(FIXED)
    got = U.unpack(data, off, size, U.params(startcode_bytes=sc, ssrc=0xA1B2C3D4))
    want = bytes.fromhex(FIXED_OUT)
    if sc == 3:
        want = want.replace(b"\x00\x00\x00\x01", b"\x00\x00\x01")
    assert got["out"].tobytes() == want
    assert got["nals"] == [bytes.fromhex(x) for x in ("4001AA", "4201BB", "4401", "26011122334455")]
    starts = [sc, 2 * sc + 3, 3 * sc + 6, 4 * sc + 8]
    assert got["index"]["start"].tolist() == starts and got["index"]["end"].tolist() == [starts[0] + 3, starts[1] + 3, starts[2] + 2, starts[3] + 7]
    assert got["index"]["status"].tolist() == [0, 0, 0, U.ST_UNTERMINATED] and not got["index"]["rbsp_off"].any() and not got["index"]["rbsp_len"].any()
    assert got["nal_au"].tolist() == [0, 0, 0, 1] and got["au_ts"].tolist() == [0x01020304, 0x01020400]
    assert got["summary"] == dict(nal_count=4, nal_found=6, rbsp_bytes=15, stream_bytes=15 + 4 * sc, stop_reason=-1, error=0,
                                  reserved=[0, 2, 1 << 32 | 1])


CASES = [(framing, mp, seed) for framing in (0, 2) for mp, seed in ((4, 1), (5, 2), (7, 3), (19, 4), (33, 5), (60, 6))]


@pytest.mark.parametrize("framing,mp,seed", CASES)
def test_round_trip_from_the_packing_reference(framing, mp, seed):
    rng = np.random.default_rng(100 * framing + seed)
    prm = R.params(max_payload=mp, framing=framing, seq=int(rng.integers(0, 65536)), ts_base=int(rng.integers(0, 1 << 32)))
    stream, index, nal_au, n_aus, pts = R.random_case(rng, 70, max_nal=3 * mp + 20)
    pts = np.sort(rng.choice(1 << 20, size=n_aus, replace=False)).astype(np.uint64)            # distinct times: an AU is known by its time
    out, nal_off, nal_packet, s = R.pack(stream, index, nal_au, n_aus, pts, prm)
    off = R.packet_offsets(nal_off, nal_packet, prm)
    pkt_off, pkt_size = off[:-1] + np.uint64(framing), np.diff(off) - np.uint64(framing)
    for sc in (3, 4):
        got = U.unpack(out, pkt_off, pkt_size, U.params(startcode_bytes=sc, ssrc=prm["ssrc"]))
        want_nals = [stream[int(a):int(b)].tobytes() for a, b in zip(index["start"], index["end"])]
        assert got["nals"] == want_nals
        assert got["out"].tobytes() == b"".join(bytes(sc - 1) + b"\x01" + n for n in want_nals)
        assert got["nal_au"].tolist() == (nal_au - nal_au[0]).tolist()
        assert got["au_ts"].tolist() == [(prm["ts_base"] + int(t)) & R.M32 for t in pts]
        assert got["summary"]["reserved"] == [0, n_aus, 0] and got["summary"]["nal_found"] == len(pkt_off)
    if framing:
        f_off, f_size, used = U.frames(out)
        assert np.array_equal(f_off, pkt_off) and np.array_equal(f_size, pkt_size) and used == len(out)


@pytest.mark.parametrize("framing,mp,seed", CASES[::3])
def test_one_packet_removed(framing, mp, seed):
    """exactly the NAL of the removed packet is missing: its other packets are dropped, and there is one sequence break unless
    the removed packet was the first or the last"""
    rng = np.random.default_rng(200 + 100 * framing + seed)
    prm = R.params(max_payload=mp, framing=framing, seq=65500)
    stream, index, nal_au, n_aus, pts = R.random_case(rng, 25, max_nal=3 * mp + 20)
    out, nal_off, nal_packet, s = R.pack(stream, index, nal_au, n_aus, pts, prm)
    off = R.packet_offsets(nal_off, nal_packet, prm)
    pkt_off, pkt_size = off[:-1] + np.uint64(framing), np.diff(off) - np.uint64(framing)
    nal_of = np.repeat(np.arange(len(index)), np.diff(nal_packet).astype(np.int64))
    want_nals = [stream[int(a):int(b)].tobytes() for a, b in zip(index["start"], index["end"])]
    uprm = U.params(ssrc=prm["ssrc"])
    for gone in range(len(pkt_off)):
        keep = np.arange(len(pkt_off)) != gone
        got = U.unpack(out, pkt_off[keep], pkt_size[keep], uprm)
        k = int(nal_of[gone])
        assert got["nals"] == want_nals[:k] + want_nals[k + 1:], gone
        others = int((nal_of == k).sum()) - 1
        brk = 0 if gone in (0, len(pkt_off) - 1) else 1
        assert got["summary"]["reserved"][2] == brk << 32 | others, gone
        assert got["summary"]["nal_found"] == len(pkt_off) - 1 and got["summary"]["error"] == 0


def test_the_reference_on_foreign_unsupported_and_faulty_packets():
    rng = np.random.default_rng(7)
    nal = U.random_nal(rng, 30)
    f = U.fu_payloads(nal, 10)
    assert len(f) == 3
    ok = [U.packet(U.random_nal(rng, 5), 9, 50), U.packet(f[0], 10, 60), U.packet(f[1], 11, 60), U.packet(f[2], 12, 60, marker=1)]
    prm = U.params()
    whole = U.unpack(*U.lay_out(ok), prm)
    assert whole["nals"][1] == nal and whole["summary"]["reserved"] == [0, 2, 0]
    # another payload type between two NALs changes nothing but the count of accepted packets; inside the chain it drops the NAL
    foreign = U.packet(b"\x40\x01", 77, 1, pt=97)
    got = U.unpack(*U.lay_out([ok[0], foreign] + ok[1:]), prm)
    assert got["nals"] == whole["nals"] and got["summary"]["nal_found"] == 4 and got["summary"]["reserved"] == [0, 2, 0]
    got = U.unpack(*U.lay_out(ok[:2] + [foreign] + ok[2:]), prm)
    assert got["nals"] == whole["nals"][:1] and got["summary"]["reserved"] == [0, 1, 3]
    # the same with another ssrc, looked at only with MATCH_SSRC
    alien = U.packet(b"\x40\x01\x55", 77, 60, ssrc=5)
    assert len(U.unpack(*U.lay_out(ok[:2] + [alien] + ok[2:]), prm)["nals"]) == 2          # a single NAL of its own, the chain broken
    got = U.unpack(*U.lay_out(ok[:2] + [alien] + ok[2:]), U.params(flags=U.MATCH_SSRC))
    assert got["nals"] == whole["nals"][:1] and got["summary"]["nal_found"] == 4
    # PACI and a payload of one byte are dropped and counted; S and E in one packet is a NAL; an empty fragment is accepted
    paci, short = U.packet(bytes([50 << 1, 1, 0, 0]), 13, 60), U.packet(b"\x40", 14, 60)
    se = U.packet(bytes([0x62, 0x01, 0xC0 | 19]) + b"\x77", 15, 70)
    empties = [U.packet(bytes([0x62, 0x01, 0x80 | 1]), 16, 80), U.packet(bytes([0x62, 0x01, 1]), 17, 80), U.packet(bytes([0x62, 0x01, 0x40 | 1]), 18, 80)]
    got = U.unpack(*U.lay_out(ok + [paci, short, se] + empties), prm)
    assert got["nals"][2:] == [b"\x26\x01\x77", b"\x02\x01"] and got["summary"]["reserved"][2] == 2 and got["summary"]["nal_found"] == 10
    # faults: the lowest is named
    bad_fu = U.packet(bytes([0x62, 0x01, 0x80 | 48, 1]), 19, 90)
    for bad, where in ((bad_fu, 2), (U.packet(U.ap_payload([]), 1, 1), 0), (U.packet(U.ap_payload([b"\x40"]), 1, 1), 1), (b"\x40" + ok[0][1:], 3),
                       (U.packet(U.ap_payload([b"\x40\x01"]) + b"\x00", 1, 1), 2), (U.packet(U.ap_payload([b"\x40\x01"])[:-1], 1, 1), 1),
                       (U.packet(U.ap_payload([bytes([48 << 1, 1])]), 1, 1), 0)):
        pk = list(ok)
        pk.insert(where, bad)
        pk.append(bad_fu)
        got = U.unpack(*U.lay_out(pk), prm)
        assert got["summary"]["error"] == U.E_ARG and got["summary"]["reserved"] == [where + 1, 0, 0] and len(got["out"]) == 0
    data, off, size = U.lay_out(ok)
    size[2] = len(data) - int(off[2]) + 1
    assert U.unpack(data, off, size, prm)["summary"]["reserved"][0] == 3
    off[1] = (1 << 64) - 4
    assert U.unpack(data, off, size, prm)["summary"]["reserved"][0] == 2
    # capacities
    need = whole["summary"]["stream_bytes"]
    assert U.unpack(*U.lay_out(ok), prm, out_cap=need, nal_cap=2, au_cap=2)["summary"]["error"] == 0
    for caps in (dict(out_cap=need - 1, nal_cap=2, au_cap=2), dict(out_cap=need, nal_cap=1, au_cap=2), dict(out_cap=need, nal_cap=2, au_cap=1)):
        got = U.unpack(*U.lay_out(ok), prm, **caps)
        assert got["summary"]["error"] == U.E_CAPACITY and got["summary"]["nal_count"] == 2 and len(got["out"]) == 0


def test_frames_host_against_a_python_walk():
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(3)
    packets = [rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() for n in (12, 0, 1, 300, 65535, 13, 2)]
    stream = b"".join(len(p).to_bytes(2, "big") + p for p in packets)
    want = U.frames(stream)
    assert want[2] == len(stream) and want[1].tolist() == [len(p) for p in packets]
    off, size, used, frames = hbs.rtp_frames(stream)
    assert np.array_equal(off, want[0]) and np.array_equal(size, want[1]) and used == want[2] and frames == len(packets)
    # a truncated tail: every cut
    tail = len(stream) - (2 + len(packets[-1]) + 2 + len(packets[-2]))
    for cut in list(range(0, 20)) + list(range(tail - 3, len(stream) + 1)):
        part = stream[:cut]
        w = U.frames(part)
        off, size, used, frames = hbs.rtp_frames(part)
        assert np.array_equal(off, w[0]) and np.array_equal(size, w[1]) and used == w[2] and frames == len(w[0]), cut
        assert used <= cut and all(int(o) + int(s) <= cut for o, s in zip(off, size))
    # cap smaller than the frame count: the first `cap` entries, all frames counted
    for cap in (0, 1, 3, 7, 9):
        off, size, used, frames = hbs.rtp_frames(stream, cap=cap)
        assert frames == len(packets) and used == len(stream) and len(off) == min(cap, len(packets))
        assert np.array_equal(off, want[0][:cap]) and np.array_equal(size, want[1][:cap])
    for nothing in (b"", b"\x00", b"\x00\x01"):
        off, size, used, frames = hbs.rtp_frames(nothing)
        assert len(off) == 0 and len(size) == 0 and used == 0 and frames == 0
    # the table goes into the receiver
    ok = [U.packet(U.random_nal(rng, 9), 5, 1), U.packet(U.random_nal(rng, 4), 6, 1, marker=1)]
    framed = b"".join(len(p).to_bytes(2, "big") + p for p in ok)
    off, size, used, _ = hbs.rtp_frames(framed + b"\x00")
    assert used == len(framed) and len(U.unpack(np.frombuffer(framed, dtype=np.uint8), off, size, U.params())["nals"]) == 2


def test_packet_host_is_unchanged_on_the_inputs_of_test_rtp_abi():
    """the rule behind hbs_rtp_packet_host is now the host/device function the kernels run: the same answers as before"""
    from tests import test_rtp_abi as T
    T.test_packet_host_on_every_packet_the_reference_writes()
    T.test_packet_host_on_hand_made_packets()
    import hevcbitstream_amd as hbs
    for pkt in FIXED:
        T.same_packet(hbs.rtp_packet(pkt), R.read_packet(pkt))


def test_the_vectorised_reference_equals_the_loop():
    rng = np.random.default_rng(17)
    for framing, mp, sc in ((0, 9, 4), (2, 30, 3), (0, 400, 4)):
        prm = R.params(max_payload=mp, framing=framing, seq=65400, ts_base=0xFFFFFF00, ts_step=77)
        stream, index, nal_au, n_aus, pts = R.random_case(rng, 300, max_nal=3 * mp, times=False)
        out, nal_off, nal_packet, _ = R.pack(stream, index, nal_au, n_aus, None, prm)
        off = R.packet_offsets(nal_off, nal_packet, prm)
        pkt_off, pkt_size = off[:-1] + np.uint64(framing), np.diff(off) - np.uint64(framing)
        uprm = U.params(startcode_bytes=sc)
        a, b = U.unpack(out, pkt_off, pkt_size, uprm), U.unpack_plain(out, pkt_off, pkt_size, uprm)
        for k in ("out", "index", "nal_au", "au_ts"):
            assert np.array_equal(a[k], b[k]), k
        assert a["summary"] == b["summary"]
