"""hbs_rtp_pack on the CPU side: the symbols and the record sizes, a fixed vector the plain restatement of the rule
(tests/_rtp_ref.py) must give, hbs_rtp_nal_packets_host and hbs_rtp_packet_host against that restatement, and the restatement
through its own receiver."""
import numpy as np
import pytest

from tests import _rtp_ref as R
from tests._rtp_ref import random_case


def test_symbols_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    for name in ("hbs_rtp_pack", "hbs_rtp_nal_packets_host", "hbs_rtp_packet_host"):
        assert name in declared_functions()
        assert name in EXPORTS
        assert hasattr(hbs.load_library(), name)
    assert hasattr(hbs.Context, "rtp_pack") and hasattr(hbs.Context, "rtp_pack_async")
    assert hbs.RTP_PARAMS.itemsize == 32 and hbs.RTP_PARAMS == R.PARAMS
    assert hbs.RTP_PACKET.itemsize == 72 and hbs.RTP_PACKET == R.PACKET
    assert hbs.RTP_OPEN_END == R.OPEN_END == 1
    assert (hbs.RTP_SINGLE, hbs.RTP_FU, hbs.RTP_AP, hbs.RTP_OTHER) == (R.SINGLE, R.FU, R.AP, R.OTHER) == (0, 1, 2, 3)
    assert callable(hbs.rtp_nal_packets) and callable(hbs.rtp_packet) and callable(hbs.rtp_packet_offsets)
    assert np.array_equal(hbs.rtp_params(**R.params(seq=7)), R.params_record(R.params(seq=7)))


FIXED_NAL = bytes.fromhex("4001AABBCCDDEE")
FIXED_PACKETS = (bytes.fromhex("8060FFFF01020304A1B2C3D46201A0AABBCC"), bytes.fromhex("80E0000001020304A1B2C3D4620160DDEE"))


@pytest.mark.parametrize("framing", (0, 2))
def test_the_fixed_vector(framing):
    """so that the reference is not its own judge"""
    prm = R.params(max_payload=6, payload_type=96, seq=0xFFFF, ts_base=0x01020304, ts_step=0, ssrc=0xA1B2C3D4, framing=framing)
    stream = np.frombuffer(FIXED_NAL, dtype=np.uint8)
    out, nal_off, nal_packet, s = R.pack(stream, R.entries([0], [7]), np.zeros(1, dtype=np.uint32), 1, None, prm)
    prefix = (b"\x00\x12", b"\x00\x11") if framing else (b"", b"")
    assert out.tobytes() == prefix[0] + FIXED_PACKETS[0] + prefix[1] + FIXED_PACKETS[1]
    assert nal_off.tolist() == [0, 35 + 2 * framing] and nal_packet.tolist() == [0, 2]
    assert s == dict(nal_count=2, nal_found=1, rbsp_bytes=7, stream_bytes=35 + 2 * framing, stop_reason=0, error=0, reserved=[0, 2, 1])
    assert R.packet_offsets(nal_off, nal_packet, prm).tolist() == [0, 18 + framing, 35 + 2 * framing]


def test_nal_packets_host_against_the_reference():
    import hevcbitstream_amd as hbs
    for mp in (4, 5, 6, 16, 19, 100, 1188, 65523):
        for L in range(0, 601):
            assert hbs.rtp_nal_packets(L, mp) == R.nal_packets(L, mp), (L, mp)
    for L, mp in ((1 << 40, 1188), (65523, 65523), (65524, 65523), (65526 + 65520, 65523), (65527 + 65520, 65523)):
        assert hbs.rtp_nal_packets(L, mp) == R.nal_packets(L, mp) > 0
    for mp in (3, 0, -1, 65524, 1 << 20):
        assert hbs.rtp_nal_packets(100, mp) == 0
    assert hbs.rtp_nal_packets(1, 100) == 0 and hbs.rtp_nal_packets(0, 100) == 0 and hbs.rtp_nal_packets(2, 100) == 1


def same_packet(got, want):
    for k, v in want.items():
        g = got[k].tolist() if k == "nal_header" else int(got[k])
        assert g == v, (k, g, v)
    assert got["reserved"].tolist() == [0, 0]


def test_packet_host_on_every_packet_the_reference_writes():
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(5)
    seen = set()
    for mp, framing in ((4, 0), (5, 2), (16, 0), (19, 2), (100, 0), (1188, 2)):
        prm = R.params(max_payload=mp, framing=framing, seq=int(rng.integers(0, 65536)), ts_base=int(rng.integers(0, 1 << 32)),
                       payload_type=int(rng.integers(0, 128)))
        stream, index, nal_au, n_aus, pts = random_case(rng, 60, max_nal=4 * mp + 10)
        out, nal_off, nal_packet, s = R.pack(stream, index, nal_au, n_aus, pts, prm)
        assert s["error"] == 0
        off = R.packet_offsets(nal_off, nal_packet, prm)
        assert np.array_equal(off, hbs.rtp_packet_offsets(nal_off, nal_packet, mp, framing))
        for j in range(len(off) - 1):
            pkt = out[int(off[j]) + framing:int(off[j + 1])].tobytes()
            want = R.read_packet(pkt)
            same_packet(hbs.rtp_packet(pkt), want)
            assert want["seq"] == (prm["seq"] + j) & 0xFFFF
            seen.add(want["kind"])
    assert seen == {R.SINGLE, R.FU}


def test_packet_host_on_hand_made_packets():
    """CSRC entries, a header extension and padding, by RFC 3550; aggregation packets, PACI and short payloads by kind"""
    import hevcbitstream_amd as hbs
    lib = hbs.load_library()
    fixed = bytes([0x80, 0x60, 0x02, 0x03, 0x11, 0x22, 0x33, 0x44, 0xA1, 0xB2, 0xC3, 0xD4])
    single, fu = bytes.fromhex("4201AABBCC"), bytes.fromhex("6203935566")
    csrc, ext = bytes(range(12)), bytes([0xBE, 0xDE, 0x00, 0x02]) + bytes(8)
    pad = bytes([0, 0, 0, 4])
    cases = [(0x80, b"", single, b""), (0x83, csrc, single, b""), (0x90, ext, fu, b""), (0xA0, b"", single, pad), (0xB3, csrc + ext, fu, pad),
             (0xA0, b"", single, b"\x01"), (0x90, bytes([0, 0, 0, 0]), single, b""), (0x80, b"", bytes.fromhex("6001FFFF"), b""),
             (0x80, b"", bytes.fromhex("6401FFFF"), b""), (0x80, b"", b"\x42", b""), (0x80, b"", b"", b""), (0x80, b"", bytes.fromhex("7E01"), b"")]
    kinds = []
    for b0, front, payload, back in cases:
        pkt = bytes([b0]) + fixed[1:] + front + payload + back
        want = R.read_packet(pkt)
        assert want is not None and want["payload_off"] == 12 + len(front) and want["payload_len"] == len(payload)
        got = hbs.rtp_packet(pkt)
        same_packet(got, want)
        kinds.append(int(got["kind"]))
    assert kinds == [R.SINGLE, R.SINGLE, R.FU, R.SINGLE, R.FU, R.SINGLE, R.SINGLE, R.AP, R.OTHER, R.OTHER, R.OTHER, R.OTHER]
    got = hbs.rtp_packet(bytes([0xB3]) + fixed[1:] + csrc + ext + fu + pad)
    assert (int(got["fu_start"]), int(got["fu_end"]), int(got["nal_type"]), got["nal_header"].tolist()) == (1, 0, 19, [0x26, 0x03])
    assert (int(got["marker"]), int(got["payload_type"]), int(got["seq"]), int(got["timestamp"]), int(got["ssrc"])) == (0, 0x60, 0x0203, 0x11223344, 0xA1B2C3D4)
    assert (int(got["nal_off"]), int(got["nal_len"])) == (12 + 12 + 12 + 3, 2)
    # refused: another version, shorter than its own fields say
    out = np.zeros(1, dtype=R.PACKET)
    refused = [bytes([0x40]) + fixed[1:] + single, bytes([0x00]) + fixed[1:] + single, fixed[:11], bytes([0x81]) + fixed[1:] + b"\x00\x00",
               bytes([0x90]) + fixed[1:] + b"\xBE\xDE\x00", bytes([0x90]) + fixed[1:] + b"\xBE\xDE\x00\x02" + bytes(7),
               bytes([0xA0]) + fixed[1:] + single + b"\x00", bytes([0xA0]) + fixed[1:] + b"\x42\x01\x04", bytes([0x80]) + fixed[1:] + b"\x62\x01"]
    for pkt in refused:
        a = np.frombuffer(pkt, dtype=np.uint8)
        assert R.read_packet(pkt) is None, pkt.hex()
        assert lib.hbs_rtp_packet_host(a.ctypes.data, len(a), out.ctypes.data) == R.E_ARG, pkt.hex()
    ok = np.frombuffer(bytes([0x80]) + fixed[1:] + single, dtype=np.uint8)
    assert lib.hbs_rtp_packet_host(None, 17, out.ctypes.data) == R.E_ARG and lib.hbs_rtp_packet_host(ok.ctypes.data, 17, None) == R.E_ARG
    assert lib.hbs_rtp_packet_host(ok.ctypes.data, 17, out.ctypes.data) == 0
    with pytest.raises(hbs.HbsError):
        hbs.rtp_packet(refused[0])


@pytest.mark.parametrize("framing", (0, 2))
def test_pack_then_unpack_is_the_identity(framing):
    rng = np.random.default_rng(9 + framing)
    for mp in (4, 5, 16, 19, 100, 1188):
        for flags in (0, R.OPEN_END):
            prm = R.params(max_payload=mp, framing=framing, flags=flags, seq=65530, ts_base=0xFFFFF000, ts_step=3003)
            for with_pts in (True, False):
                stream, index, nal_au, n_aus, pts = random_case(rng, 80, max_nal=3 * mp + 20, times=with_pts)
                out, nal_off, nal_packet, s = R.pack(stream, index, nal_au, n_aus, pts, prm)
                assert s["error"] == 0 and len(out) == s["stream_bytes"] and s["nal_count"] == s["reserved"][1] == int(nal_packet[-1])
                nals, aus, times, packets = R.unpack(out, R.packet_offsets(nal_off, nal_packet, prm), prm)
                assert nals == [stream[int(a):int(b)].tobytes() for a, b in zip(index["start"], index["end"])]
                rel = (nal_au - nal_au[0]).astype(np.int64)
                assert aus == rel.tolist()
                assert times == [(prm["ts_base"] + (int(pts[a]) if with_pts else a * 3003)) & R.M32 for a in rel]
                assert bool(packets[-1]["marker"]) == (flags == 0)
                assert sum(p["marker"] for p in packets) == n_aus - (1 if flags else 0)


def test_the_reference_names_the_lowest_malformed_nal():
    rng = np.random.default_rng(11)
    stream, index, nal_au, n_aus, pts = random_case(rng, 40)
    prm = R.params(max_payload=100)
    assert R.pack(stream, index, nal_au, n_aus, pts, prm)[3]["error"] == 0
    need = R.pack(stream, index, nal_au, n_aus, pts, prm)[3]["stream_bytes"]
    assert R.pack(stream, index, nal_au, n_aus, pts, prm, out_cap=need)[3]["error"] == 0
    assert R.pack(stream, index, nal_au, n_aus, pts, prm, out_cap=need - 1)[3]["error"] == R.E_CAPACITY
    bad = stream.copy()
    bad[int(index["start"][7])] = 49 << 1
    bad[int(index["start"][30])] = 48 << 1
    assert R.pack(bad, index, nal_au, n_aus, pts, prm)[3]["reserved"][0] == 8
    late = pts.copy()
    late[int(nal_au[5] - nal_au[0])] = 1 << 33
    s = R.pack(bad, index, nal_au, n_aus, late, prm)[3]
    first = int(np.flatnonzero(nal_au == nal_au[5])[0])
    assert s["error"] == R.E_ARG and s["reserved"][0] == first + 1 <= 6


def test_the_vectorised_reference_equals_the_loop():
    rng = np.random.default_rng(13)
    for framing, flags, with_aus, with_pts in ((0, 0, True, True), (2, R.OPEN_END, True, False), (2, 0, False, True), (0, 0, False, False)):
        prm = R.params(max_payload=40, framing=framing, flags=flags, seq=65000, ts_base=0xFFFFFF00, ts_step=77)
        stream, index, nal_au, n_aus, pts = random_case(rng, 900, max_nal=41, aus=with_aus, times=with_pts)
        a, b = R.pack(stream, index, nal_au, n_aus, pts, prm), R.pack_single_packets(stream, index, nal_au, n_aus, pts, prm)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
