"""HBS_RTP_AGGREGATE on the CPU side: the constants and the params record, the plain restatement (tests/_rtp_ap_ref.py) against
hand-written packets for the edges of the group rule, the restatement through an independent reader (tests/_rtp_unpack_ref.py),
hbs_rtp_ap_units_host and rtp_packet_offsets against the restatement."""
import os
import re

import numpy as np
import pytest

from tests import _rtp_ref as R
from tests import _rtp_ap_ref as A
from tests import _rtp_unpack_ref as U
from tests._rtp_ref import random_case


def test_symbols_constants_and_the_params_record():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    assert "hbs_rtp_ap_units_host" in declared_functions() and "hbs_rtp_ap_units_host" in EXPORTS
    assert hasattr(hbs.load_library(), "hbs_rtp_ap_units_host")
    assert hbs.RTP_AGGREGATE == A.AGGREGATE == 4 and hbs.RTP_AP_SPAN == A.AP_SPAN == 256 and hbs.RTP_OPEN_END == 1
    assert callable(hbs.rtp_ap_units)
    prm = R.params(flags=hbs.RTP_AGGREGATE | hbs.RTP_OPEN_END, seq=9)
    assert np.array_equal(hbs.rtp_params(**prm), R.params_record(prm)) and int(hbs.rtp_params(**prm)["flags"][0]) == 5


def test_the_header_names_the_flag():
    """fails on a library without the feature: HBS_RTP_AGGREGATE is not in the header"""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(here, "include", "hevcbitstream_amd.h")).read()
    assert re.search(r"#define\s+HBS_RTP_AGGREGATE\s+4u", text) and re.search(r"#define\s+HBS_RTP_AP_SPAN\s+256", text)
    assert "no aggregation packets" not in text


def ap(prm, marker, j, ts, hdr, nals):
    body = bytes(hdr) + b"".join(len(x).to_bytes(2, "big") + x for x in nals)
    p = R.header(prm, marker, j, ts) + body
    return (len(p).to_bytes(2, "big") if prm["framing"] else b"") + p


def single(prm, marker, j, ts, nal):
    p = R.header(prm, marker, j, ts) + nal
    return (len(p).to_bytes(2, "big") if prm["framing"] else b"") + p


def case_of(nals, aus=None):
    starts = np.concatenate([[0], np.cumsum([len(x) for x in nals[:-1]])]).astype(np.int64)
    stream = np.frombuffer(b"".join(nals), dtype=np.uint8)
    index = R.entries(starts, starts + np.array([len(x) for x in nals]))
    return stream, index, (np.array(aus, dtype=np.uint32) if aus is not None else None)


@pytest.mark.parametrize("framing", (0, 2))
def test_hand_written_packets(framing):
    """so that the restatement is not its own judge"""
    a, b, c, d = bytes.fromhex("4001AA"), bytes.fromhex("C3FA"), bytes.fromhex("4E09BBCCDD"), bytes.fromhex("0201")
    hdr_abc = [0xE0, 0x01]                                                     # F from b, layer 0 from a, tid 1 from a and c
    # one access unit, everything fits: one AP, marker from its last unit
    prm = R.params(max_payload=100, framing=framing, flags=A.AGGREGATE, seq=0xFFFF, ts_base=5, ssrc=0xA1B2C3D4)
    stream, index, _ = case_of([a, b, c])
    out, off, pkt, s = A.pack(stream, index, None, 0, None, prm)
    assert out.tobytes() == ap(prm, True, 0, 5, hdr_abc, [a, b, c])
    h = framing + 14
    assert off.tolist() == [0, h + 2 + 3, h + 2 + 3 + 2 + 2, len(out)] and pkt.tolist() == [0, 0, 0, 1]
    assert s == dict(nal_count=1, nal_found=3, rbsp_bytes=10, stream_bytes=len(out), stop_reason=0, error=0, reserved=[0, 1, 1 << 32])
    assert len(out) == framing + 12 + 2 + 2 + 3 + 2 + 2 + 2 + 5
    # the payload is exactly mp = 2 + 5 + 4 + 7 = 18; with mp = 17 c is alone
    hdr_ab = [0xE0, 0x01]
    assert A.payload_hdr([(a[0], a[1]), (b[0], b[1])]) == bytes(hdr_ab) and A.payload_hdr([(x[0], x[1]) for x in (a, b, c)]) == bytes(hdr_abc)
    out, off, pkt, s = A.pack(stream, index, None, 0, None, dict(prm, max_payload=18))
    assert out.tobytes() == ap(prm, True, 0, 5, hdr_abc, [a, b, c])
    out, off, pkt, s = A.pack(stream, index, None, 0, None, dict(prm, max_payload=17))
    assert out.tobytes() == ap(prm, False, 0, 5, hdr_ab, [a, b]) + single(prm, True, 1, 5, c)
    assert pkt.tolist() == [0, 0, 1, 2] and s["reserved"] == [0, 2, 1 << 32]
    # an access unit boundary inside a would-be group; OPEN_END takes the marker off the last AP
    stream, index, aus = case_of([a, b, c, d], [7, 7, 8, 8])
    prm2 = dict(prm, flags=A.AGGREGATE | R.OPEN_END, ts_step=10)
    out, off, pkt, s = A.pack(stream, index, aus, 2, None, prm2)
    want = ap(prm2, True, 0, 5, A.payload_hdr([(0x40, 0x01), (0xC3, 0xFA)]), [a, b]) + \
        ap(prm2, False, 1, 15, A.payload_hdr([(0x4E, 0x09), (0x02, 0x01)]), [c, d])
    assert out.tobytes() == want and pkt.tolist() == [0, 0, 1, 1, 2] and s["reserved"] == [0, 2, 2 << 32]
    assert A.payload_hdr([(0x4E, 0x09), (0x02, 0x01)]) == bytes([0x60, 0x01])
    assert A.payload_hdr([(0x41, 0x0B), (0x01, 0xFA)]) == bytes([0x61, 0x0A])      # layers 33 and 63: 33; tids 3 and 2: 2
    # mp = 10 with 2-byte NALs: pairs; mp = 9: no AP, the flag-less output
    twos = [bytes([2 * k, k + 1]) for k in range(5)]
    stream, index, _ = case_of(twos)
    out, off, pkt, s = A.pack(stream, index, None, 0, None, dict(prm, max_payload=10))
    assert pkt.tolist() == [0, 0, 1, 1, 2, 3] and s["reserved"] == [0, 3, 2 << 32]
    assert out.tobytes() == ap(prm, False, 0, 5, A.payload_hdr([(0, 1), (2, 2)]), twos[:2]) + \
        ap(prm, False, 1, 5, A.payload_hdr([(4, 3), (6, 4)]), twos[2:4]) + single(prm, True, 2, 5, twos[4])
    nine = A.pack(stream, index, None, 0, None, dict(prm, max_payload=9))
    plain = R.pack(stream, index, None, 0, None, dict(prm, max_payload=9, flags=0))
    assert np.array_equal(nine[0], plain[0]) and np.array_equal(nine[1], plain[1]) and np.array_equal(nine[2], plain[2]) and nine[3] == plain[3]
    # L = mp (single), L = mp + 1 (FUs), L = mp - 4 (fits alone, pairs with nothing), each between small NALs
    mp = 40
    big = [bytes([0x02, 0x01]) + bytes(range(L - 2)) for L in (mp, mp + 1, mp - 4)]
    nals = [d, big[0], d, d, big[1], d, big[2], d]
    stream, index, _ = case_of(nals)
    out, off, pkt, s = A.pack(stream, index, None, 0, None, dict(prm, max_payload=mp))
    assert pkt.tolist() == [0, 1, 2, 2, 3, 5, 6, 7, 8] and s["reserved"] == [0, 8, 1 << 32 | 1]


def test_the_cut_at_every_multiple_of_the_span():
    sizes, rel = [2] * 600, [0] * 600
    g = A.groups(sizes, rel, 65523)
    assert g == [(0, 256), (256, 512), (512, 600)]
    assert A.groups([2, 2, 2], [0, 0, 1], 100) == [(0, 2), (2, 3)]
    assert A.groups([2, 92, 2, 2], [0] * 4, 100) == [(0, 2), (2, 4)] and A.groups([2, 93, 2, 2], [0] * 4, 100) == [(0, 1), (1, 2), (2, 4)]


@pytest.mark.parametrize("framing", (0, 2))
def test_through_an_independent_reader(framing):
    """the packets of the restatement, read by the restatement of hbs_rtp_unpack: exactly the NALs, AU numbers and timestamps;
    never longer than the flag-less output; flag off is tests/_rtp_ref.py"""
    rng = np.random.default_rng(21 + framing)
    kinds = set()
    for mp in (10, 19, 100, 1188):
        for flags in (A.AGGREGATE, A.AGGREGATE | R.OPEN_END):
            for with_pts in (True, False):
                prm = R.params(max_payload=mp, framing=framing, flags=flags, seq=65500, ts_base=0xFFFFF000, ts_step=3003)
                stream, index, nal_au, n_aus, pts = random_case(rng, 300, max_nal={10: 5, 19: 38, 100: 200, 1188: 900}[mp], times=with_pts)
                out, nal_off, nal_packet, s = A.pack(stream, index, nal_au, n_aus, pts, prm)
                plain = R.pack(stream, index, nal_au, n_aus, pts, dict(prm, flags=flags & ~A.AGGREGATE))
                off_out = A.pack(stream, index, nal_au, n_aus, pts, dict(prm, flags=flags & ~A.AGGREGATE))
                assert all(np.array_equal(x, y) for x, y in zip(plain[:3], off_out[:3])) and plain[3] == off_out[3]
                assert s["error"] == 0 and len(out) == s["stream_bytes"] <= plain[3]["stream_bytes"]
                assert s["reserved"][2] >> 32 > 0 and s["nal_count"] == int(nal_packet[-1]) == s["reserved"][1]
                assert s["stream_bytes"] == plain[3]["stream_bytes"] - sum(
                    (m - 1) * (framing + 12) - 2 - 2 * m for m in np.bincount(nal_packet[:-1].astype(np.int64)) if m > 1)
                offs = A.packet_offsets(nal_off, nal_packet, prm)
                assert len(offs) == s["nal_count"] + 1 and (np.diff(offs.astype(np.int64)) - framing - 12 <= mp).all()
                got = U.unpack(out, offs[:-1] + np.uint64(framing), np.diff(offs) - np.uint64(framing), U.params())
                assert got["summary"]["error"] == 0 and got["summary"]["reserved"][2] == 0
                assert got["nals"] == [stream[int(a):int(b)].tobytes() for a, b in zip(index["start"], index["end"])]
                rel = (nal_au - nal_au[0]).astype(np.int64)
                want_ts = [(prm["ts_base"] + (int(pts[a]) if with_pts else a * 3003)) & R.M32 for a in rel]
                assert got["nal_au"].tolist() == rel.tolist()
                assert got["au_ts"].tolist() == [want_ts[int(np.flatnonzero(rel == a)[0])] for a in range(n_aus)]
                for j in range(len(offs) - 1):
                    r = R.read_packet(out[int(offs[j]) + framing:int(offs[j + 1])].tobytes())
                    assert r["seq"] == (prm["seq"] + j) & 0xFFFF
                    kinds.add(r["kind"])
    assert kinds == {R.SINGLE, R.FU, R.AP}


def test_ap_units_and_packet_offsets_against_the_restatement():
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(23)
    aps = 0
    for mp, framing in ((19, 0), (100, 2), (1188, 0)):
        prm = R.params(max_payload=mp, framing=framing, flags=A.AGGREGATE, seq=3)
        stream, index, nal_au, n_aus, pts = random_case(rng, 200, max_nal=mp + 30)
        out, nal_off, nal_packet, s = A.pack(stream, index, nal_au, n_aus, pts, prm)
        offs = A.packet_offsets(nal_off, nal_packet, prm)
        assert np.array_equal(hbs.rtp_packet_offsets(nal_off, nal_packet, mp, framing), offs)
        first = {int(nal_packet[k]): k for k in range(len(index) - 1, -1, -1)}
        for j in range(len(offs) - 1):
            pkt = out[int(offs[j]) + framing:int(offs[j + 1])].tobytes()
            units = A.ap_units(pkt)
            if R.read_packet(pkt)["kind"] != R.AP:
                assert units is None
                with pytest.raises(hbs.HbsError):
                    hbs.rtp_ap_units(pkt)
                continue
            aps += 1
            o, z = hbs.rtp_ap_units(pkt)
            assert list(zip(o.tolist(), z.tolist())) == units and len(units) >= 2
            k = first[j]
            for i, (uo, us) in enumerate(units):                                # the tables name the same bytes
                assert us == int(index["end"][k + i] - index["start"][k + i])
                assert int(nal_off[k + i]) == (int(offs[j]) if i == 0 else int(offs[j]) + framing + uo - 2)
    assert aps > 50
    # without shared packets the result is what it was
    prm = R.params(max_payload=50, framing=2)
    stream, index, nal_au, n_aus, pts = random_case(rng, 100, max_nal=300)
    _, nal_off, nal_packet, _ = R.pack(stream, index, nal_au, n_aus, pts, prm)
    assert np.array_equal(hbs.rtp_packet_offsets(nal_off, nal_packet, 50, 2), R.packet_offsets(nal_off, nal_packet, prm))
    assert hbs.rtp_packet_offsets([0], [0], 50, 2).tolist() == [0]


def test_ap_units_host_refusals():
    import hevcbitstream_amd as hbs
    lib = hbs.load_library()
    fixed = bytes([0x80, 0x60, 0x02, 0x03, 0x11, 0x22, 0x33, 0x44, 0xA1, 0xB2, 0xC3, 0xD4])
    good = fixed + bytes.fromhex("6001" "0002" "4201" "0003" "4401AA")
    o, z = hbs.rtp_ap_units(good)
    assert o.tolist() == [16, 20] and z.tolist() == [2, 3]
    one = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    a = np.frombuffer(good, dtype=np.uint8)
    assert lib.hbs_rtp_ap_units_host(a.ctypes.data, len(a), one[0].ctypes.data, one[1].ctypes.data, 1) == 2      # counted beyond cap
    assert (int(one[0][0]), int(one[1][0])) == (16, 2)
    assert lib.hbs_rtp_ap_units_host(a.ctypes.data, len(a), None, None, 1) == R.E_ARG
    bad = [fixed + bytes.fromhex("6001"),                              # no unit
           fixed + bytes.fromhex("6001" "00"),                         # a byte for a size
           fixed + bytes.fromhex("6001" "0001" "42"),                  # a size below 2
           fixed + bytes.fromhex("6001" "0003" "4201"),                # a size beyond what is left
           fixed + bytes.fromhex("6001" "0002" "4201" "0004" "6001" "0000"),   # a nested AP
           fixed + bytes.fromhex("6001" "0002" "6201"),                # an FU inside
           fixed + bytes.fromhex("4201AA"),                            # a single NAL unit packet
           fixed[:11], b""]
    for pkt in bad:
        assert A.ap_units(pkt) is None, pkt.hex()
        with pytest.raises(hbs.HbsError):
            hbs.rtp_ap_units(pkt)
