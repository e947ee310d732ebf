"""hbs_ts_demux on the CPU side: the symbols and record sizes, hbs_ts_packet_host -- the function the kernels run -- on packets
worked out by hand and on random ones against the plain restatement of the rule (tests/_ts_ref.py), and hbs_ts_find_pid_host
on muxed heads."""
import numpy as np
import pytest

from tests import _ts_ref as R

PID = 0x100


def test_symbols_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    for name in ("hbs_ts_demux", "hbs_ts_packet_host", "hbs_ts_find_pid_host"):
        assert name in declared_functions()
        assert name in EXPORTS
        assert hasattr(hbs.load_library(), name)
    assert hasattr(hbs.Context, "ts_demux") and hasattr(hbs.Context, "ts_demux_async")
    assert hbs.TS_PES.itemsize == 32 and hbs.TS_PES == R.TS_PES and hbs.TS_PACKET.itemsize == 48
    assert callable(hbs.ts_packet) and callable(hbs.ts_find_pid)


def hexpkt(head, fill="AB"):
    """188 bytes: the hex string `head`, then `fill` repeated"""
    b = bytes.fromhex(head.replace(" ", ""))
    return b + bytes.fromhex(fill) * (188 - len(b))


def got(pkt, pid=PID, B=188):
    import hevcbitstream_amd as hbs
    r = hbs.ts_packet(pkt, pid, B)
    return {k: int(r[k]) for k in r.dtype.names}


def check(pkt, **want):
    g = got(pkt, PID)
    assert g == R.classify(pkt, PID), (g, R.classify(pkt, PID))
    for k, v in want.items():
        assert g[k] == v, (k, g[k], v)
    return g


def test_hand_worked_packets():
    # PID 0x100, payload only, cc 7
    check(hexpkt("47 01 00 17"), cls=R.PAYLOAD, off=4, len=184, es_off=4, es_len=184, cc=7, flags=0, pts=R.NO_TIME, dts=R.NO_TIME)
    # a PES start with a PTS of 90000: 21 00 05 BF 21; header_data_length 5 -> H = 14
    check(hexpkt("47 41 00 10  00 00 01 E0 00 00 80 80 05  21 00 05 BF 21"), cls=R.PES_START, off=4, len=184, es_off=18, es_len=170,
          flags=R.F_PTS, pts=90000, dts=90000)
    # PTS 90000 + DTS 86400 (31 00 05 BF 21 / 11 00 05 A3 01), data_alignment_indicator, two stuffing bytes: H = 9 + 12
    check(hexpkt("47 41 00 1F  00 00 01 E0 00 00 84 C0 0C  31 00 05 BF 21  11 00 05 A3 01  FF FF"), cls=R.PES_START, es_off=25,
          es_len=163, cc=15, flags=R.F_PTS | R.F_DTS | R.F_ALIGN, pts=90000, dts=86400)
    # the top bits: PTS 2^33 - 1
    check(hexpkt("47 41 00 10  00 00 01 E0 00 00 80 80 05  2F FF FF FF FF"), pts=(1 << 33) - 1)
    # no time stamps, header_data_length 0: the ES bytes begin 9 bytes in
    check(hexpkt("47 41 00 10  00 00 01 E0 00 00 80 00 00"), cls=R.PES_START, es_off=13, es_len=175, flags=0, pts=R.NO_TIME)
    # the other PID; the null PID
    check(hexpkt("47 01 01 17"), cls=R.OTHER, pid=0x101)
    check(hexpkt("47 1F FF 10"), cls=R.OTHER, pid=0x1FFF)
    # sync loss is a fault whatever the PID
    check(hexpkt("46 01 00 17"), cls=R.FAULT)
    check(hexpkt("48 1F FF 17"), cls=R.FAULT)
    # transport_error_indicator; scrambling: skipped, and nothing else looked at (an adaptation_field_length of 255 behind)
    check(hexpkt("47 81 00 30 FF"), cls=R.SKIPPED)
    check(hexpkt("47 01 00 B0 FF"), cls=R.SKIPPED)
    check(hexpkt("47 01 00 50"), cls=R.SKIPPED)


def test_adaptation_field_control_and_length():
    # afc 1: payload only.  afc 2: adaptation field only, no payload whatever its length.  afc 0 (reserved): no payload
    check(hexpkt("47 01 00 13"), cls=R.PAYLOAD, off=4, len=184)
    check(hexpkt("47 01 00 23 B7 00"), cls=R.NO_PAYLOAD, off=188)
    check(hexpkt("47 01 00 23 07 C0"), cls=R.NO_PAYLOAD, off=12, flags=R.F_DI | R.F_RAI)
    check(hexpkt("47 01 00 03"), cls=R.NO_PAYLOAD, off=4)
    check(hexpkt("47 41 00 23 B7 00"), cls=R.NO_PAYLOAD)                 # payload_unit_start is ignored without a payload
    # afc 3, adaptation_field_length 0: one byte of adaptation field, no flags byte (the byte behind is payload: C0 is no flag)
    check(hexpkt("47 01 00 33 00 C0"), cls=R.PAYLOAD, off=5, len=183, flags=0)
    # 1: the flags byte alone
    check(hexpkt("47 01 00 33 01 80"), cls=R.PAYLOAD, off=6, len=182, flags=R.F_DI)
    check(hexpkt("47 01 00 33 01 40"), cls=R.PAYLOAD, off=6, len=182, flags=R.F_RAI)
    # 182: one payload byte.  183: none.  184: past the packet, a fault
    check(hexpkt("47 01 00 33 B6 00", "FF"), cls=R.PAYLOAD, off=187, len=1, es_off=187, es_len=1)
    check(hexpkt("47 01 00 33 B7 00", "FF"), cls=R.NO_PAYLOAD, off=188, len=0)
    check(hexpkt("47 01 00 33 B8 00", "FF"), cls=R.FAULT)
    check(hexpkt("47 01 00 23 B8 00", "FF"), cls=R.FAULT)
    check(hexpkt("47 01 00 33 FF 00", "FF"), cls=R.FAULT)
    # the three packet sizes: the same transport bytes behind a 4-byte prefix / in front of 16 parity bytes
    pkt = hexpkt("47 41 00 10  00 00 01 E0 00 00 80 80 05  21 00 05 BF 21")
    want = got(pkt)
    assert got(b"\x47\x47\x47\x47" + pkt, B=192) == want and got(pkt + b"\x47" * 16, B=204) == want


def test_each_pes_fault():
    ok = "47 41 00 10  00 00 01 E0 00 00 80 80 05  21 00 05 BF 21"
    assert check(hexpkt(ok))["cls"] == R.PES_START
    for bad in ("47 41 00 10  00 00 02 E0 00 00 80 80 05  21 00 05 BF 21",      # no packet_start_code_prefix
                "47 41 00 10  01 00 01 E0 00 00 80 80 05  21 00 05 BF 21",
                "47 41 00 10  00 00 01 E0 00 00 00 80 05  21 00 05 BF 21",      # not '10': an MPEG-1 header
                "47 41 00 10  00 00 01 E0 00 00 C0 80 05  21 00 05 BF 21",
                "47 41 00 10  00 00 01 E0 00 00 80 40 05  21 00 05 BF 21",      # PTS_DTS_flags '01'
                "47 41 00 10  00 00 01 E0 00 00 80 80 04  21 00 05 BF 21",      # a PTS needs 5 bytes
                "47 41 00 10  00 00 01 E0 00 00 80 C0 09  31 00 05 BF 21 11 00 05 A3 01",   # PTS + DTS need 10
                "47 41 00 10  00 00 01 E0 00 00 80 80 B0  21 00 05 BF 21"):     # the header ends behind the packet: 9 + 176 > 184
        check(hexpkt(bad), cls=R.FAULT, pid=PID)
    # the header may end exactly at the packet's end: no ES bytes
    check(hexpkt("47 41 00 10  00 00 01 E0 00 00 80 80 AF  21 00 05 BF 21"), cls=R.PES_START, es_off=188, es_len=0, pts=90000)
    # a payload too short for a PES header (8 bytes); 9 bytes are enough
    check(hexpkt("47 41 00 30 AF 00", "FF")[:180] + bytes.fromhex("00 00 01 E0 00 00 80 00"), cls=R.FAULT)
    check(hexpkt("47 41 00 30 AE 00", "FF")[:179] + bytes.fromhex("00 00 01 E0 00 00 80 00 00"), cls=R.PES_START, es_len=0)


def random_packet(rng, count):
    """one packet whose fields are drawn so that every branch of the rule comes up; count: what was planted"""
    b = bytearray(rng.integers(0, 256, size=188, dtype=np.uint8).tobytes())
    b[0] = 0x47 if rng.random() < 0.97 else int(rng.integers(0, 256))
    pid = PID if rng.random() < 0.85 else int(rng.integers(0, 8192))
    tei = rng.random() < 0.04
    tsc = int(rng.integers(1, 4)) if rng.random() < 0.04 else 0
    pusi = rng.random() < 0.5
    afc = int(rng.choice([0, 1, 1, 2, 3, 3, 3]))
    b[1] = tei << 7 | pusi << 6 | pid >> 8
    b[2] = pid & 0xFF
    b[3] = tsc << 6 | afc << 4 | int(rng.integers(0, 16))
    afl = int(rng.choice([0, 1, 2, 7, 100, 170, 174, 175, 176, 182, 183, 184, 200, 255, int(rng.integers(0, 184))]))
    off = 4
    if afc & 2:
        b[4] = afl
        off = 5 + afl
    if pusi and (afc & 1) and off + 9 <= 188:
        f = int(rng.choice([0, 2, 3, 1])) if rng.random() < 0.9 else 1
        need = {0: 0, 1: 0, 2: 5, 3: 10}[f]
        q8 = need + int(rng.integers(0, 4))
        what = rng.choice(["ok", "ok", "ok", "prefix", "mpeg1", "short", "long", "fill"])
        if what == "short" and need:
            q8 = need - 1
        if what == "long":
            q8 = 188 - off - 9 + 1 + int(rng.integers(0, 20))
        if what == "fill":
            q8 = 188 - off - 9
        q8 = min(q8, 255)
        b[off:off + 3] = b"\x00\x00\x01" if what != "prefix" else bytes([0, int(rng.integers(0, 2)), int(rng.integers(2, 256))])
        b[off + 6] = (0x80 if what != "mpeg1" else int(rng.choice([0x00, 0x40, 0xC0]))) | int(rng.integers(0, 64))
        b[off + 7] = f << 6 | int(rng.integers(0, 64))
        b[off + 8] = q8
        count["planted " + str(what)] = count.get("planted " + str(what), 0) + 1
    return bytes(b)


def test_random_packets_against_the_rule():
    rng = np.random.default_rng(2024)
    count = {}
    n = 24000
    for _ in range(n):
        pkt = random_packet(rng, count)
        g = got(pkt)
        w = R.classify(pkt, PID)
        assert g == w, (pkt.hex(), g, w)
        count[w["cls"]] = count.get(w["cls"], 0) + 1
        for name, bit in (("pts", R.F_PTS), ("dts", R.F_DTS), ("rai", R.F_RAI), ("di", R.F_DI), ("align", R.F_ALIGN)):
            if w["flags"] & bit:
                count[name] = count.get(name, 0) + 1
        if w["cls"] == R.PES_START and w["es_len"] == 0:
            count["empty es"] = count.get("empty es", 0) + 1
        if w["cls"] == R.FAULT and pkt[0] == 0x47:
            why = "afl" if (pkt[3] & 0x20 and pkt[4] > 183) else "pes"
            count["fault " + why] = count.get("fault " + why, 0) + 1
        if w["cls"] == R.FAULT and pkt[0] != 0x47:
            count["fault sync"] = count.get("fault sync", 0) + 1
        if w["cls"] == R.NO_PAYLOAD:
            key = "no payload, afc %d" % ((pkt[3] >> 4) & 3)
            count[key] = count.get(key, 0) + 1
    for key in (R.FAULT, R.OTHER, R.SKIPPED, R.NO_PAYLOAD, R.PAYLOAD, R.PES_START, "pts", "dts", "rai", "di", "align", "empty es",
                "fault afl", "fault pes", "fault sync", "no payload, afc 0", "no payload, afc 2", "no payload, afc 3",
                "planted ok", "planted prefix", "planted mpeg1", "planted short", "planted long", "planted fill"):
        assert count.get(key, 0) > 0, (key, count)


def test_packet_host_refuses_bad_arguments():
    import ctypes as C
    import hevcbitstream_amd as hbs
    lib = hbs.load_library()
    pkt = np.frombuffer(hexpkt("47 01 00 17"), dtype=np.uint8).copy()
    out = np.zeros(1, dtype=hbs.TS_PACKET)
    for B, pid in ((187, PID), (0, PID), (189, PID), (188, -1), (188, 8192)):
        assert lib.hbs_ts_packet_host(pkt.ctypes.data, B, pid, out.ctypes.data) == -3
    assert lib.hbs_ts_packet_host(None, 188, PID, out.ctypes.data) == -3 and lib.hbs_ts_packet_host(pkt.ctypes.data, 188, PID, None) == -3
    assert lib.hbs_ts_packet_host(pkt.ctypes.data, 188, 8191, out.ctypes.data) == 0 and int(out["cls"][0]) == R.OTHER
    assert C.sizeof(C.c_int) == 4


# ---- hbs_ts_find_pid_host -------------------------------------------------------------------------------------------------------

def find(parts, B=188, stream_type=0x24):
    import hevcbitstream_amd as hbs
    return hbs.ts_find_pid(b"".join(parts), B, stream_type)


@pytest.mark.parametrize("B", R.SIZES)
def test_find_pid_on_muxed_heads(B):
    other = R.packet(0x101, b"\x47" * 184, cc=3, B=B)
    null = R.packet(R.NULL_PID, b"\xFF" * 184, B=B)
    pat1 = R.section_packet(0, R.pat([(1, 0x1000)]), B=B)
    pmt1 = R.section_packet(0x1000, R.pmt(1, [(0x0F, 0x101, b""), (0x24, 0x100, b"\x05\x04HEVC"), (0x24, 0x102, b"")]), B=B)
    assert find([pat1, pmt1], B) == (0x100, 1)
    assert find([pat1, pmt1], B, stream_type=0x0F) == (0x101, 1)
    # the PMT behind other packets (and one in front of the PAT); a pointer_field that skips bytes
    assert find([other, null, pat1, other, other, null, pmt1, other], B) == (0x100, 1)
    assert find([pmt1, other, pat1], B) == (0x100, 1)
    ptr = R.section_packet(0x1000, R.pmt(1, [(0x24, 0x123, b"")], info=b"\x09\x04abcd"), pointer=9, B=B)
    assert find([R.section_packet(0, R.pat([(1, 0x1000)]), pointer=5, B=B), ptr], B) == (0x123, 1)
    # two programs, the network PID entry (program 0) in front: the first real program's PMT decides
    pat2 = R.section_packet(0, R.pat([(0, 0x10), (7, 0x1001), (8, 0x1000)]), B=B)
    pmt7 = R.section_packet(0x1001, R.pmt(7, [(0x1B, 0x200, b""), (0x24, 0x201, b"")]), B=B)
    assert find([pat2, pmt1, pmt7], B) == (0x201, 7)
    # no HEVC stream; no PMT; no PAT; a PAT with the network entry alone; nothing at all; half a packet
    assert find([pat1, R.section_packet(0x1000, R.pmt(1, [(0x1B, 0x200, b""), (0x0F, 0x201, b"")]), B=B)], B) is None
    assert find([pat1, other, null], B) is None and find([pmt1, other], B) is None
    assert find([R.section_packet(0, R.pat([(0, 0x10)]), B=B), pmt1], B) is None
    assert find([], B) is None and find([pat1[: B // 2]], B) is None
    # a section that leaves its packet: a PAT of 60 programs (252 bytes), a PMT whose length says more than the packet holds
    big = R.pat([(k + 1, 0x1000 + k) for k in range(60)])
    assert find([R.packet(0, b"\x00" + big[:183], pusi=1, B=B), pmt1], B) is None
    long_pmt = bytearray(R.pmt(1, [(0x24, 0x100, b"")]))
    long_pmt[2] = 0xB5
    assert find([pat1, R.section_packet(0x1000, bytes(long_pmt), B=B)], B) is None
    assert find([pat1, R.packet(0x1000, bytes([183]) + b"\xFF" * 183, pusi=1, B=B)], B) is None      # the pointer_field points behind the packet
    # hostile lengths inside a section that does lie inside its packet: program_info_length / ES_info_length past its end
    evil = bytearray(R.pmt(1, [(0x1B, 0x200, b""), (0x24, 0x100, b"")]))
    evil[10:12] = b"\xFF\xFF"
    assert find([pat1, R.section_packet(0x1000, bytes(evil), B=B)], B) is None
    evil = bytearray(R.pmt(1, [(0x1B, 0x200, b""), (0x24, 0x100, b"")]))
    evil[15:17] = b"\xFF\xFF"
    assert find([pat1, R.section_packet(0x1000, bytes(evil), B=B)], B) is None


def test_the_reference_demux_on_a_muxed_stream():
    """the muxer and the plain loop agree with each other: units in, units out, times as stamped"""
    rng = np.random.default_rng(5)
    units = [rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 900, size=40)]
    times = [(3000 * k + 7, 3000 * k if k % 3 else None) for k in range(40)]
    for B in R.SIZES:
        ts, begins = R.mux_units(units, PID, B, times, rng)
        import hevcbitstream_amd as hbs
        assert hbs.ts_find_pid(ts[: 20 * B], B) == (PID, 1)
        out, pes, s = R.demux(ts, B, PID)
        assert out.tobytes() == b"".join(units) and s["error"] == 0 and s["reserved"] == [0, 0, 0]
        assert pes["packet"].tolist() == begins
        assert pes["out_off"].tolist() == np.cumsum([0] + [len(u) for u in units[:-1]]).tolist()
        assert pes["pts"].tolist() == [t[0] for t in times]
        assert pes["dts"].tolist() == [t[1] if t[1] is not None else t[0] for t in times]
