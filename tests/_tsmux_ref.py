"""hbs_ts_mux restated as one plain loop over the access units and their packets (include/hevcbitstream_amd.h is the
specification), with a bitwise CRC.  Test infrastructure: numpy only, no GPU, nothing of the library."""
import numpy as np

from tests._segments import materialise, run_of

ACCESS_UNIT = np.dtype([("first_nal", "<u8"), ("unit_begin", "<u8"), ("unit_end", "<u8"), ("nal_count", "<u4"), ("vcl_count", "<u4"),
                        ("first_vcl", "<u4"), ("nal_unit_type", "<i4"), ("temporal_id_plus1", "<i4"), ("pic_order_cnt", "<i4"),
                        ("poc_lsb", "<i4"), ("slice_types", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
PARAMS = np.dtype([("packet_bytes", "<i4"), ("pid", "<i4"), ("pmt_pid", "<i4"), ("program_number", "<i4"),
                   ("transport_stream_id", "<i4"), ("flags", "<u4"), ("cc_es", "<u4"), ("cc_pat", "<u4"), ("cc_pmt", "<u4"),
                   ("reserved", "<u4"), ("pcr_lead", "<u8")])
AU_IRAP = 1
PCR, PSI_AT_IRAP, NO_PSI = 1, 2, 4
NO_TIME = (1 << 64) - 1
E_ARG, E_CAPACITY = -3, -4
SIZES = (188, 192, 204)
MASK33 = (1 << 33) - 1


def params(pid=0x100, pmt_pid=0x1000, packet_bytes=188, program_number=1, transport_stream_id=1, flags=0, cc_es=0, cc_pat=0, cc_pmt=0,
           pcr_lead=0, reserved=0):
    return dict(packet_bytes=packet_bytes, pid=pid, pmt_pid=pmt_pid, program_number=program_number, transport_stream_id=transport_stream_id,
                flags=flags, cc_es=cc_es, cc_pat=cc_pat, cc_pmt=cc_pmt, reserved=reserved, pcr_lead=pcr_lead)


def params_record(prm):
    p = np.zeros(1, dtype=PARAMS)
    for k, v in prm.items():
        p[k][0] = v
    return p


def aus(begins, ends, irap=None):
    """an ACCESS_UNIT table with the three fields the call reads; the others hold junk it must not look at"""
    n = len(begins)
    a = np.frombuffer(np.random.default_rng(n).integers(0, 256, size=n * ACCESS_UNIT.itemsize, dtype=np.uint8).tobytes(), dtype=ACCESS_UNIT).copy()
    a["unit_begin"] = np.asarray(begins, dtype=np.uint64)
    a["unit_end"] = np.asarray(ends, dtype=np.uint64)
    a["flags"] &= ~np.uint32(AU_IRAP)
    if irap is not None:
        a["flags"] |= np.asarray(irap, dtype=bool).astype(np.uint32) * np.uint32(AU_IRAP)
    return a


def random_case(rng, n, prm, max_es=900, gaps=True):
    """n AUs with random sizes, gaps, times of every form and IRAP flags -> (stream, au, pts, dts)"""
    sizes = rng.integers(0, max_es, size=n)
    gap = rng.integers(0, 20, size=n) * (rng.random(n) < 0.5) if gaps else np.zeros(n, dtype=np.int64)
    begins = np.cumsum(gap + np.concatenate([[0], sizes[:-1]])) if n else np.zeros(0, dtype=np.int64)
    ends = begins + sizes
    stream = rng.integers(0, 256, size=int(ends[-1]) if n else 0, dtype=np.uint8)
    form = rng.integers(0, 3, size=n)
    pts = np.where(form == 0, NO_TIME, rng.integers(0, 1 << 33, size=n, dtype=np.uint64)).astype(np.uint64)
    dts = np.where(form == 2, rng.integers(0, 1 << 33, size=n, dtype=np.uint64), np.where(rng.random(n) < 0.5, pts, NO_TIME)).astype(np.uint64)
    dts = np.where(form == 0, NO_TIME, dts).astype(np.uint64)
    return stream, aus(begins, ends, rng.random(n) < 0.2), pts, dts


def crc32(data):
    """MPEG-2 CRC-32, bit by bit: polynomial 0x04C11DB7, initial value 0xFFFFFFFF, not reflected, no final xor"""
    crc = 0xFFFFFFFF
    for byte in bytes(data):
        for bit in range(7, -1, -1):
            top = (crc >> 31) & 1
            crc = (crc << 1) & 0xFFFFFFFF
            if top ^ ((byte >> bit) & 1):
                crc ^= 0x04C11DB7
    return crc


def section_packet(pid, cc, section):
    section = bytes(section)
    section += crc32(section).to_bytes(4, "big")
    body = bytes([0x47, 0x40 | pid >> 8, pid & 0xFF, 0x10 | (cc & 15), 0]) + section
    return body + b"\xFF" * (188 - len(body))


def psi(prm, k=0):
    """the k-th PAT / PMT pair"""
    pid, pmt_pid, prog, tsid = prm["pid"], prm["pmt_pid"], prm["program_number"], prm["transport_stream_id"]
    pat = bytes([0x00, 0xB0, 0x0D, tsid >> 8, tsid & 0xFF, 0xC1, 0, 0, prog >> 8, prog & 0xFF, 0xE0 | pmt_pid >> 8, pmt_pid & 0xFF])
    pmt = bytes([0x02, 0xB0, 0x18, prog >> 8, prog & 0xFF, 0xC1, 0, 0, 0xE0 | pid >> 8, pid & 0xFF, 0xF0, 0x00,
                 0x24, 0xE0 | pid >> 8, pid & 0xFF, 0xF0, 0x06, 0x05, 0x04]) + b"HEVC"
    return section_packet(0, prm["cc_pat"] + k, pat), section_packet(pmt_pid, prm["cc_pmt"] + k, pmt)


def time_fields(pts, dts):
    """f"""
    return 3 if (dts != NO_TIME and dts != pts) else 2 if pts != NO_TIME else 0


def time5(t, marker):
    return bytes([(marker << 4 | ((t >> 30) & 7) << 1 | 1) & 0xFF, (t >> 22) & 0xFF, (((t >> 15) & 0x7F) << 1 | 1) & 0xFF, (t >> 7) & 0xFF,
                  ((t & 0x7F) << 1 | 1) & 0xFF])


def au_packets(E, f, pcr):
    """N(a); pcr: a PCR is present (the flag is set and f != 0)"""
    H = {0: 9, 2: 14, 3: 19}[f]
    R1 = 184 - (8 if pcr else 2)
    T = H + E
    return 1 if T <= R1 else 1 + -(-(T - R1) // 184)


def au_to_packets(es, pts, dts, irap, prm, cc):
    """the 188-byte packets of one AU; cc: the continuity counter of its first packet"""
    f = time_fields(pts, dts)
    pes = bytes([0, 0, 1, 0xE0, 0, 0, 0x84, f << 6, {0: 0, 2: 5, 3: 10}[f]])
    if f == 2:
        pes += time5(pts, 2)
    if f == 3:
        pes += time5(pts, 3) + time5(dts, 1)
    pcr = bool(prm["flags"] & PCR) and f != 0
    af = bytes([(0x40 if irap else 0) | (0x10 if pcr else 0)])
    if pcr:
        base = ((dts if f == 3 else pts) - prm["pcr_lead"]) & MASK33
        af += bytes([(base >> 25) & 0xFF, (base >> 17) & 0xFF, (base >> 9) & 0xFF, (base >> 1) & 0xFF, (base & 1) << 7 | 0x7E, 0])
    A1 = 1 + len(af)
    R1 = 184 - A1
    data = pes + bytes(es)
    T = len(data)
    pid = prm["pid"]
    out = []

    def header(pusi, afc):
        return bytes([0x47, pusi << 6 | pid >> 8, pid & 0xFF, afc << 4 | ((cc + len(out)) & 15)])
    if T <= R1:
        afl = 183 - T
        out.append(header(1, 3) + bytes([afl]) + af + b"\xFF" * (afl - len(af)) + data)
    else:
        out.append(header(1, 3) + bytes([A1 - 1]) + af + data[:R1])
        at = R1
        while at < T:
            r = min(184, T - at)
            if r == 184:
                out.append(header(0, 1) + data[at:at + 184])
            else:
                afl = 183 - r
                field = bytes([afl]) + (b"\x00" + b"\xFF" * (afl - 1) if afl >= 1 else b"")
                out.append(header(0, 3) + field + data[at:at + r])
            at += r
    assert all(len(p) == 188 for p in out) and len(out) == au_packets(len(es), f, pcr)
    return out


def frame(p188, B):
    return (b"\x00" * 4 if B == 192 else b"") + p188 + (b"\x00" * 16 if B == 204 else b"")


def es_run_heads(prm, cc):
    """the headers of the packets of an AU that are neither its first nor its last (184 ES bytes each, no adaptation field),
    without a loop: packet i of the run has the continuity counter (cc + i) & 15 -> a function (lo, hi) -> (hi - lo, 4 or 8) uint8"""
    B, pid = prm["packet_bytes"], prm["pid"]
    lead = 4 if B == 192 else 0
    fixed = np.frombuffer(bytes(lead) + bytes([0x47, pid >> 8, pid & 0xFF, 0x10]), dtype=np.uint8)

    def heads(lo, hi):
        h = np.tile(fixed, (hi - lo, 1))
        h[:, lead + 3] = 0x10 | ((cc + np.arange(lo, hi, dtype=np.int64)) & 15)
        return h
    return heads


def plan(stream_bytes, au, pts, dts, prm, out_cap=None):
    """mux() without the stream's bytes -> (segments of tests/_segments.py, au_packet uint32 array of n + 1, summary dict).  A PSI
    packet is a literal; an AU is its first and its last packet, each a literal front (from au_to_packets on an ES of zeros
    with the same length modulo 16 full packets, so the same stuffing and the same continuity counters) and a verbatim range,
    and between them one strided run of full packets."""
    n, B, flags = len(au), prm["packet_bytes"], prm["flags"]
    lead, trail = bytes(4 if B == 192 else 0), bytes(16 if B == 204 else 0)
    segs, au_packet = [], []
    total = es_packets = pairs = es_bytes = 0
    prev_end, bad = 0, 0

    def one(k, p188, es_off, es_len):
        """packet k: its front as a literal, its last es_len bytes from the stream"""
        o = k * B
        if es_len == 0:
            segs.append(("lit", o, lead + p188 + trail))
            return
        segs.append(("lit", o, lead + p188[:188 - es_len]))
        segs.append(("copy", o + len(lead) + 188 - es_len, es_off, es_len))
        if trail:
            segs.append(("lit", o + 188, trail))
    for a in range(n):
        b, e, irap = int(au["unit_begin"][a]), int(au["unit_end"][a]), bool(int(au["flags"][a]) & AU_IRAP)
        p = int(pts[a]) if pts is not None else NO_TIME
        d = int(dts[a]) if dts is not None else NO_TIME
        ok = b <= e <= stream_bytes and b >= prev_end
        ok = ok and (p == NO_TIME or p <= MASK33) and (d == NO_TIME or (d <= MASK33 and p != NO_TIME))
        prev_end = e
        if not ok:
            bad = bad or a + 1
            continue
        if not flags & NO_PSI and (a == 0 or (flags & PSI_AT_IRAP and irap)):
            for q in psi(prm, pairs):
                segs.append(("lit", total * B, frame(q, B)))
                total += 1
            pairs += 1
        au_packet.append(total)
        E, f = e - b, time_fields(p, d)
        pcr = bool(flags & PCR) and f != 0
        N = au_packets(E, f, pcr)
        cc = prm["cc_es"] + es_packets
        mine = au_to_packets(bytes(E - 184 * 16 * ((N - 2) // 16) if N > 2 else E), p, d, irap, prm, cc)
        assert (N - len(mine)) % 16 == 0 and len(mine) <= 18
        if N == 1:
            one(total, mine[0], b, E)
        else:
            e1 = 184 - (8 if pcr else 2) - {0: 9, 2: 14, 3: 19}[f]
            r = E - e1 - (N - 2) * 184
            assert 1 <= r <= 184
            one(total, mine[0], b, e1)
            if N > 2:
                segs.append(("run", (total + 1) * B, run_of(N - 2, B, len(lead) + 4, 184, b + e1, es_run_heads(prm, cc + 1), trail)))
            one(total + N - 1, mine[-1], e - r, r)
        total += N
        es_packets += N
        es_bytes += E
    s = dict(nal_count=total, nal_found=n, rbsp_bytes=es_bytes, stream_bytes=total * B, stop_reason=0, error=0, reserved=[0, es_packets, pairs])
    if bad:
        s.update(error=E_ARG, reserved=[bad, None, None], nal_count=None, rbsp_bytes=None, stream_bytes=None)
    elif out_cap is not None and out_cap < total * B:
        s["error"] = E_CAPACITY
    if s["error"]:
        return [], np.zeros(0, np.uint32), s
    return segs, np.array(au_packet + [total], dtype=np.uint32), s


def mux(stream, au, pts, dts, prm, out_cap=None):
    """-> (out uint8 array, au_packet uint32 array of n + 1, summary dict).  stream: bytes-like; au: a table with unit_begin,
    unit_end, flags; pts / dts: None or one value per AU; out_cap None: large enough (and the plan's summary).  plan() and the
    bytes of its segments."""
    data = bytes(stream)
    segs, au_packet, s = plan(len(data), au, pts, dts, prm, out_cap)
    if s["error"]:
        return np.zeros(0, np.uint8), au_packet, s
    return materialise(segs, s["stream_bytes"], data), au_packet, s


def mux_one_packet_aus(stream, au, prm):
    """mux() for a call whose AUs have no times and at most 173 ES bytes (one packet each, no PCR) and whose only PSI pair stands
    in front of AU 0 or nowhere: the same bytes, built with numpy instead of a loop"""
    data = np.frombuffer(bytes(stream), dtype=np.uint8)
    n, B, flags = len(au), prm["packet_bytes"], prm["flags"]
    b, e = au["unit_begin"].astype(np.int64), au["unit_end"].astype(np.int64)
    E = e - b
    irap = (au["flags"] & AU_IRAP) != 0
    assert n > 0 and not flags & PSI_AT_IRAP and (E <= 173).all() and (E >= 0).all() and (b[1:] >= e[:-1]).all() and e[-1] <= len(data)
    t = np.full((n, 188), 0xFF, dtype=np.uint8)
    pid = prm["pid"]
    t[:, 0], t[:, 1], t[:, 2] = 0x47, 0x40 | pid >> 8, pid & 0xFF
    t[:, 3] = 0x30 | ((prm["cc_es"] + np.arange(n)) & 15)
    t[:, 4] = 183 - (9 + E)
    t[:, 5] = np.where(irap, 0x40, 0)
    pes = np.array([0, 0, 1, 0xE0, 0, 0, 0x84, 0, 0], dtype=np.uint8)
    for size in np.unique(E):                                                    # the packet ends in the PES header and the ES bytes
        rows = np.flatnonzero(E == size)
        t[rows, 188 - size - 9:188 - size] = pes
        if size:
            t[rows, 188 - size:] = data[b[rows][:, None] + np.arange(size)[None, :]]
    pair = [] if flags & NO_PSI else [np.frombuffer(p, dtype=np.uint8) for p in psi(prm, 0)]
    rows = np.concatenate([np.stack(pair), t]) if pair else t
    full = np.zeros((len(rows), B), dtype=np.uint8)
    lead = 4 if B == 192 else 0
    full[:, lead:lead + 188] = rows
    au_packet = np.concatenate([np.arange(n) + len(pair), [n + len(pair)]]).astype(np.uint32)
    s = dict(nal_count=len(rows), nal_found=n, rbsp_bytes=int(E.sum()), stream_bytes=len(rows) * B, stop_reason=0, error=0,
             reserved=[0, n, len(pair) // 2])
    return full.reshape(-1), au_packet, s
