"""hbs_ts_demux restated as one plain loop over the packets (include/hevcbitstream_amd.h is the specification), and a small
transport-stream muxer for building inputs.  Test infrastructure: numpy only, no GPU, nothing of the library."""
import numpy as np

TS_PES = np.dtype([("out_off", "<u8"), ("pts", "<u8"), ("dts", "<u8"), ("packet", "<u4"), ("flags", "<u4")])
FAULT, OTHER, SKIPPED, NO_PAYLOAD, PAYLOAD, PES_START = -1, 0, 1, 2, 3, 4
F_PTS, F_DTS, F_RAI, F_DI, F_ALIGN = 1, 2, 4, 8, 16
NO_TIME = (1 << 64) - 1
E_ARG, E_CAPACITY = -3, -4
SIZES = (188, 192, 204)
NULL_PID = 0x1FFF


def lead(B):
    return 4 if B == 192 else 0


def stamp(x):
    return ((x[0] >> 1) & 7) << 30 | x[1] << 22 | (x[2] >> 1) << 15 | x[3] << 7 | x[4] >> 1


def classify(b, pid):
    """the packet rule for the 188 transport bytes b -> dict(cls, pid, off, len, es_off, es_len, cc, flags, pts, dts)"""
    r = dict(cls=FAULT, pid=0, off=0, len=0, es_off=0, es_len=0, cc=0, flags=0, pts=NO_TIME, dts=NO_TIME)
    if b[0] != 0x47:
        return r
    tei, pusi = b[1] >> 7, (b[1] >> 6) & 1
    r["pid"] = (b[1] & 0x1F) << 8 | b[2]
    if r["pid"] != pid:
        r["cls"] = OTHER
        return r
    tsc, afc, cc = b[3] >> 6, (b[3] >> 4) & 3, b[3] & 15
    if tei or tsc:
        r["cls"] = SKIPPED
        return r
    off, flags = 4, 0
    if afc & 2:
        afl = b[4]
        if afl > 183:
            return r
        off = 5 + afl
        if afl >= 1:
            flags |= (F_DI if b[5] >> 7 else 0) | (F_RAI if (b[5] >> 6) & 1 else 0)
    if (afc & 1) == 0 or off == 188:
        r.update(cls=NO_PAYLOAD, cc=cc, off=off, flags=flags)
        return r
    n = 188 - off
    es_off, es_len, pts, dts = off, n, NO_TIME, NO_TIME
    if pusi:
        q = b[off:188]
        if n < 9 or q[0] != 0 or q[1] != 0 or q[2] != 1 or (q[6] & 0xC0) != 0x80:
            return r
        f, H = q[7] >> 6, 9 + q[8]
        if f == 1 or H > n or (f == 2 and q[8] < 5) or (f == 3 and q[8] < 10):
            return r
        if f >= 2:
            pts = dts = stamp(q[9:14])
            flags |= F_PTS
        if f == 3:
            dts = stamp(q[14:19])
            flags |= F_DTS
        if q[6] & 4:
            flags |= F_ALIGN
        es_off, es_len = off + H, n - H
    r.update(cls=PES_START if pusi else PAYLOAD, off=off, len=n, es_off=es_off, es_len=es_len, cc=cc, flags=flags, pts=pts, dts=dts)
    return r


def demux(ts, B, pid, out_cap=None, pes_cap=None):
    """-> (out uint8 array, pes ndarray[TS_PES], summary dict).  out_cap / pes_cap None: large enough (pes_cap None also
    stands for "no d_pes")."""
    data = bytes(ts)
    assert B in SIZES and len(data) % B == 0
    h, n = lead(B), len(data) // B
    parts, pes = [], []
    out_bytes = of_pid = skipped = breaks = 0
    started, prev_cc, fault = False, None, 0
    for p in range(n):
        o = p * B + h
        if data[o] == 0x47 and ((data[o + 1] & 0x1F) << 8 | data[o + 2]) != pid:
            continue
        r = classify(data[o:o + 188], pid)
        if r["cls"] == FAULT:
            fault = p + 1
            break
        of_pid += 1
        if not started and r["cls"] != PES_START:
            skipped += 1
            continue
        started = True
        if r["cls"] == SKIPPED:
            skipped += 1
        if r["cls"] not in (PAYLOAD, PES_START):
            continue
        if prev_cc is not None and r["cc"] != (prev_cc + 1) & 15 and not r["flags"] & F_DI:
            breaks += 1
        prev_cc = r["cc"]
        if r["cls"] == PES_START:
            pes.append((out_bytes, r["pts"], r["dts"], p, r["flags"]))
        parts.append(data[o + r["es_off"]: o + r["es_off"] + r["es_len"]])
        out_bytes += r["es_len"]
    s = dict(nal_count=len(pes), nal_found=of_pid, rbsp_bytes=0, stream_bytes=out_bytes, stop_reason=0, error=0,
             reserved=[0, breaks, skipped])
    if fault:
        s.update(error=E_ARG, reserved=[fault, None, None], nal_count=None, nal_found=None, stream_bytes=None)
    elif (out_cap is not None and out_cap < out_bytes) or (pes_cap is not None and pes_cap < len(pes)):
        s["error"] = E_CAPACITY
    if s["error"]:
        return np.zeros(0, np.uint8), np.zeros(0, TS_PES), s
    return np.frombuffer(b"".join(parts), dtype=np.uint8), np.array(pes, dtype=TS_PES), s


# ---- a small muxer ------------------------------------------------------------------------------------------------------------

def time5(t, marker):
    """the five bytes of a PES time stamp (marker: 2 PTS alone, 3 PTS of a pair, 1 DTS)"""
    return bytes([marker << 4 | ((t >> 30) & 7) << 1 | 1, (t >> 22) & 0xFF, ((t >> 15) & 0x7F) << 1 | 1, (t >> 7) & 0xFF, (t & 0x7F) << 1 | 1])


def pes_header(pts=None, dts=None, stuffing=0, align=False, stream_id=0xE0):
    opt = b""
    if pts is not None and dts is not None:
        opt = time5(pts, 3) + time5(dts, 1)
    elif pts is not None:
        opt = time5(pts, 2)
    opt += b"\xFF" * stuffing
    f = 3 if dts is not None else 2 if pts is not None else 0
    return bytes([0, 0, 1, stream_id, 0, 0, 0x80 | (4 if align else 0), f << 6, len(opt)]) + opt


def packet(pid, payload=b"", pusi=0, cc=0, afl=None, af_flags=0, tei=0, tsc=0, B=188, pcr=False):
    """one packet: the adaptation field (afl None: none; else exactly afl bytes behind the length byte, the first of them
    af_flags, with pcr six more meaningful ones, the rest FF stuffing), then the payload, which must fill the rest"""
    afc = (2 if afl is not None else 0) | (1 if len(payload) else 0)
    body = bytes([0x47, tei << 7 | pusi << 6 | pid >> 8, pid & 0xFF, tsc << 6 | afc << 4 | cc])
    if afl is not None:
        af = bytes([af_flags | (0x10 if pcr else 0)]) + (bytes([1, 2, 3, 4, 0x7E, 5]) if pcr else b"")
        af = af[:afl] + b"\xFF" * (afl - len(af))
        body += bytes([afl]) + af
    body += bytes(payload)
    assert len(body) == 188, len(body)
    return (b"\x11\x22\x33\x44" if B == 192 else b"") + body + (b"\xEE" * 16 if B == 204 else b"")


def fit(pid, data, **kw):
    """a packet that carries all of `data` (<= 184 bytes): an adaptation field of stuffing takes the rest"""
    spare = 184 - len(data)
    assert spare >= 0
    if kw.get("afl") is None and kw.get("af_flags") is None and not kw.get("pcr") and spare == 0:
        return packet(pid, data, **kw)
    kw.pop("afl", None)
    need = 1 + (1 if (kw.get("af_flags") or kw.get("pcr")) else 0) + (6 if kw.get("pcr") else 0)
    assert spare >= need, "no room for the adaptation field"
    return packet(pid, data, afl=spare - 1, **kw)


def section_packet(pid, section, cc=0, pointer=0, B=188):
    pay = bytes([pointer]) + b"\xFF" * pointer + section
    return packet(pid, pay + b"\xFF" * (184 - len(pay)), pusi=1, cc=cc, B=B)


def pat(programs, tsid=1):
    """programs: [(program_number, pid)]"""
    body = bytes([tsid >> 8, tsid & 0xFF, 0xC1, 0, 0]) + b"".join(bytes([n >> 8, n & 0xFF, 0xE0 | p >> 8, p & 0xFF]) for n, p in programs)
    n = len(body) + 4
    return bytes([0, 0xB0 | n >> 8, n & 0xFF]) + body + b"\xDE\xAD\xBE\xEF"


def pmt(program, streams, pcr_pid=0x100, info=b""):
    """streams: [(stream_type, pid, descriptor bytes)]"""
    body = bytes([program >> 8, program & 0xFF, 0xC1, 0, 0, 0xE0 | pcr_pid >> 8, pcr_pid & 0xFF, 0xF0 | len(info) >> 8, len(info) & 0xFF]) + info
    for st, p, d in streams:
        body += bytes([st, 0xE0 | p >> 8, p & 0xFF, 0xF0 | len(d) >> 8, len(d) & 0xFF]) + d
    n = len(body) + 4
    return bytes([2, 0xB0 | n >> 8, n & 0xFF]) + body + b"\xDE\xAD\xBE\xEF"


def mux_units(units, pid, B=188, times=None, rng=None, other_every=7, pmt_pid=0x1000):
    """one PES packet per unit (bytes), PAT and PMT in front, packets of another PID and null packets in between.
    times: [(pts, dts or None)] per unit.  -> (stream bytes, [number of the packet each PES begins in])"""
    rng = rng or np.random.default_rng(1)
    out = [section_packet(0, pat([(0, 0x10), (1, pmt_pid)]), B=B), section_packet(pmt_pid, pmt(1, [(0x0F, 0x101, b""), (0x24, pid, b"\x05\x04HEVC")]), B=B)]
    cc, k, begins = 0, 0, []
    for u, unit in enumerate(units):
        pts, dts = times[u] if times else (None, None)
        data = pes_header(pts, dts, stuffing=int(rng.integers(0, 4)), align=True) + bytes(unit)
        at, first = 0, True
        while at < len(data):
            take = min(184, len(data) - at)
            if first and take == 184 and rng.integers(3) == 0:
                take = 184 - 8                          # room for an adaptation field with a PCR-sized field in the PES's first packet
            kw = dict(pusi=1 if first else 0, cc=cc, B=B)
            if first:
                begins.append(len(out))
                if take <= 176:
                    kw.update(af_flags=0x40 if u % 5 == 0 else 0, pcr=True)
            out.append(fit(pid, data[at:at + take], **kw))
            at, first, cc, k = at + take, False, (cc + 1) & 15, k + 1
            if k % other_every == 0:
                out.append(packet(0x101, rng.integers(0, 256, 184, dtype=np.uint8).tobytes(), cc=k & 15, B=B))
            if k % 31 == 0:
                out.append(packet(NULL_PID, b"\xFF" * 184, B=B))
    return b"".join(out), begins


def random_ts(rng, n, B, pid, share=1.0, first_pes=0, p_pes=0.06, p_skip=0.02, p_nopay=0.03, p_empty=0.15, lens="mixed", p_break=0.0,
              cc_events=()):
    """n random packets as an (n, B) uint8 array, built vectorised.  share: part of the packets on `pid`; first_pes: the packet
    in front of which `pid` carries no PES start (None: none at all), that packet being one when it is on the PID.
    lens: "mixed" payloads of 1..184 bytes, "full" 184.  p_empty: PES starts whose ES part is empty.  p_break: continuity
    breaks at random; cc_events: [(packet, "break" | "dup" | "break_di")] on top."""
    h = lead(B)
    a = rng.integers(0, 256, size=(n, B), dtype=np.uint8)
    if n == 0:
        return a
    t = a[:, h:h + 188]
    on = rng.random(n) < share if share < 1.0 else np.ones(n, bool)
    if first_pes is not None and first_pes < n and share > 0:
        on[first_pes] = True
    ev = np.array([p for p, _ in cc_events], dtype=np.int64)
    on[ev] = True
    pids = np.where(on, pid, rng.choice([0x21, 0x101, NULL_PID, pid ^ 1], size=n))
    kind = rng.random(n)
    pes = on & (kind < p_pes)
    skip = on & ~pes & (kind < p_pes + p_skip)
    nopay = on & ~pes & ~skip & (kind < p_pes + p_skip + p_nopay)
    skip[ev] = False
    nopay[ev] = False
    if first_pes is None:
        pes[:] = False
    else:
        pes[:first_pes] = False
        if first_pes < n and on[first_pes]:
            pes[first_pes], skip[first_pes], nopay[first_pes] = True, False, False
    # payload lengths
    plen = np.full(n, 184) if lens == "full" else rng.integers(1, 185, size=n)
    plen = np.where(rng.random(n) < 0.3, 184, plen)
    hdr_extra = rng.integers(0, 6, size=n)                     # stuffing bytes in a PES header
    fl = rng.choice([0, 2, 3], size=n)
    q8 = np.where(fl == 3, 10, np.where(fl == 2, 5, 0)) + hdr_extra
    empty = pes & (rng.random(n) < p_empty)
    plen = np.where(pes, np.maximum(plen, 9 + q8), plen)
    plen = np.where(empty, 9 + q8, plen)
    plen = np.where(plen == 183, 182, plen)                     # 183 payload bytes need an adaptation field of one byte (afl 0): kept for afl0 below
    afl0 = on & ~pes & (rng.random(n) < 0.05)
    afl0[ev] = False
    plen[ev] = np.minimum(plen[ev], 150)                        # room for an adaptation field with a flags byte
    plen = np.where(afl0, 183, plen)
    has_af = (plen < 184) | nopay
    afl = np.where(nopay, 183, 183 - plen)
    nopay_plain = nopay & (rng.random(n) < 0.3)                 # afc 0 / no adaptation field at all also means "no payload"
    has_af &= ~nopay_plain
    afc = np.where(nopay_plain, 0, np.where(nopay, 2, np.where(has_af, 3, 1)))
    di = on & has_af & (afl >= 1) & (rng.random(n) < 0.03)
    rai = on & has_af & (afl >= 1) & (rng.random(n) < 0.2)
    # continuity counters over the packets with ES bytes
    es = on & ~skip & ~nopay
    step = np.where(es, 1, 0)
    jump = es & (rng.random(n) < p_break)
    step = step + np.where(jump, rng.integers(1, 15, size=n), 0)
    for p, what in cc_events:
        assert es[p] and has_af[p] and afl[p] >= 1
        step[p] = 0 if what == "dup" else 5
        di[p] = what == "break_di"
    cc = (np.cumsum(step) + 7) & 15
    cc = np.where(es, cc, rng.integers(0, 16, size=n))
    tei = skip & (rng.random(n) < 0.5)
    tsc = np.where(skip & ~tei, rng.integers(1, 4, size=n), 0)
    t[:, 0] = 0x47
    t[:, 1] = (tei.astype(int) << 7) | (pes.astype(int) << 6) | (pids >> 8)
    t[:, 2] = pids & 0xFF
    t[:, 3] = (tsc << 6) | (afc << 4) | cc
    rows = np.flatnonzero(on & has_af & ~skip)
    t[rows, 4] = afl[rows]
    rows = np.flatnonzero(on & has_af & ~skip & (afl >= 1))
    t[rows, 5] = (di[rows].astype(int) << 7) | (rai[rows].astype(int) << 6) | (t[rows, 5] & 0x0F)
    rows = np.flatnonzero(pes)
    off = 188 - plen[rows]
    ptsv = rng.integers(0, 1 << 33, size=len(rows))
    dtsv = rng.integers(0, 1 << 33, size=len(rows))
    head = np.zeros((len(rows), 19), dtype=np.int64)
    head[:, 2] = 1
    head[:, 3] = 0xE0
    head[:, 6] = 0x80 | (rng.integers(0, 2, size=len(rows)) << 2) | rng.integers(0, 4, size=len(rows))
    head[:, 7] = (fl[rows] << 6) | rng.integers(0, 64, size=len(rows))
    head[:, 8] = q8[rows]
    for base, tv in ((9, ptsv), (14, dtsv)):
        head[:, base] = ((tv >> 30) & 7) << 1 | (rng.integers(0, 2, size=len(rows))) | 0x20
        head[:, base + 1] = (tv >> 22) & 0xFF
        head[:, base + 2] = ((tv >> 15) & 0x7F) << 1 | 1
        head[:, base + 3] = (tv >> 7) & 0xFF
        head[:, base + 4] = (tv & 0x7F) << 1 | 1
    for k in range(19):
        w = np.flatnonzero((k < 9) | (k < 9 + q8[rows]))
        t[rows[w], off[w] + k] = head[w, k]
    return a
