"""hbs_rtp_pack restated as one plain loop over the NALs and their packets (include/hevcbitstream_amd.h is the specification),
a receiver that turns packets back into NALs, and a vectorised restatement for batches of single NAL unit packets.  Test
infrastructure: numpy only, no GPU, nothing of the library."""
import numpy as np

from tests._segments import materialise, run_of

NAL_ENTRY = np.dtype([("start", "<u8"), ("end", "<u8"), ("rbsp_off", "<u8"), ("rbsp_len", "<u4"), ("status", "<i4")])
PARAMS = np.dtype([("max_payload", "<i4"), ("payload_type", "<i4"), ("framing", "<i4"), ("flags", "<u4"), ("ssrc", "<u4"),
                   ("seq", "<u4"), ("ts_base", "<u4"), ("ts_step", "<u4")])
PACKET = np.dtype([("payload_off", "<u8"), ("payload_len", "<u8"), ("nal_off", "<u8"), ("nal_len", "<u8"), ("kind", "<i4"),
                   ("nal_type", "<i4"), ("marker", "<u4"), ("payload_type", "<u4"), ("seq", "<u4"), ("timestamp", "<u4"),
                   ("ssrc", "<u4"), ("fu_start", "<u4"), ("fu_end", "<u4"), ("nal_header", "u1", (2,)), ("reserved", "u1", (2,))])
OPEN_END = 1
SINGLE, FU, AP, OTHER = 0, 1, 2, 3
E_ARG, E_CAPACITY = -3, -4
MP_MIN, MP_MAX = 4, 65523
TIME_LIMIT = 1 << 33
M32 = (1 << 32) - 1


def params(max_payload=1188, payload_type=96, framing=0, flags=0, ssrc=0x1234ABCD, seq=0, ts_base=0, ts_step=0):
    return dict(max_payload=max_payload, payload_type=payload_type, framing=framing, flags=flags, ssrc=ssrc, seq=seq, ts_base=ts_base,
                ts_step=ts_step)


def params_record(prm):
    p = np.zeros(1, dtype=PARAMS)
    for k, v in prm.items():
        p[k][0] = v
    return p


def entries(starts, ends):
    """a NAL_ENTRY table with the two fields the call reads; the others hold junk it must not look at"""
    n = len(starts)
    e = np.frombuffer(np.random.default_rng(n).integers(0, 256, size=n * NAL_ENTRY.itemsize, dtype=np.uint8).tobytes(), dtype=NAL_ENTRY).copy()
    e["start"] = np.asarray(starts, dtype=np.uint64)
    e["end"] = np.asarray(ends, dtype=np.uint64)
    return e


def nal_packets(L, mp):
    """the packets of a NAL of L bytes (0: no such NAL, no such max_payload)"""
    if L < 2 or not MP_MIN <= mp <= MP_MAX:
        return 0
    return 1 if L <= mp else -(-(L - 2) // (mp - 3))


def header(prm, marker, j, ts):
    seq = (prm["seq"] + j) & 0xFFFF
    return bytes([0x80, (0x80 if marker else 0) | prm["payload_type"], seq >> 8, seq & 0xFF]) + (ts & M32).to_bytes(4, "big") + \
        (prm["ssrc"] & M32).to_bytes(4, "big")


def nal_to_packets(nal, prm, marker, j, ts):
    """the RTP packets (no length fields) of one NAL (bytes) whose first packet is the call's j-th"""
    mp, L = prm["max_payload"], len(nal)
    if L <= mp:
        return [header(prm, marker, j, ts) + nal]
    F, body, t = mp - 3, nal[2:], (nal[0] >> 1) & 63
    n = -(-len(body) // F)
    out = []
    for i in range(n):
        fu = bytes([(nal[0] & 0x81) | 0x62, nal[1], (0x80 if i == 0 else 0) | (0x40 if i == n - 1 else 0) | t])
        out.append(header(prm, marker and i == n - 1, j + i, ts) + fu + body[i * F:(i + 1) * F])
    return out


def offending(stream, index, nal_au, n_aus, pts, k):
    """is NAL k malformed?  -> (bad, its AU number relative to the first NAL's)"""
    s = int(index["start"][k])
    return offending_of(len(stream), int(stream[s]) if s < len(stream) else 0, index, nal_au, n_aus, pts, k)


def offending_of(stream_bytes, first_byte, index, nal_au, n_aus, pts, k):
    """offending() from the stream's size and the NAL's first byte"""
    s, e = int(index["start"][k]), int(index["end"][k])
    prev_end = int(index["end"][k - 1]) if k else 0
    bad = s > e or e > stream_bytes or s < prev_end
    if not bad:
        bad = e - s < 2 or ((first_byte >> 1) & 63) >= 48
    a = 0
    if nal_au is not None:
        au = int(nal_au[k])
        a = au - int(nal_au[0])
        if (k and au - int(nal_au[k - 1]) not in (0, 1)) or not 0 <= a < n_aus:
            return True, 0
    if pts is not None and int(pts[a]) >= TIME_LIMIT:
        bad = True
    return bad, a


def nal_headers(stream, index):
    """the first two bytes of every NAL, (n, 2) uint8: all of the stream's contents that plan() needs (0 where the stream ends)"""
    stream = np.asarray(stream, dtype=np.uint8)
    s = index["start"].astype(np.int64)
    padded = np.concatenate([stream, np.zeros(2, dtype=np.uint8)])
    at = np.clip(s, 0, len(stream))
    return np.stack([padded[at], padded[at + 1]], axis=1) if len(index) else np.zeros((0, 2), dtype=np.uint8)


def fu_run_heads(prm, j, ts, hdr2):
    """the headers of the FU packets of a NAL that are neither its first nor its last, without a loop: packet i of the run is
    the call's (j + i)-th packet -> a function (lo, hi) -> (hi - lo, framing + 15) uint8"""
    fr = prm["framing"]
    fixed = header(prm, False, 0, ts) + bytes([(hdr2[0] & 0x81) | 0x62, hdr2[1], (hdr2[0] >> 1) & 63])
    if fr:
        fixed = (12 + prm["max_payload"]).to_bytes(fr, "big") + fixed

    def heads(lo, hi):
        h = np.tile(np.frombuffer(fixed, dtype=np.uint8), (hi - lo, 1))
        seq = (prm["seq"] + j + np.arange(lo, hi, dtype=np.int64)) & 0xFFFF
        h[:, fr + 2], h[:, fr + 3] = seq >> 8, seq & 0xFF
        return h
    return heads


def plan(stream_bytes, hdr, index, nal_au, n_aus, pts, prm, out_cap=None):
    """pack() without the stream's bytes; hdr: nal_headers() -> (segments of tests/_segments.py, nal_off uint64[n + 1],
    nal_packet uint64[n + 1], summary dict); on an error there are no segments and the tables are None.  A NAL of one packet is
    a literal header and a verbatim range; a fragmented NAL is its first and its last packet in that form (their headers from
    nal_to_packets on a NAL of two or three fragments with the same header bytes, the same last fragment and the same packet numbers)
    and, between them, one strided run of full packets."""
    n, mp, fr = len(index), prm["max_payload"], prm["framing"]
    summary = dict(nal_count=0, nal_found=n, rbsp_bytes=0, stream_bytes=0, stop_reason=0, error=0, reserved=[0, 0, 0])
    rel = []
    for k in range(n):
        bad, a = offending_of(stream_bytes, int(hdr[k][0]), index, nal_au, n_aus, pts, k)
        if bad:
            summary["error"], summary["reserved"] = E_ARG, [k + 1, 0, 0]
            return [], None, None, summary
        rel.append(a)
    segs, nal_off, nal_packet, at, j, carried, fus = [], [], [], 0, 0, 0, 0
    F, P = mp - 3, fr + 12 + mp

    def framed(p, head):
        return (len(p).to_bytes(fr, "big") if fr else b"") + p[:head]
    for k in range(n):
        S, L = int(index["start"][k]), int(index["end"][k]) - int(index["start"][k])
        h2 = bytes([int(hdr[k][0]), int(hdr[k][1])])
        if k == n - 1:
            marker = not prm["flags"] & OPEN_END
        else:
            marker = nal_au is not None and int(nal_au[k + 1]) != int(nal_au[k])
        ts = prm["ts_base"] + (int(pts[rel[k]]) if pts is not None else rel[k] * prm["ts_step"])
        nal_off.append(at)
        nal_packet.append(j)
        count = nal_packets(L, mp)
        if count == 1:
            (p,) = nal_to_packets(h2 + bytes(L - 2), prm, marker, j, ts)
            segs += [("lit", at, framed(p, 12)), ("copy", at + fr + 12, S, L)]
            at += fr + 12 + L
        else:
            last = L - 2 - (count - 1) * F
            assert 1 <= last <= F
            mid = min(count, 3) - 2                            # (a body of F + 1 bytes is one packet: three fragments where the NAL has three or more)
            packets = nal_to_packets(h2 + bytes((1 + mid) * F + last), prm, marker, j, ts)
            first_p = packets[0]
            last_p = nal_to_packets(h2 + bytes((1 + mid) * F + last), prm, marker, j + count - 2 - mid, ts)[-1]
            assert len(packets) == 2 + mid
            assert len(first_p) == 12 + mp and len(last_p) == 15 + last
            segs += [("lit", at, framed(first_p, 15)), ("copy", at + fr + 15, S + 2, F)]
            if count > 2:
                segs.append(("run", at + P, run_of(count - 2, P, fr + 15, F, S + 2 + F, fu_run_heads(prm, j + 1, ts, h2))))
            o = at + (count - 1) * P
            segs += [("lit", o, framed(last_p, 15)), ("copy", o + fr + 15, S + 2 + (count - 1) * F, last)]
            at = o + fr + 15 + last
        j += count
        carried += L
        fus += L > mp
    summary.update(nal_count=j, rbsp_bytes=carried, stream_bytes=at, reserved=[0, j, fus])
    tabs = np.array(nal_off + [at], dtype=np.uint64), np.array(nal_packet + [j], dtype=np.uint64)
    if out_cap is not None and at > out_cap:
        summary["error"] = E_CAPACITY
        return [], None, None, summary
    return segs, tabs[0], tabs[1], summary


def pack(stream, index, nal_au, n_aus, pts, prm, out_cap=None):
    """-> (out uint8 array, nal_off uint64[n + 1], nal_packet uint64[n + 1], summary dict); on an error out is empty and the
    tables are None.  plan() and the bytes of its segments."""
    segs, nal_off, nal_packet, summary = plan(len(stream), nal_headers(stream, index), index, nal_au, n_aus, pts, prm, out_cap)
    if summary["error"]:
        return np.zeros(0, dtype=np.uint8), None, None, summary
    return materialise(segs, summary["stream_bytes"], stream), nal_off, nal_packet, summary


def packet_offsets(nal_off, nal_packet, prm):
    """where every packet begins, and the total: all packets of a NAL but its last take framing + 12 + max_payload bytes
    (np.repeat arithmetic; tests/test_big_checks.py holds it against the loop over the NALs and their packets)"""
    nal_off, nal_packet = np.asarray(nal_off, dtype=np.uint64), np.asarray(nal_packet, dtype=np.uint64)
    count = np.diff(nal_packet).astype(np.int64)
    within = np.arange(int(nal_packet[-1]), dtype=np.uint64) - np.repeat(nal_packet[:-1], count)
    off = np.repeat(nal_off[:-1], count) + within * np.uint64(prm["framing"] + 12 + prm["max_payload"])
    return np.concatenate([off, nal_off[-1:]]).astype(np.uint64)


def read_packet(pkt):
    """one RTP packet as a receiver reads it (RFC 3550 5.1, 5.3.1; RFC 7798 4.4) -> a dict with the fields of hbs_rtp_packet, or
    None where hbs_rtp_packet_host refuses"""
    n = len(pkt)
    if n < 12 or pkt[0] >> 6 != 2:
        return None
    head = 12 + 4 * (pkt[0] & 15)
    if head > n:
        return None
    if pkt[0] & 0x10:
        if n - head < 4:
            return None
        words = pkt[head + 2] << 8 | pkt[head + 3]
        head += 4
        if n - head < 4 * words:
            return None
        head += 4 * words
    pad = 0
    if pkt[0] & 0x20:
        pad = pkt[n - 1]
        if pad == 0 or pad > n - head:
            return None
    r = dict(payload_off=head, payload_len=n - head - pad, marker=pkt[1] >> 7, payload_type=pkt[1] & 127, seq=pkt[2] << 8 | pkt[3],
             timestamp=int.from_bytes(pkt[4:8], "big"), ssrc=int.from_bytes(pkt[8:12], "big"), kind=OTHER, nal_type=-1, fu_start=0, fu_end=0,
             nal_off=head, nal_len=n - head - pad, nal_header=[0, 0])
    if r["payload_len"] >= 2:
        p = pkt[head:]
        t = (p[0] >> 1) & 63
        r.update(nal_type=t, nal_header=[p[0], p[1]])
        if t < 48:
            r["kind"] = SINGLE
        elif t == 48:
            r["kind"] = AP
        elif t == 49:
            if r["payload_len"] < 3:
                return None
            r.update(kind=FU, fu_start=p[2] >> 7, fu_end=(p[2] >> 6) & 1, nal_type=p[2] & 63, nal_header=[(p[0] & 0x81) | (p[2] & 63) << 1, p[1]],
                     nal_off=head + 3, nal_len=r["payload_len"] - 3)
    return r


def unpack(out, offsets, prm):
    """the receiver: the packets of `out` that begin at offsets[:-1] -> (NAL byte strings, the AU of each NAL counted from the
    marker bits, the timestamp of each NAL, the packets as read_packet dicts).  Sequence numbers must count up from prm's, the
    fragments of a NAL must be consecutive, begin with S, end with E and share a timestamp."""
    out = bytes(np.asarray(out, dtype=np.uint8).tobytes())
    fr = prm["framing"]
    nals, aus, times, packets = [], [], [], []
    au, cur, cur_ts = 0, None, None
    for j in range(len(offsets) - 1):
        lo, hi = int(offsets[j]), int(offsets[j + 1])
        if fr:
            assert int.from_bytes(out[lo:lo + fr], "big") == hi - lo - fr, j
        pkt = out[lo + fr:hi]
        r = read_packet(pkt)
        assert r is not None and r["seq"] == (prm["seq"] + j) & 0xFFFF and r["payload_type"] == prm["payload_type"], (j, r)
        assert r["ssrc"] == prm["ssrc"] and r["payload_len"] <= prm["max_payload"], (j, r)
        packets.append(r)
        data = pkt[r["nal_off"]:r["nal_off"] + r["nal_len"]]
        if r["kind"] == SINGLE:
            assert cur is None, j
            nals.append(data)
            aus.append(au)
            times.append(r["timestamp"])
        else:
            assert r["kind"] == FU and not (r["fu_start"] and r["fu_end"]) and len(data) > 0, (j, r)
            if r["fu_start"]:
                assert cur is None, j
                cur, cur_ts = bytes(r["nal_header"]), r["timestamp"]
            assert cur is not None and r["timestamp"] == cur_ts, j
            cur += data
            if r["fu_end"]:
                nals.append(cur)
                aus.append(au)
                times.append(cur_ts)
                cur = None
            else:
                assert not r["marker"] and len(pkt) - 12 == prm["max_payload"], j
        if r["marker"]:
            assert cur is None, j
            au += 1
    assert cur is None
    return nals, aus, times, packets


def random_case(rng, n, max_nal=900, gaps=True, aus=True, times=True, min_nal=2):
    """n NALs of random sizes, types below 48, gaps, AU numbers that begin at a random number and times -> (stream, index, nal_au,
    n_aus, pts)"""
    sizes = rng.integers(min_nal, max_nal, size=n)
    gap = rng.integers(0, 20, size=n) * (rng.random(n) < 0.5) if gaps else np.zeros(n, dtype=np.int64)
    starts = np.cumsum(gap + np.concatenate([[0], sizes[:-1]])) if n else np.zeros(0, dtype=np.int64)
    ends = starts + sizes
    stream = rng.integers(0, 256, size=int(ends[-1]) if n else 0, dtype=np.uint8)
    if n:
        stream[starts] = (rng.integers(0, 48, size=n) << 1 | rng.integers(0, 2, size=n) | rng.integers(0, 2, size=n) << 7).astype(np.uint8)
    if not aus:
        return stream, entries(starts, ends), None, 0, (rng.integers(0, TIME_LIMIT, size=1, dtype=np.uint64) if times else None)
    rel = np.cumsum(rng.random(n) < 0.3).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    if n:
        rel -= rel[0]
    n_aus = int(rel[-1]) + 1 if n else 0
    nal_au = (rel + int(rng.integers(0, 1000))).astype(np.uint32)
    pts = rng.integers(0, TIME_LIMIT, size=n_aus, dtype=np.uint64) if times else None
    return stream, entries(starts, ends), nal_au, n_aus, pts


def pack_single_packets(stream, index, nal_au, n_aus, pts, prm):
    """pack() for a well-formed batch in which every NAL is one packet, without a loop over the NALs"""
    n, mp, fr = len(index), prm["max_payload"], prm["framing"]
    start, L = index["start"].astype(np.int64), (index["end"] - index["start"]).astype(np.int64)
    assert n and (L >= 2).all() and (L <= mp).all()
    head = fr + 12
    off = np.concatenate([[0], np.cumsum(L + head)])
    rel = (nal_au.astype(np.int64) - int(nal_au[0])) if nal_au is not None else np.zeros(n, dtype=np.int64)
    ts = (prm["ts_base"] + (pts[rel].astype(np.int64) if pts is not None else rel * prm["ts_step"])) & M32
    marker = np.zeros(n, dtype=bool)
    if nal_au is not None:
        marker[:-1] = nal_au[1:] != nal_au[:-1]
    marker[-1] = not prm["flags"] & OPEN_END
    seq = (prm["seq"] + np.arange(n)) & 0xFFFF
    H = np.zeros((n, head), dtype=np.uint8)
    if fr:
        H[:, 0], H[:, 1] = (L + 12) >> 8, (L + 12) & 0xFF
    H[:, fr] = 0x80
    H[:, fr + 1] = marker * 0x80 | prm["payload_type"]
    H[:, fr + 2], H[:, fr + 3] = seq >> 8, seq & 0xFF
    for b in range(4):
        H[:, fr + 4 + b] = (ts >> (8 * (3 - b))) & 0xFF
        H[:, fr + 8 + b] = (prm["ssrc"] >> (8 * (3 - b))) & 0xFF
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    out[(off[:-1, None] + np.arange(head)[None, :]).reshape(-1)] = H.reshape(-1)
    before = np.concatenate([[0], np.cumsum(L)[:-1]])
    run = np.arange(int(L.sum()))
    out[np.repeat(off[:-1] + head - before, L) + run] = stream[np.repeat(start - before, L) + run]
    summary = dict(nal_count=n, nal_found=n, rbsp_bytes=int(L.sum()), stream_bytes=int(off[-1]), stop_reason=0, error=0, reserved=[0, n, 0])
    return out, off.astype(np.uint64), np.arange(n + 1, dtype=np.uint64), summary
