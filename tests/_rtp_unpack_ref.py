"""hbs_rtp_unpack restated as one plain loop over the packet table (include/hevcbitstream_amd.h is the specification), with
generators for the packets hbs_rtp_pack never makes: aggregation packets, CSRC entries, a header extension, padding.  The header
of a packet is read with tests/_rtp_ref.read_packet.  Test infrastructure: numpy only, no GPU, nothing of the library."""
import numpy as np

from tests import _rtp_ref as R

PARAMS = np.dtype([("payload_type", "<i4"), ("startcode_bytes", "<i4"), ("flags", "<u4"), ("ssrc", "<u4")])
NAL_ENTRY = R.NAL_ENTRY
MATCH_SSRC = 1
E_ARG, E_CAPACITY = R.E_ARG, R.E_CAPACITY
ST_UNTERMINATED = 4
FAULT, OTHER, UNSUPPORTED, SINGLE, AP, FU = range(6)


def params(payload_type=96, startcode_bytes=4, flags=0, ssrc=0x1234ABCD):
    return dict(payload_type=payload_type, startcode_bytes=startcode_bytes, flags=flags, ssrc=ssrc)


def params_record(prm):
    p = np.zeros(1, dtype=PARAMS)
    for k, v in prm.items():
        p[k][0] = v
    return p


# ---- generators -----------------------------------------------------------------------------------------------------------

def packet(payload, seq, ts, marker=0, pt=96, ssrc=0x1234ABCD, csrc=0, ext=None, pad=0):
    """one RTP packet: csrc entries of 4 bytes, ext = None or the number of 32-bit words of a header extension, pad = 0 or the
    padding bytes (1..255), the last of which counts them"""
    b0 = 0x80 | (0x20 if pad else 0) | (0x10 if ext is not None else 0) | csrc
    head = bytes([b0, (0x80 if marker else 0) | pt, (seq >> 8) & 0xFF, seq & 0xFF]) + (ts & R.M32).to_bytes(4, "big") + (ssrc & R.M32).to_bytes(4, "big")
    head += bytes((7 * i + 1) & 0xFF for i in range(4 * csrc))
    if ext is not None:
        head += bytes([0xBE, 0xDE, ext >> 8, ext & 0xFF]) + bytes((3 * i + 2) & 0xFF for i in range(4 * ext))
    tail = (bytes(pad - 1) + bytes([pad])) if pad else b""
    return head + bytes(payload) + tail


def ap_payload(nals, layer_tid=(0, 1)):
    """the payload of an aggregation packet (type 48, no DONL) that carries the NALs"""
    out = bytes([48 << 1 | layer_tid[0] >> 5, (layer_tid[0] & 31) << 3 | layer_tid[1]])
    for n in nals:
        out += len(n).to_bytes(2, "big") + bytes(n)
    return out


def fu_payloads(nal, frag):
    """the payloads of the fragmentation units of one NAL, `frag` body bytes each (the last may be short)"""
    nal = bytes(nal)
    body, t = nal[2:], (nal[0] >> 1) & 63
    n = max(1, -(-len(body) // frag))
    return [bytes([(nal[0] & 0x81) | 0x62, nal[1], (0x80 if i == 0 else 0) | (0x40 if i == n - 1 else 0) | t]) + body[i * frag:(i + 1) * frag]
            for i in range(n)]


def random_nal(rng, size):
    nal = rng.integers(0, 256, size=size, dtype=np.uint8)
    nal[0] = int(rng.integers(0, 48)) << 1 | int(rng.integers(0, 2)) | int(rng.integers(0, 2)) << 7
    return nal.tobytes()


def random_packets(rng, n_packets, lo=4, hi=60, seq=None, pt=96, ssrc=0x1234ABCD, odd_headers=False, aps=True):
    """n_packets packets of single NALs, whole FU chains and aggregation packets with payloads of lo..hi bytes, consecutive
    sequence numbers, in access units that end by the marker, by the timestamp or by both
    -> (packets, NALs, AU of each NAL, timestamp of each AU)"""
    seq = int(rng.integers(0, 65536)) if seq is None else seq
    packets, nals, aus, times = [], [], [], []
    ts, au, new_au = int(rng.integers(0, 1 << 32)), -1, True

    def hdr():
        if not odd_headers:
            return {}
        return dict(csrc=int(rng.integers(0, 16)), ext=(None, 0, 1, 3)[int(rng.integers(0, 4))], pad=(0, 1, 2, 7)[int(rng.integers(0, 4))])
    while len(packets) < n_packets:
        left = n_packets - len(packets)
        kind = int(rng.integers(0, 3 if aps else 2))
        end_au = rng.random() < 0.3
        if new_au:
            au += 1
            times.append(ts)
        if kind == 0 or left == 1:
            nal = random_nal(rng, int(rng.integers(max(lo, 2), hi + 1)))
            packets.append(packet(nal, seq + len(packets), ts, marker=end_au, pt=pt, ssrc=ssrc, **hdr()))
            nals.append(nal)
            aus.append(au)
        elif kind == 1:
            frag = int(rng.integers(max(lo - 3, 1), hi - 2))
            count = min(left, int(rng.integers(2, 6)))
            nal = random_nal(rng, 2 + frag * (count - 1) + int(rng.integers(1, frag + 1)))
            pays = fu_payloads(nal, frag)
            assert len(pays) == count
            for i, pay in enumerate(pays):
                packets.append(packet(pay, seq + len(packets), ts, marker=end_au and i == count - 1, pt=pt, ssrc=ssrc, **hdr()))
            nals.append(nal)
            aus.append(au)
        else:
            units = [random_nal(rng, int(rng.integers(2, 12))) for _ in range(int(rng.integers(1, 5)))]
            packets.append(packet(ap_payload(units), seq + len(packets), ts, marker=end_au, pt=pt, ssrc=ssrc, **hdr()))
            nals += units
            aus += [au] * len(units)
        step = rng.random()
        new_au = end_au or step < 0.1                      # an AU ends by the marker, by the timestamp, or by both
        if (end_au and step < 0.8) or (not end_au and step < 0.1):
            ts = (ts + int(rng.integers(1, 5000))) & R.M32
    return packets, nals, aus, times


def lay_out(packets, rng=None, align=None, reverse=False, framing=0):
    """the packets in one buffer -> (buffer uint8, pkt_off uint64, pkt_size uint64).  align: the residue modulo 16 of packet p's
    first byte is align(p); reverse: stored back to front (the table stays in packet order); framing 2: a 16-bit length in front
    of each packet, as hbs_rtp_pack writes them"""
    order = range(len(packets) - 1, -1, -1) if reverse else range(len(packets))
    parts, at, off = [], 0, [0] * len(packets)
    for p in order:
        if framing:
            parts.append(len(packets[p]).to_bytes(2, "big"))
            at += 2
        if align is not None:
            gap = (align(p) - at) % 16
            parts.append(bytes(gap))
            at += gap
        elif rng is not None and rng.random() < 0.3:
            gap = int(rng.integers(0, 20))
            parts.append(bytes([0xEE]) * gap)
            at += gap
        off[p] = at
        parts.append(packets[p])
        at += len(packets[p])
    return (np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(off, dtype=np.uint64),
            np.array([len(p) for p in packets], dtype=np.uint64))


# ---- the receiver ---------------------------------------------------------------------------------------------------------

def classify(pkt, prm):
    """steps 2 to 4 of the packet rule for one packet (bytes) -> (class, read_packet's dict or None, the NALs of an aggregation
    packet)"""
    r = R.read_packet(pkt)
    if r is None:
        return FAULT, None, None
    if r["payload_type"] != prm["payload_type"] or (prm["flags"] & MATCH_SSRC and r["ssrc"] != prm["ssrc"] & R.M32):
        return OTHER, r, None
    if r["kind"] == R.SINGLE:
        return SINGLE, r, None
    if r["kind"] == R.FU:
        return (FAULT if r["nal_type"] >= 48 else FU), r, None
    if r["kind"] == R.AP:
        pay = pkt[r["payload_off"]:r["payload_off"] + r["payload_len"]]
        at, units = 2, []
        if at == len(pay):
            return FAULT, r, None
        while at < len(pay):
            if len(pay) - at < 2:
                return FAULT, r, None
            s = pay[at] << 8 | pay[at + 1]
            at += 2
            if s < 2 or s > len(pay) - at or (pay[at] >> 1) & 63 >= 48:
                return FAULT, r, None
            units.append(bytes(pay[at:at + s]))
            at += s
        return AP, r, units
    return UNSUPPORTED, r, None


def continues(cur, prev):
    """cur, prev: (class, dict, raw PayloadHdr bytes)"""
    (cc, c, ch), (pc, p, ph) = cur, prev
    return (cc == FU and not c["fu_start"] and pc == FU and not p["fu_end"] and c["nal_type"] == p["nal_type"] and ch == ph and
            c["timestamp"] == p["timestamp"] and c["ssrc"] == p["ssrc"] and c["seq"] == (p["seq"] + 1) & 0xFFFF)


def unpack(data, pkt_off, pkt_size, prm, out_cap=None, nal_cap=None, au_cap=None):
    """-> dict(out uint8 array, index ndarray[NAL_ENTRY], nal_au uint32, au_ts uint64, summary, nals list of bytes); on an error
    the outputs are empty.  out_cap None: plan only, no capacity is looked at"""
    data = bytes(np.asarray(data, dtype=np.uint8).tobytes())
    n, sc = len(pkt_off), prm["startcode_bytes"]
    summary = dict(nal_count=0, nal_found=0, rbsp_bytes=0, stream_bytes=0, stop_reason=0, error=0, reserved=[0, 0, 0])
    empty = dict(out=np.zeros(0, dtype=np.uint8), index=np.zeros(0, dtype=NAL_ENTRY), nal_au=np.zeros(0, dtype=np.uint32),
                 au_ts=np.zeros(0, dtype=np.uint64), summary=summary, nals=[])
    seen = []
    for p in range(n):
        off, size = int(pkt_off[p]), int(pkt_size[p])
        if off + size >= 1 << 64 or off + size > len(data):
            cls, r, units, pkt = FAULT, None, None, b""
        else:
            pkt = data[off:off + size]
            cls, r, units = classify(pkt, prm)
        if cls == FAULT:
            summary.update(error=E_ARG, reserved=[p + 1, 0, 0])
            return empty
        seen.append((cls, r, units, pkt))
    start_code = bytes(sc - 1) + b"\x01"
    nals, accepted, dropped, breaks = [], 0, 0, 0             # nals: (bytes, timestamp, marker)
    chain = None                                              # the open chain: [has S, header + fragments, timestamp, packets]
    prev = None

    def close_chain(last):
        nonlocal chain, dropped
        if chain is None:
            return
        if chain[0] and last[1]["fu_end"]:
            nals.append((chain[1], chain[2], last[1]["marker"]))
        else:
            dropped += chain[3]
        chain = None
    for p in range(n):
        cls, r, units, pkt = seen[p]
        hdr = pkt[r["payload_off"]:r["payload_off"] + 2]
        cur = (cls, r, hdr)
        if cls >= UNSUPPORTED:
            accepted += 1
            if prev is not None and prev[0] >= UNSUPPORTED and r["seq"] != (prev[1]["seq"] + 1) & 0xFFFF:
                breaks += 1
        if chain is not None and not (prev is not None and continues(cur, prev)):
            close_chain(prev)
        if cls == UNSUPPORTED:
            dropped += 1
        elif cls == SINGLE:
            nals.append((pkt[r["nal_off"]:r["nal_off"] + r["nal_len"]], r["timestamp"], r["marker"]))
        elif cls == AP:
            for i, u in enumerate(units):
                nals.append((u, r["timestamp"], r["marker"] if i == len(units) - 1 else 0))
        elif cls == FU:
            frag = pkt[r["nal_off"]:r["nal_off"] + r["nal_len"]]
            if chain is None:
                chain = [r["fu_start"], bytes(r["nal_header"]) + frag, r["timestamp"], 1]
            else:
                chain[1] += frag
                chain[3] += 1
        prev = cur
    close_chain(prev)
    parts, index, nal_au, au_ts, at, au = [], np.zeros(len(nals), dtype=NAL_ENTRY), [], [], 0, -1
    for k, (nal, ts, marker) in enumerate(nals):
        if k == 0 or ts != nals[k - 1][1] or nals[k - 1][2]:
            au += 1
            au_ts.append(ts)
        nal_au.append(au)
        parts.append(start_code + nal)
        index[k] = (at + sc, at + sc + len(nal), 0, 0, ST_UNTERMINATED if k == len(nals) - 1 else 0)
        at += sc + len(nal)
    summary.update(nal_count=len(nals), nal_found=accepted, rbsp_bytes=at - sc * len(nals), stream_bytes=at, stop_reason=-1 if nals else 0,
                   reserved=[0, len(au_ts), breaks << 32 | dropped])
    if out_cap is not None and (at > out_cap or (nal_cap is not None and len(nals) > nal_cap) or (au_cap is not None and len(au_ts) > au_cap)):
        summary["error"] = E_CAPACITY
        return empty
    return dict(out=np.frombuffer(b"".join(parts), dtype=np.uint8), index=index, nal_au=np.array(nal_au, dtype=np.uint32),
                au_ts=np.array(au_ts, dtype=np.uint64), summary=summary, nals=[x[0] for x in nals])


def frames(data):
    """an RFC 4571 byte stream -> (packet offsets, packet sizes, bytes consumed): stops in front of the first incomplete frame"""
    data, at, off, size = bytes(data), 0, [], []
    while len(data) - at >= 2:
        n = data[at] << 8 | data[at + 1]
        if n > len(data) - at - 2:
            break
        off.append(at + 2)
        size.append(n)
        at += 2 + n
    return np.array(off, dtype=np.uint64), np.array(size, dtype=np.uint64), at


def unpack_plain(data, pkt_off, pkt_size, prm):
    """unpack() without a loop over the packets, for a table in which every packet has the fixed 12-byte header, the right payload
    type, and is a single NAL unit or an FU of a whole chain in order (tests/test_rtp_unpack_ref.py holds it against the loop)"""
    data = np.asarray(data, dtype=np.uint8)
    off, size = np.asarray(pkt_off).astype(np.int64), np.asarray(pkt_size).astype(np.int64)
    n, sc = len(off), prm["startcode_bytes"]
    assert n and (data[off] == 0x80).all() and ((data[off + 1] & 127) == prm["payload_type"]).all() and (size >= 14).all()
    t = (data[off + 12] >> 1) & 63
    fu = t == 49
    assert ((t < 48) | fu).all() and (size[fu] >= 15).all()
    fh = np.where(fu, data[np.minimum(off + 14, len(data) - 1)], 0)
    S, E = fu & (fh >> 7 == 1), fu & ((fh >> 6) & 1 == 1)
    first, last = ~fu | S, ~fu | E                            # the packet begins / ends a NAL
    assert first[0] and last[-1] and (first[1:] == last[:-1]).all()
    lit = np.where(first, np.where(fu, sc + 2, sc), 0)
    skip = np.where(fu, 15, 12)
    pay = size - skip
    out_len = lit + pay
    o = np.concatenate([[0], np.cumsum(out_len)])
    out = np.zeros(int(o[-1]), dtype=np.uint8)
    out[o[:-1][first] + sc - 1] = 1
    f = np.flatnonzero(S)
    out[o[f] + sc] = (data[off[f] + 12] & 0x81) | ((fh[f] & 63) << 1)
    out[o[f] + sc + 1] = data[off[f] + 13]
    before = np.concatenate([[0], np.cumsum(pay)[:-1]])
    run = np.arange(int(pay.sum()))
    out[np.repeat(o[:-1] + lit - before, pay) + run] = data[np.repeat(off + skip - before, pay) + run]
    be32 = lambda at: (data[off + at].astype(np.int64) << 24 | data[off + at + 1].astype(np.int64) << 16 |          # noqa: E731
                       data[off + at + 2].astype(np.int64) << 8 | data[off + at + 3])
    seq = data[off + 2].astype(np.int64) << 8 | data[off + 3]
    ts, marker = be32(4)[first], (data[off + 1] >> 7)[last]
    nals = int(first.sum())
    starts = np.ones(nals, dtype=bool)
    starts[1:] = (ts[1:] != ts[:-1]) | (marker[:-1] == 1)
    index = np.zeros(nals, dtype=NAL_ENTRY)
    index["start"], index["end"] = o[:-1][first] + sc, o[1:][last]
    index["status"][-1] = ST_UNTERMINATED
    breaks = int((seq[1:] != (seq[:-1] + 1) & 0xFFFF).sum())
    summary = dict(nal_count=nals, nal_found=n, rbsp_bytes=int(o[-1]) - sc * nals, stream_bytes=int(o[-1]), stop_reason=-1, error=0,
                   reserved=[0, int(starts.sum()), breaks << 32])
    return dict(out=out, index=index, nal_au=(np.cumsum(starts) - 1).astype(np.uint32), au_ts=ts[starts].astype(np.uint64), summary=summary)
