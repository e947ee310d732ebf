"""hbs_rtp_pack with HBS_RTP_AGGREGATE restated as one plain loop (include/hevcbitstream_amd.h is the specification): the greedy
group rule walked one NAL at a time, a group of two or more NALs written as one aggregation packet, everything else left to the
single NAL unit packets and fragmentation units of tests/_rtp_ref.py.  Test infrastructure: numpy only, no GPU, nothing of the
library."""
import numpy as np

from tests import _rtp_ref as R

AGGREGATE = 4
AP_SPAN = 256


def groups(sizes, rel, mp):
    """the group rule: sizes[k] = L_k, rel[k] = a_k -> the list of (first NAL, one behind the last NAL).  A group grows one NAL at
    a time until the next NAL is the call's end, a multiple of AP_SPAN, of another access unit, or would make the payload
    2 + sum (2 + L) exceed mp"""
    out, i, n = [], 0, len(sizes)
    while i < n:
        j, payload = i + 1, 2 + 2 + sizes[i]
        while j < n and j % AP_SPAN != 0 and rel[j] == rel[i] and payload + 2 + sizes[j] <= mp:
            payload += 2 + sizes[j]
            j += 1
        out.append((i, j))
        i = j
    return out


def payload_hdr(headers):
    """the PayloadHdr of an AP over its units' (h0, h1): F the OR, layer id and TID the lowest"""
    f = max(h0 >> 7 for h0, _ in headers)
    layer = min((h0 & 1) << 5 | h1 >> 3 for h0, h1 in headers)
    tid = min(h1 & 7 for _, h1 in headers)
    return bytes([f << 7 | 48 << 1 | layer >> 5, (layer & 31) << 3 | tid])


def pack(stream, index, nal_au, n_aus, pts, prm, out_cap=None):
    """-> (out uint8 array, nal_off uint64[n + 1], nal_packet uint64[n + 1], summary dict); on an error out is empty and the
    tables are None.  Without AGGREGATE in prm["flags"] it is R.pack."""
    if not prm["flags"] & AGGREGATE:
        return R.pack(stream, index, nal_au, n_aus, pts, prm, out_cap)
    stream = np.asarray(stream, dtype=np.uint8)
    n, mp, fr = len(index), prm["max_payload"], prm["framing"]
    summary = dict(nal_count=0, nal_found=n, rbsp_bytes=0, stream_bytes=0, stop_reason=0, error=0, reserved=[0, 0, 0])
    rel = []
    for k in range(n):
        bad, a = R.offending(stream, index, nal_au, n_aus, pts, k)
        if bad:
            summary["error"], summary["reserved"] = R.E_ARG, [k + 1, 0, 0]
            return np.zeros(0, dtype=np.uint8), None, None, summary
        rel.append(a)
    start = [int(x) for x in index["start"]]
    sizes = [int(e) - int(s) for s, e in zip(index["start"], index["end"])]
    raw = stream.tobytes()

    def ends_au(k):
        if k == n - 1:
            return not prm["flags"] & R.OPEN_END
        return nal_au is not None and int(nal_au[k + 1]) != int(nal_au[k])
    out, nal_off, nal_packet, j, fus, aps = bytearray(), [0] * n, [0] * n, 0, 0, 0
    for i, e in groups(sizes, rel, mp):
        ts = prm["ts_base"] + (int(pts[rel[i]]) if pts is not None else rel[i] * prm["ts_step"])
        nals = [raw[start[k]:start[k] + sizes[k]] for k in range(i, e)]
        if e - i == 1:
            packets = R.nal_to_packets(nals[0], prm, ends_au(i), j, ts)
            nal_off[i], nal_packet[i] = len(out), j
            fus += len(packets) > 1
        else:
            body = payload_hdr([(nal[0], nal[1]) for nal in nals])
            at = len(out) + fr + 12 + 2                          # where the first unit's size field lies
            for k, nal in zip(range(i, e), nals):
                nal_off[k], nal_packet[k] = at, j
                at += 2 + len(nal)
                body += len(nal).to_bytes(2, "big") + nal
            nal_off[i] = len(out)                                # the first NAL of a packet: the packet's beginning
            assert len(body) <= mp
            packets = [R.header(prm, ends_au(e - 1), j, ts) + body]
            aps += 1
        for p in packets:
            out += (len(p).to_bytes(fr, "big") if fr else b"") + p
        j += len(packets)
    summary.update(nal_count=j, rbsp_bytes=sum(sizes), stream_bytes=len(out), reserved=[0, j, aps << 32 | fus])
    if out_cap is not None and len(out) > out_cap:
        summary["error"] = R.E_CAPACITY
        return np.zeros(0, dtype=np.uint8), None, None, summary
    return (np.frombuffer(bytes(out), dtype=np.uint8), np.array(nal_off + [len(out)], dtype=np.uint64),
            np.array(nal_packet + [j], dtype=np.uint64), summary)


def packet_offsets(nal_off, nal_packet, prm):
    """where every packet begins, and the total, by the loop: NAL k opens a packet when k == 0 or nal_packet[k] differs from
    nal_packet[k - 1]; all packets of a NAL but its last take framing + 12 + max_payload bytes"""
    n = len(nal_off) - 1
    opens = [k for k in range(n) if k == 0 or int(nal_packet[k]) != int(nal_packet[k - 1])]
    off = []
    for k, m in zip(opens, opens[1:] + [n]):
        for p in range(int(nal_packet[m]) - int(nal_packet[k])):
            off.append(int(nal_off[k]) + p * (prm["framing"] + 12 + prm["max_payload"]))
    return np.array(off + [int(nal_off[n])], dtype=np.uint64)


def ap_units(pkt):
    """the units of an aggregation packet (bytes, no length field) -> [(offset, size)], or None where hbs_rtp_ap_units_host refuses"""
    r = R.read_packet(pkt)
    if r is None or r["kind"] != R.AP:
        return None
    p, e, units = r["payload_off"] + 2, r["payload_off"] + r["payload_len"], []
    if p == e:
        return None
    while p < e:
        if e - p < 2:
            return None
        s = pkt[p] << 8 | pkt[p + 1]
        p += 2
        if s < 2 or s > e - p or (pkt[p] >> 1) & 63 >= 48:
            return None
        units.append((p, s))
        p += s
    return units
