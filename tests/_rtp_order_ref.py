"""hbs_rtp_order restated as one plain sequential loop over the packet table (include/hevcbitstream_amd.h is the specification):
one packet after another, a dict of first arrivals, `sorted` -- deliberately not the prefix sums and the slot table of the kernels.
order_plain is a second restatement without a loop (cumsum of sext16 differences, np.minimum.at into slots), which
tests/test_rtp_order_ref.py holds against the loop; and the generators of arrival orders: a shuffle inside a window, duplicates,
losses, packets of other streams.  The header of a packet is read with tests/_rtp_ref.read_packet.  Test infrastructure: numpy
only, no GPU, nothing of the library."""
import numpy as np

from tests import _rtp_ref as R
from tests import _rtp_unpack_ref as U

PARAMS = np.dtype([("payload_type", "<i4"), ("flags", "<u4"), ("ssrc", "<u4"), ("reserved", "<u4"), ("max_span", "<u8"), ("after_ext", "<u8")])
MATCH_SSRC, AFTER = 1, 2
E_ARG, E_CAPACITY = R.E_ARG, R.E_CAPACITY
START = 1 << 48
SSRC = 0x1234ABCD


def params(payload_type=96, flags=0, ssrc=SSRC, reserved=0, max_span=1 << 20, after_ext=0):
    return dict(payload_type=payload_type, flags=flags, ssrc=ssrc, reserved=reserved, max_span=max_span, after_ext=after_ext)


def params_record(prm):
    p = np.zeros(1, dtype=PARAMS)
    for k, v in prm.items():
        p[k][0] = v
    return p


def sext16(x):
    """the low 16 bits of x read as a signed number"""
    x &= 0xFFFF
    return x - 0x10000 if x & 0x8000 else x


def empty_summary():
    return dict(nal_count=0, nal_found=0, rbsp_bytes=0, stream_bytes=0, stop_reason=0, error=0, reserved=[0, 0, 0])


def no_tables(summary):
    return dict(off=np.zeros(0, dtype=np.uint64), size=np.zeros(0, dtype=np.uint64), src=np.zeros(0, dtype=np.uint32),
                ext=np.zeros(0, dtype=np.uint64), summary=summary)


def order(data, pkt_off, pkt_size, prm, out_cap=None):
    """-> dict(off uint64, size uint64, src uint32, ext uint64, summary); on an error the tables are empty.  out_cap None: plan
    only, no capacity but max_span is looked at (the tables are still returned)"""
    data = bytes(np.asarray(data, dtype=np.uint8).tobytes())
    summary = empty_summary()
    after = bool(prm["flags"] & AFTER)
    accepted = late = duplicates = moved = 0
    ext = prev_seq = highest = None
    first = {}                                          # ext -> the table position of its first arrival
    for p in range(len(pkt_off)):
        off, size = int(pkt_off[p]), int(pkt_size[p])
        r = None if off + size >= 1 << 64 or off + size > len(data) else R.read_packet(data[off:off + size])
        if r is None:
            summary.update(error=E_ARG, reserved=[p + 1, 0, 0])
            return no_tables(summary)
        if r["payload_type"] != prm["payload_type"] or (prm["flags"] & MATCH_SSRC and r["ssrc"] != prm["ssrc"] & R.M32):
            continue
        accepted += 1
        seq = r["seq"]
        if ext is None:
            ext = prm["after_ext"] + sext16(seq - prm["after_ext"]) if after else START + seq
        else:
            ext += sext16(seq - prev_seq)
        prev_seq = seq
        if after and ext <= prm["after_ext"]:
            late += 1
            continue
        if ext in first:
            duplicates += 1
        else:
            first[ext] = p
            if highest is not None and highest > ext:
                moved += 1
        highest = ext if highest is None else max(highest, ext)
    kept = sorted(first)
    span = 0
    if kept:
        span = kept[-1] - (prm["after_ext"] + 1 if after else kept[0]) + 1
    summary.update(nal_found=accepted, stream_bytes=span)
    if span > prm["max_span"]:
        summary["error"] = E_CAPACITY
        return no_tables(summary)
    summary.update(nal_count=len(kept), rbsp_bytes=kept[-1] if kept else 0, reserved=[0, span - len(kept), duplicates << 32 | moved])
    assert late == accepted - len(kept) - duplicates
    if out_cap is not None and len(kept) > out_cap:
        summary["error"] = E_CAPACITY
        return no_tables(summary)
    src = np.array([first[e] for e in kept], dtype=np.uint32)
    return dict(off=np.asarray(pkt_off, dtype=np.uint64)[src], size=np.asarray(pkt_size, dtype=np.uint64)[src], src=src,
                ext=np.array(kept, dtype=np.uint64), summary=summary)


def order_plain(seq, accepted, prm, pkt_off=None, pkt_size=None):
    """order() without a loop over the packets, for a table without faults: seq = the sequence number of every entry, accepted =
    which entries are this stream's.  Signed 64-bit arithmetic: every ext is below 2^63"""
    seq, accepted = np.asarray(seq, dtype=np.int64), np.asarray(accepted, dtype=bool)
    after, after_ext = bool(prm["flags"] & AFTER), int(prm["after_ext"])
    summary = empty_summary()
    pos = np.flatnonzero(accepted)
    s = seq[pos]
    summary["nal_found"] = len(pos)
    if len(pos) == 0:
        return no_tables(summary)
    sx = lambda x: ((x & 0xFFFF) ^ 0x8000) - 0x8000          # noqa: E731
    d = np.empty(len(s), dtype=np.int64)
    d[0] = after_ext + sx(int(s[0]) - after_ext) if after else START + int(s[0])
    d[1:] = sx(s[1:] - s[:-1])
    ext = np.cumsum(d)
    live = ext > after_ext if after else np.ones(len(ext), dtype=bool)
    pos, ext = pos[live], ext[live]
    if len(pos) == 0:
        return no_tables(summary)
    base = after_ext + 1 if after else int(ext.min())
    span = int(ext.max()) - base + 1
    summary["stream_bytes"] = span
    if span > prm["max_span"]:
        summary["error"] = E_CAPACITY
        return no_tables(summary)
    slots = np.full(span, 0xFFFFFFFF, dtype=np.int64)
    np.minimum.at(slots, ext - base, pos)
    taken = np.flatnonzero(slots != 0xFFFFFFFF)
    src = slots[taken]
    before = np.concatenate([[0], np.maximum.accumulate(ext)[:-1]])
    owns = slots[ext - base] == pos
    moved = int((owns & (before > ext)).sum())
    kept = len(taken)
    summary.update(nal_count=kept, rbsp_bytes=int(ext.max()), reserved=[0, span - kept, (len(pos) - kept) << 32 | moved])
    out = dict(src=src.astype(np.uint32), ext=(taken + base).astype(np.uint64), summary=summary)
    if pkt_off is not None:
        out.update(off=np.asarray(pkt_off, dtype=np.uint64)[src], size=np.asarray(pkt_size, dtype=np.uint64)[src])
    return out


# ---- generators -----------------------------------------------------------------------------------------------------------

def arrival_order(n, window, rng):
    """the positions 0..n-1 in the order a receiver sees them: a stable sort on position + random(0..window)"""
    if window <= 0 or n == 0:
        return np.arange(n)
    return np.argsort(np.arange(n) + rng.integers(0, window + 1, size=n), kind="stable")


def other_packet(rng, kind):
    """a packet that is not this stream's: another payload type, or (for HBS_RTPO_MATCH_SSRC) another ssrc"""
    nal = U.random_nal(rng, int(rng.integers(2, 20)))
    if kind == "pt":
        return U.packet(nal, int(rng.integers(0, 65536)), 5, pt=97)
    return U.packet(nal, int(rng.integers(0, 65536)), 5, ssrc=0x77)


def arrive(packets, rng, window=8, duplicates=0, lose=(), others=0.0, other_kind="pt"):
    """what a receiver gets of the in-order packet list: without the positions in `lose`, shuffled inside `window`, `duplicates`
    of them a second time somewhere behind their first arrival (at most window + 4 entries behind), and a packet of another
    stream in front of a share `others` of the entries -> (arrived packets, sent: the position in `packets` of each, -1 for a
    packet of another stream)"""
    lose = set(int(x) for x in lose)
    sent = [i for i in range(len(packets)) if i not in lose]
    sent = [sent[i] for i in arrival_order(len(sent), window, rng)]
    for _ in range(duplicates):
        at = int(rng.integers(0, len(sent)))
        sent.insert(min(len(sent), at + 1 + int(rng.integers(0, window + 4))), sent[at])
    out, origin = [], []
    for i in sent:
        if others and rng.random() < others:
            out.append(other_packet(rng, other_kind))
            origin.append(-1)
        out.append(packets[i])
        origin.append(i)
    return out, origin


def seq_packets(seqs, rng=None, pt=96, ssrc=SSRC, size=2):
    """one single NAL unit packet of 12 + size bytes for every sequence number given"""
    return [U.packet(bytes([0x40, 0x01]) + bytes((7 * k + j) & 0xFF for j in range(size - 2)), int(s) & 0xFFFF, 1000 + k, pt=pt, ssrc=ssrc)
            for k, s in enumerate(seqs)]


def header_table(n, seqs, pt=96, ssrc=SSRC):
    """n packets of 14 bytes back to back, without a Python loop -> (buffer, pkt_off, pkt_size): the fixed header with the given
    sequence numbers, timestamp = position, a payload of 40 01"""
    seqs = np.asarray(seqs, dtype=np.int64) & 0xFFFF
    pk = np.zeros((n, 14), dtype=np.uint8)
    pk[:, 0], pk[:, 1] = 0x80, pt
    pk[:, 2], pk[:, 3] = seqs >> 8, seqs & 0xFF
    ts = np.arange(n, dtype=np.int64)
    for b in range(4):
        pk[:, 4 + b] = (ts >> (8 * (3 - b))) & 0xFF
        pk[:, 8 + b] = (ssrc >> (8 * (3 - b))) & 0xFF
    pk[:, 12], pk[:, 13] = 0x40, 0x01
    return pk.reshape(-1), np.arange(n, dtype=np.uint64) * np.uint64(14), np.full(n, 14, dtype=np.uint64)
