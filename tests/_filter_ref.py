"""Pure-numpy reference of hbs_filter_annexb (include/hevcbitstream_amd.h): which NAL units a rule keeps, the output bytes,
the output index and the summary.  Test infrastructure only."""
import numpy as np

NAL_ENTRY = np.dtype([("start", "<u8"), ("end", "<u8"), ("rbsp_off", "<u8"),
                      ("rbsp_len", "<u4"), ("status", "<i4")])
ST_UNTERMINATED = 4
E_ARG, E_CAPACITY = -3, -4
ALL_TYPES = (1 << 64) - 1


def header_fields(stream, idx):
    """(nal_unit_type, nuh_layer_id, nuh_temporal_id_plus1, has_header) per entry, from the two raw header bytes"""
    s = np.asarray(stream, dtype=np.uint8)
    st = idx["start"].astype(np.int64)
    has = (idx["end"].astype(np.int64) - st) >= 2
    b0 = np.zeros(len(idx), dtype=np.int64)
    b1 = np.zeros(len(idx), dtype=np.int64)
    b0[has] = s[st[has]]
    b1[has] = s[st[has] + 1]
    return (b0 >> 1) & 63, ((b0 & 1) << 5) | (b1 >> 3), b1 & 7, has


def rule_keep(stream, idx, keep_types=ALL_TYPES, max_temporal_id_plus1=7, max_layer_id=63, keep_short=True):
    t, layer, tid1, has = header_fields(stream, idx)
    bit = np.array([(int(keep_types) >> int(x)) & 1 for x in t], dtype=bool) if len(idx) else np.zeros(0, dtype=bool)
    k = bit & (tid1 <= max_temporal_id_plus1) & (layer <= max_layer_id)
    return np.where(has, k, bool(keep_short))


def consistent(idx, stream_bytes):
    st = idx["start"].astype(np.uint64)
    en = idx["end"].astype(np.uint64)
    prev = np.concatenate([[0], en[:-1]]).astype(np.uint64) if len(idx) else en
    return not np.any((st > en) | (en > np.uint64(stream_bytes)) | (st < prev))


def filter_ref(stream, idx, keep):
    """stream: uint8 array; idx: entries; keep: bool array of len(idx).  Returns (out bytes, index_out, summary dict)
    for a consistent index."""
    s = np.asarray(stream, dtype=np.uint8)
    keep = np.asarray(keep, dtype=bool)
    n = len(idx)
    en = idx["end"].astype(np.int64)
    u = np.concatenate([[0], en[:-1]]).astype(np.int64) if n else en
    kk = np.nonzero(keep)[0]
    out = np.concatenate([s[u[k]:en[k]] for k in kk]) if len(kk) else np.zeros(0, dtype=np.uint8)
    io = np.zeros(len(kk), dtype=NAL_ENTRY)
    pos = 0
    roff = 0
    for j, k in enumerate(kk):
        io["start"][j] = pos + int(idx["start"][k]) - u[k]
        io["end"][j] = pos + en[k] - u[k]
        io["rbsp_off"][j] = roff
        io["rbsp_len"][j] = idx["rbsp_len"][k]
        io["status"][j] = int(idx["status"][k]) & ~ST_UNTERMINATED
        pos += en[k] - u[k]
        roff += int(idx["rbsp_len"][k])
    if len(kk):
        io["status"][-1] |= ST_UNTERMINATED
    summ = dict(nal_count=len(kk), nal_found=n, rbsp_bytes=roff, stream_bytes=len(out),
                stop_reason=-1 if len(kk) else 0, error=0)
    return out, io, summ


def rescan_misses_last(out, io):
    """The stated exception: find_nal_unit does not find the last kept NAL when its start code does not begin its unit
    and its payload is short (< 2 bytes behind 00 00 01, none behind 00 00 00 01)."""
    if not len(io):
        return False
    u = int(io["end"][-2]) if len(io) > 1 else 0
    st, en = int(io["start"][-1]), int(io["end"][-1])
    four = st - 4 >= u and out[st - 4] == 0
    i_f = st - 4 if four else st - 3
    return i_f > u and en - u <= i_f - u + 4


def random_stream(rng, size, mean, zeros_p=0.03):
    """An Annex-B stream of about `size` bytes, NAL payloads of about `mean` bytes with random two-byte headers (any type,
    layer, temporal id), 3- and 4-byte start codes, extra zeros and junk between NALs, sometimes leading junk, trailing zeros,
    an empty NAL the walk stops at, or a short last NAL."""
    out = bytearray()
    if rng.random() < 0.3:
        out += bytes(rng.integers(1, 256, size=int(rng.integers(1, 9)), dtype=np.uint8))
    while len(out) < size:
        r = rng.random()
        if r < 0.1:
            out += b"\x00" * int(rng.integers(1, 6))
        elif r < 0.15 and len(out):
            out += b"\x00\x00\x00" + bytes(rng.integers(4, 256, size=int(rng.integers(1, 5)), dtype=np.uint8))
        out += b"\x00\x00\x00\x01" if rng.random() < 0.4 else b"\x00\x00\x01"
        t = int(rng.integers(0, 64))
        layer = 0 if rng.random() < 0.7 else int(rng.integers(0, 64))
        tid1 = int(rng.integers(0, 8))
        plen = int(rng.geometric(1.0 / max(mean, 1)))
        if rng.random() < 0.05:
            plen = int(rng.integers(0, 3))
        pay = rng.integers(1, 256, size=plen, dtype=np.uint8)
        pay[rng.random(plen) < zeros_p] = 0
        hdr = bytes([(t << 1) | (layer >> 5), ((layer & 31) << 3) | tid1])
        out += (hdr + pay.tobytes())[: max(plen, 0)] if plen < 2 else hdr + pay[2:].tobytes()
    k = rng.random()
    if k < 0.15:
        out += b"\x00" * int(rng.integers(1, 8))
    elif k < 0.25:
        out += b"\x00\x00\x01\x00\x00\x01" + bytes(rng.integers(1, 256, size=20, dtype=np.uint8))    # empty NAL: the walk stops
    elif k < 0.35:
        out += b"\x00\x00\x01" + bytes(rng.integers(1, 256, size=int(rng.integers(0, 2)), dtype=np.uint8))
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()
