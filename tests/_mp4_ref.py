"""hbs_mp4_fragment and hbs_mp4_init_host restated in plain Python (include/hevcbitstream_amd.h is the specification): a writer
that is one loop over the access units, a reader that knows nothing of the writer and walks the boxes of what either wrote, and
random cases.  Test infrastructure: numpy and struct only, no GPU, nothing of the library."""
import struct

import numpy as np

NAL_ENTRY = np.dtype([("start", "<u8"), ("end", "<u8"), ("rbsp_off", "<u8"), ("rbsp_len", "<u4"), ("status", "<i4")])
ACCESS_UNIT = np.dtype([("first_nal", "<u8"), ("unit_begin", "<u8"), ("unit_end", "<u8"), ("nal_count", "<u4"), ("vcl_count", "<u4"),
                        ("first_vcl", "<u4"), ("nal_unit_type", "<i4"), ("temporal_id_plus1", "<i4"), ("pic_order_cnt", "<i4"),
                        ("poc_lsb", "<i4"), ("slice_types", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
PARAMS = np.dtype([("length_size", "<i4"), ("flags", "<u4"), ("track_id", "<u4"), ("sequence", "<u4"), ("max_samples", "<u4"),
                   ("sample_duration", "<u4"), ("base_time", "<u8")])
FRAG = np.dtype([("out_off", "<u8"), ("out_bytes", "<u8"), ("first_au", "<u8"), ("decode_time", "<u8"), ("samples", "<u4"),
                 ("sequence", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
INIT_PARAMS = np.dtype([("track_id", "<u4"), ("timescale", "<u4"), ("width", "<u4"), ("height", "<u4"), ("length_size", "<i4"),
                        ("chroma_format_idc", "<i4"), ("bit_depth_luma", "<i4"), ("bit_depth_chroma", "<i4")])
CUT_AT_IRAP = 1
HEV1 = 1
AU_IRAP = 1
E_ARG, E_CAPACITY = -3, -4
TIME_LIMIT = 1 << 62
M32 = (1 << 32) - 1
MDAT_MAX = (1 << 32) - 9
SAMPLES_MAX = ((1 << 32) - 89) // 16


def params(length_size=4, flags=0, track_id=1, sequence=1, max_samples=0, sample_duration=3000, base_time=0):
    return dict(length_size=length_size, flags=flags, track_id=track_id, sequence=sequence, max_samples=max_samples,
                sample_duration=sample_duration, base_time=base_time)


def params_record(prm):
    p = np.zeros(1, dtype=PARAMS)
    for k, v in prm.items():
        p[k][0] = v
    return p


def entries(starts, ends, seed=0):
    """a NAL_ENTRY table with the two fields the call reads; the others hold junk it must not look at"""
    n = len(starts)
    e = np.frombuffer(np.random.default_rng(n + seed).integers(0, 256, size=n * NAL_ENTRY.itemsize, dtype=np.uint8).tobytes(), dtype=NAL_ENTRY).copy()
    e["start"] = np.asarray(starts, dtype=np.uint64)
    e["end"] = np.asarray(ends, dtype=np.uint64)
    return e


def au_records(flags, seed=0):
    """an ACCESS_UNIT table with the one field the call reads (flags & HBS_AU_IRAP; the other flag bits are junk too)"""
    n = len(flags)
    rng = np.random.default_rng(n + 7 + seed)
    a = np.frombuffer(rng.integers(0, 256, size=n * ACCESS_UNIT.itemsize, dtype=np.uint8).tobytes(), dtype=ACCESS_UNIT).copy()
    a["flags"] = (a["flags"] & ~np.uint32(AU_IRAP)) | (np.asarray(flags, dtype=np.uint32) & np.uint32(AU_IRAP))
    return a


def fragment_bytes(samples, sample_bytes):
    return 96 + 16 * samples + sample_bytes


# ---- the writer ---------------------------------------------------------------------------------------------------------------

def box(kind, *payload):
    body = b"".join(payload)
    return struct.pack(">I4s", 8 + len(body), kind) + body


def full(kind, version, flags, *payload):
    return box(kind, struct.pack(">I", version << 24 | flags), *payload)


def one_fragment(sequence, track_id, decode_time, samples):
    """samples: [(duration, flags, cts, bytes)] -> the moof and the mdat"""
    S = len(samples)
    trun = full(b"trun", 1, 0x000F01, struct.pack(">II", S, 96 + 16 * S),
                *[struct.pack(">IIIi", d, len(b), f, c) for d, f, c, b in samples])
    moof = box(b"moof", full(b"mfhd", 0, 0, struct.pack(">I", sequence)),
               box(b"traf", full(b"tfhd", 0, 0x020000, struct.pack(">I", track_id)), full(b"tfdt", 1, 0, struct.pack(">Q", decode_time)), trun))
    return moof + box(b"mdat", *[b for _, _, _, b in samples])


def summary(error=0, frags=0, n_nals=0, rec=0, total=0, bad_nal=0, bad_au=0, kept=0):
    return dict(error=error, nal_count=frags, nal_found=n_nals, rbsp_bytes=rec, stream_bytes=total, stop_reason=0, reserved=[bad_nal, bad_au, kept])


def fragment(stream, index, keep, nal_au, au, dts, pts, prm, out_cap=None, frag_cap=None, stream_bytes=None):
    """-> (output uint8 array, sample_off, sample_size, ndarray[FRAG], summary dict); on an error the first four are None"""
    n, n_aus = len(index), len(au)
    nbytes = len(stream) if stream_bytes is None else stream_bytes
    L, M = prm["length_size"], prm["max_samples"]
    cut_irap = bool(prm["flags"] & CUT_AT_IRAP)
    data = bytes(stream) if not isinstance(stream, np.ndarray) else stream.tobytes()
    if n == 0:
        assert n_aus == 0
        return np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, FRAG), summary()
    # the NAL rules
    bad_nal, prev_end = 0, 0
    starts, ends, nal_au = index["start"].tolist(), index["end"].tolist(), np.asarray(nal_au).tolist()       # (plain ints)
    keep = None if keep is None else np.asarray(keep).tolist()
    au_flags = au["flags"].tolist()
    dts = None if dts is None else np.asarray(dts).tolist()
    pts = None if pts is None else np.asarray(pts).tolist()
    rel = [(x - nal_au[0]) & M32 for x in nal_au]
    for k in range(n):
        s, e = starts[k], ends[k]
        wrong = s > e or e > nbytes or s < prev_end
        if not wrong and (keep is None or keep[k]) and e - s > (1 << (8 * L)) - 1:
            wrong = True
        if k and ((nal_au[k] - nal_au[k - 1]) & M32) > 1:
            wrong = True
        if k == n - 1 and rel[k] + 1 != n_aus:
            wrong = True
        if wrong and not bad_nal:
            bad_nal = k + 1
        prev_end = e
    # the time rules
    def dts_of(a):
        return dts[a] if dts is not None else prm["base_time"] + a * prm["sample_duration"]
    bad_au = 0
    times = []
    for a in range(n_aus):
        d = dts_of(a)
        dur = prm["sample_duration"] if a == n_aus - 1 else dts_of(a + 1) - d
        p = pts[a] if pts is not None else d
        ok = d < TIME_LIMIT and 0 <= dur <= M32 and p < TIME_LIMIT and -(1 << 31) <= p - d <= (1 << 31) - 1
        if not ok and not bad_au:
            bad_au = a + 1
        times.append((d, dur, p - d))
    if bad_nal:
        return None, None, None, None, summary(E_ARG, n_nals=n, bad_nal=bad_nal, bad_au=bad_au)
    # ONE LOOP OVER THE ACCESS UNITS
    pieces, frags, sample_off, sample_size = [], [], [], []
    open_samples, first, s_of, at, rec, kept, k = [], 0, 0, 0, 0, 0, 0
    big = 0

    def close():
        nonlocal at, big
        if not open_samples:
            return
        S, P = len(open_samples), sum(len(b) for _, _, _, b in open_samples)
        if (P > MDAT_MAX or S > SAMPLES_MAX) and not big:
            big = first + 1
        r = len(frags)
        seq = (prm["sequence"] + r) & M32
        b = b"" if bad_au else one_fragment(seq, prm["track_id"], times[first][0], list(open_samples))
        frags.append((at, fragment_bytes(S, P), first, times[first][0], S, seq, au_flags[first] & AU_IRAP, 0))
        o = at + 96 + 16 * S
        for _, _, _, x in open_samples:
            sample_off.append(o)
            sample_size.append(len(x))
            o += len(x)
        pieces.append(b)
        at += fragment_bytes(S, P)
        open_samples.clear()

    for a in range(n_aus):
        irap = bool(au_flags[a] & AU_IRAP)
        if a == 0 or (cut_irap and irap):
            s_of = a
        if a == s_of or (M > 0 and (a - s_of) % M == 0):
            close()
            first = a
        recs = []
        while k < n and rel[k] == a:
            if keep is None or keep[k]:
                s, e = starts[k], ends[k]
                recs.append((e - s).to_bytes(L, "big") + data[s:e])
                kept += 1
            k += 1
        sample = b"".join(recs)
        rec += len(sample)
        d, dur, cts = times[a]
        open_samples.append((dur & M32, 0x02000000 if irap else 0x01010000, cts if -(1 << 31) <= cts < (1 << 31) else 0, sample))
    close()
    bad_au = min(x for x in (bad_au, big) if x) if (bad_au or big) else 0
    if bad_au:
        return None, None, None, None, summary(E_ARG, n_nals=n, bad_au=bad_au)
    R, total = len(frags), at
    assert total == rec + 16 * n_aus + 96 * R
    s = summary(0, R, n, rec, total, kept=kept)
    if (out_cap is not None and out_cap < total) or (frag_cap is not None and frag_cap < R):
        return None, None, None, None, dict(s, error=E_CAPACITY)
    out = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    assert len(out) == total
    return (out, np.array(sample_off, dtype=np.uint64), np.array(sample_size, dtype=np.uint64),
            np.array(frags, dtype=FRAG) if R else np.zeros(0, FRAG), s)


def strip_epb(nal, want=None):
    out, zeros = bytearray(), 0
    for b in nal:
        if want is not None and len(out) >= want:
            break
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        zeros = zeros + 1 if b == 0 else 0
        out.append(b)
    return bytes(out)


def init_segment(nals, track_id=1, timescale=90000, width=1920, height=1080, length_size=4, chroma_format_idc=1, bit_depth_luma=8,
                 bit_depth_chroma=8, flags=0):
    """-> bytes, or E_ARG"""
    nals = [bytes(x) for x in nals]
    if flags & ~HEV1 or not 1 <= len(nals) <= 65535 or not 1 <= track_id < M32 or not 1 <= timescale <= M32:
        return E_ARG
    if not (1 <= width <= 65535 and 1 <= height <= 65535 and length_size in (1, 2, 4) and 0 <= chroma_format_idc <= 3):
        return E_ARG
    if not (8 <= bit_depth_luma <= 15 and 8 <= bit_depth_chroma <= 15):
        return E_ARG
    for x in nals:
        if not 2 <= len(x) <= 65535 or not 32 <= (x[0] >> 1) & 0x3F <= 34:
            return E_ARG
    sps = [x for x in nals if (x[0] >> 1) & 0x3F == 33]
    if not sps:
        return E_ARG
    pre = strip_epb(sps[0], 15)
    if len(pre) < 15:
        return E_ARG
    hev1 = bool(flags & HEV1)
    arrays = []
    for t in (32, 33, 34):
        of = [x for x in nals if (x[0] >> 1) & 0x3F == t]
        if of:
            arrays.append(struct.pack(">BH", (0 if hev1 else 0x80) | t, len(of)) + b"".join(struct.pack(">H", len(x)) + x for x in of))
    hvcc = box(b"hvcC", b"\x01", pre[3:15], b"\xF0\x00\xFC", bytes([0xFC | chroma_format_idc, 0xF8 | (bit_depth_luma - 8), 0xF8 | (bit_depth_chroma - 8)]),
               b"\x00\x00", bytes([(((pre[2] >> 1) & 7) + 1) << 3 | (pre[2] & 1) << 2 | (length_size - 1), len(arrays)]), *arrays)
    matrix = struct.pack(">9I", 0x10000, 0, 0, 0, 0x10000, 0, 0, 0, 0x40000000)
    entry = box(b"hev1" if hev1 else b"hvc1", bytes(6), struct.pack(">H", 1), bytes(16), struct.pack(">HHIIIH", width, height, 0x480000, 0x480000, 0, 1),
                bytes(32), struct.pack(">HH", 0x18, 0xFFFF), hvcc)
    stbl = box(b"stbl", full(b"stsd", 0, 0, struct.pack(">I", 1), entry), full(b"stts", 0, 0, bytes(4)), full(b"stsc", 0, 0, bytes(4)),
               full(b"stsz", 0, 0, bytes(8)), full(b"stco", 0, 0, bytes(4)))
    minf = box(b"minf", full(b"vmhd", 0, 1, bytes(8)), box(b"dinf", full(b"dref", 0, 0, struct.pack(">I", 1), full(b"url ", 0, 1))), stbl)
    mdia = box(b"mdia", full(b"mdhd", 0, 0, struct.pack(">IIIIHH", 0, 0, timescale, 0, 0x55C4, 0)),
               full(b"hdlr", 0, 0, bytes(4), b"vide", bytes(12), b"VideoHandler\0"), minf)
    trak = box(b"trak", full(b"tkhd", 0, 3, struct.pack(">IIIII", 0, 0, track_id, 0, 0), bytes(8), bytes(8), matrix,
                             struct.pack(">II", width << 16, height << 16)), mdia)
    mvhd = full(b"mvhd", 0, 0, struct.pack(">IIII", 0, 0, timescale, 0), struct.pack(">IH", 0x10000, 0x100), bytes(10), matrix, bytes(24),
                struct.pack(">I", track_id + 1))
    moov = box(b"moov", mvhd, trak, box(b"mvex", full(b"trex", 0, 0, struct.pack(">IIIII", track_id, 1, 0, 0, 0))))
    return box(b"ftyp", b"iso6", bytes(4), b"iso6", b"mp41") + moov


# ---- the reader ---------------------------------------------------------------------------------------------------------------

CONTAINERS = {b"moof", b"traf", b"moov", b"trak", b"mdia", b"minf", b"dinf", b"stbl", b"mvex"}


def u32(b, at):
    return int.from_bytes(b[at:at + 4], "big")


def walk(b, lo, hi):
    """the boxes that tile b[lo, hi) exactly: [(type, payload begin, end)]"""
    found = []
    while lo < hi:
        assert hi - lo >= 8, "a box header leaves its parent"
        size, kind = u32(b, lo), bytes(b[lo + 4:lo + 8])
        assert 8 <= size <= hi - lo, ("box %r of %d bytes in %d" % (kind, size, hi - lo))
        found.append((kind, lo + 8, lo + size))
        lo += size
    assert lo == hi
    return found


def tree(b, lo, hi):
    """{type: [(payload begin, end)]} of every box below b[lo, hi), containers walked through"""
    seen = {}
    for kind, p, e in walk(b, lo, hi):
        seen.setdefault(kind, []).append((p, e))
        if kind in CONTAINERS:
            for k2, v in tree(b, p, e).items():
                seen.setdefault(k2, []).extend(v)
    return seen


def only(t, kind):
    assert len(t.get(kind, [])) == 1, (kind, t.get(kind))
    return t[kind][0]


def read_fragments(b):
    """b: moof + mdat pairs.  -> [dict(off, bytes, sequence, track_id, decode_time, samples=[(off, size, duration, flags, cts)])]"""
    b = bytes(b)
    top = walk(b, 0, len(b))
    assert len(top) % 2 == 0 and all(k == (b"moof", b"mdat")[i % 2] for i, (k, _, _) in enumerate(top)), [k for k, _, _ in top]
    frags = []
    for (_, mp, me), (_, dp, de) in zip(top[0::2], top[1::2]):
        moof_at = mp - 8
        t = tree(b, mp, me)
        assert sorted(t) == [b"mfhd", b"tfdt", b"tfhd", b"traf", b"trun"], sorted(t)
        p, e = only(t, b"mfhd")
        assert e - p == 8 and u32(b, p) == 0
        seq = u32(b, p + 4)
        p, e = only(t, b"tfhd")
        assert e - p == 8 and u32(b, p) == 0x00020000, "tfhd: default-base-is-moof and nothing else"
        track = u32(b, p + 4)
        p, e = only(t, b"tfdt")
        assert e - p == 12 and u32(b, p) == 0x01000000
        dt = int.from_bytes(b[p + 4:p + 12], "big")
        p, e = only(t, b"trun")
        assert u32(b, p) == 0x01000F01
        count, data_offset = u32(b, p + 4), u32(b, p + 8)
        assert e - p == 12 + 16 * count
        assert moof_at + data_offset == dp, "data_offset does not land behind the mdat header"
        at, samples = dp, []
        for i in range(count):
            q = p + 12 + 16 * i
            dur, size, fl = u32(b, q), u32(b, q + 4), u32(b, q + 8)
            cts = int.from_bytes(b[q + 12:q + 16], "big", signed=True)
            samples.append((at, size, dur, fl, cts))
            at += size
        assert at == de, "the trun sizes do not add up to the mdat"
        frags.append(dict(off=moof_at, bytes=de - moof_at, sequence=seq, track_id=track, decode_time=dt, samples=samples))
    return frags


def read_init(b):
    """-> dict(entry, track_id, timescale, width, height, config (the 22 bytes in front of numOfArrays), arrays=[(byte, [nal])])"""
    b = bytes(b)
    top = walk(b, 0, len(b))
    assert [k for k, _, _ in top] == [b"ftyp", b"moov"]
    assert b[top[0][1]:top[0][2]] == b"iso6\0\0\0\0iso6mp41"
    t = tree(b, top[1][1], top[1][2])
    p, e = only(t, b"mvhd")
    assert e - p == 100
    timescale, next_track = u32(b, p + 12), u32(b, e - 4)
    p, e = only(t, b"tkhd")
    assert e - p == 84 and u32(b, p) == 3
    track = u32(b, p + 12)
    tw, th = u32(b, e - 8), u32(b, e - 4)
    assert next_track == track + 1
    p, e = only(t, b"mdhd")
    assert u32(b, p + 12) == timescale
    p, e = only(t, b"hdlr")
    assert b[p + 8:p + 12] == b"vide"
    p, e = only(t, b"trex")
    assert u32(b, p + 4) == track and u32(b, p + 8) == 1
    for k in (b"stts", b"stsc", b"stco", b"stsz", b"vmhd", b"dref"):
        only(t, k)
    p, e = only(t, b"stsd")
    assert u32(b, p + 4) == 1
    (kind, sp, se), = walk(b, p + 8, e)
    assert kind in (b"hvc1", b"hev1")
    width, height = int.from_bytes(b[sp + 24:sp + 26], "big"), int.from_bytes(b[sp + 26:sp + 28], "big")
    assert (tw, th) == (width << 16, height << 16)
    (k2, cp, ce), = walk(b, sp + 78, se)
    assert k2 == b"hvcC"
    config, arrays, at = b[cp:cp + 22], [], cp + 23
    for _ in range(b[cp + 22]):
        head, cnt = b[at], int.from_bytes(b[at + 1:at + 3], "big")
        at += 3
        nals = []
        for _ in range(cnt):
            ln = int.from_bytes(b[at:at + 2], "big")
            nals.append(b[at + 2:at + 2 + ln])
            at += 2 + ln
        arrays.append((head, nals))
    assert at == ce
    return dict(entry=kind, track_id=track, timescale=timescale, width=width, height=height, config=config, arrays=arrays)


def samples_to_nals(b, off, size, L):
    """the payloads of the records of sample b[off, off + size)"""
    out, p, e = [], off, off + size
    while p < e:
        assert e - p >= L
        n = int.from_bytes(b[p:p + L], "big")
        assert n <= e - p - L
        out.append(bytes(b[p + L:p + L + n]))
        p += L + n
    return out


# ---- random cases -------------------------------------------------------------------------------------------------------------

def random_case(rng, n_aus, max_nal=300, max_nals_per_au=4, keep_some=True, irap_every=None, times=True, neg_cts=True, lead=None,
                gaps=True, empty_aus=True, au_base=None):
    """-> (stream, index, keep or None, nal_au, au, dts or None, pts or None).  lead: bytes in front of the first NAL (its
    alignment); irap_every: None for random IRAPs (AU 0 is never one then), else the distance."""
    counts = rng.integers(1, max_nals_per_au + 1, size=n_aus)
    n = int(counts.sum())
    lens = rng.integers(0, max_nal + 1, size=n)
    small = rng.integers(0, 5, size=n) == 0
    lens[small] = rng.integers(0, 4, size=int(small.sum()))
    gap = rng.integers(3, 9, size=n) if gaps else np.full(n, 3)
    if n:
        gap[0] = int(rng.integers(3, 40)) if lead is None else lead
    starts = np.cumsum(gap + np.concatenate(([0], lens[:-1]))) if n else np.zeros(0, np.int64)
    ends = starts + lens
    total = int(ends[-1]) + int(rng.integers(0, 5)) if n else 0
    stream = rng.integers(0, 256, size=total, dtype=np.uint8)
    index = entries(starts, ends, seed=int(rng.integers(1 << 30)))
    base = int(rng.integers(0, 1000)) if au_base is None else au_base
    nal_au = ((np.repeat(np.arange(n_aus, dtype=np.uint64), counts) + base) & M32).astype(np.uint32)
    keep = None
    if keep_some:
        keep = (rng.integers(0, 4, size=n) != 0).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8)
        if empty_aus and n_aus > 2:
            for a in rng.integers(0, n_aus, size=max(1, n_aus // 8)):
                keep[np.repeat(np.arange(n_aus), counts) == a] = 0
    if irap_every is None:
        fl = (rng.integers(0, 5, size=n_aus) == 0).astype(np.uint32)
        if n_aus:
            fl[0] = 0
    else:
        fl = (np.arange(n_aus) % irap_every == 0).astype(np.uint32)
    au = au_records(fl, seed=int(rng.integers(1 << 30)))
    dts = pts = None
    if times:
        step = rng.integers(0, 6000, size=n_aus).astype(np.uint64)
        dts = (np.uint64(int(rng.integers(0, 1 << 40))) + np.concatenate(([0], np.cumsum(step)[:-1])).astype(np.uint64)).astype(np.uint64)
        off = rng.integers(-5000 if neg_cts else 0, 20000, size=n_aus)
        pts = (dts.astype(np.int64) + np.maximum(off, -dts.astype(np.int64))).astype(np.uint64)
    return stream, index, keep, nal_au, au, dts, pts
