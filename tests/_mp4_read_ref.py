"""hbs_mp4_samples / hbs_mp4_init_read_host in plain Python, from ISO/IEC 14496-12 and the call's header comment and
independent of the C rule functions (hbs_mp4rd.h): a reader that goes box by box with exact integers, a general fragment writer
that uses every optional field the call honours, and a generator of random valid segments that knows what it wrote."""
import itertools
import struct

import numpy as np

from tests import _mp4_ref as R

E_ARG, E_CAPACITY = -3, -4
AU_IRAP = 1
TIME_LIMIT = 1 << 62
READ_PARAMS = np.dtype([("flags", "<u4"), ("track_id", "<u4"), ("trex_duration", "<u4"), ("trex_size", "<u4"), ("trex_flags", "<u4"),
                        ("reserved", "<u4", (3,))])
TRACK = np.dtype([("track_id", "<u4"), ("timescale", "<u4"), ("width", "<u4"), ("height", "<u4"), ("length_size", "<i4"),
                  ("entry", "<u4"), ("trex_duration", "<u4"), ("trex_size", "<u4"), ("trex_flags", "<u4"), ("n_nals", "<u4"),
                  ("hvcc_off", "<u8"), ("hvcc_bytes", "<u8"), ("reserved", "<u4", (2,))])


def read_params(track_id=0, trex_duration=0, trex_size=0, trex_flags=0):
    return dict(track_id=track_id, trex_duration=trex_duration, trex_size=trex_size, trex_flags=trex_flags)


# ---- the reader ---------------------------------------------------------------------------------------------------------------

class Malformed(Exception):
    pass


def be(b, at, n, signed=False):
    return int.from_bytes(b[at:at + n], "big", signed=signed)


def each_box(b, lo, hi):
    """the boxes that tile b[lo, hi), one at a time: (type, box begin, payload begin, end); Malformed when the one that is
    reached breaks a size rule (what lies behind the last one taken is not looked at)"""
    while lo < hi:
        if hi - lo < 8:
            raise Malformed("header leaves the container")
        size, kind, head = be(b, lo, 4), bytes(b[lo + 4:lo + 8]), 8
        if size == 1:
            if hi - lo < 16:
                raise Malformed("largesize leaves the container")
            size, head = be(b, lo + 8, 8), 16
            if size < 16:
                raise Malformed("largesize below 16")
        elif size == 0:
            size = hi - lo
        elif size < 8:
            raise Malformed("size below 8")
        if size > hi - lo:
            raise Malformed("box leaves the container")
        yield kind, lo, lo + head, lo + size
        lo += size


def boxes(b, lo, hi):
    """all the boxes that tile b[lo, hi): [(type, box begin, payload begin, end)]; Malformed when one breaks a size rule"""
    return list(each_box(b, lo, hi))


def stsd_entries(b, lo, hi, count):
    """the sample entries of a stsd whose payload is b[lo, hi), one at a time and entry_count at the most: the caller stops at the
    entry it chooses, and nothing behind that one is looked at"""
    return itertools.islice(each_box(b, lo + 8, hi), count)


def read_traf(b, p, e):
    """-> (the first tfhd as a dict, the children)"""
    kids = boxes(b, p, e)
    for kind, _, kp, ke in kids:
        if kind == b"tfhd":
            if ke - kp < 8:
                raise Malformed("tfhd too short")
            fl = be(b, kp, 4) & 0xFFFFFF
            h = dict(flags=fl, track_id=be(b, kp + 4, 4))
            at = kp + 8
            for bit, name, n in ((1, "base", 8), (2, "sdi", 4), (8, "dur", 4), (0x10, "size", 4), (0x20, "sflags", 4)):
                if fl & bit:
                    if ke - at < n:
                        raise Malformed("tfhd too short for its flags")
                    h[name] = be(b, at, n)
                    at += n
            return h, kids
    raise Malformed("traf without tfhd")


RUN = 4096          # a trun of more samples than this whose entries have no bytes is kept as one Run


class Run:
    """`count` samples of one size and duration with no composition offset, from `begin` on"""
    def __init__(self, begin, count, size, dur, first_flags, flags):
        self.begin, self.count, self.size, self.dur, self.first_flags, self.flags = begin, count, size, dur, first_flags, flags

    def good(self, e, t, n):
        """sample e, whose moof's time stands at t in front of the run, in a buffer of n bytes"""
        return self.begin >= 0 and self.begin + (e + 1) * self.size <= n and 0 <= t + e * self.dur < TIME_LIMIT

    def lowest_bad(self, t, n):
        """offsets and times grow with e: bisection.  None: all good"""
        if self.good(self.count - 1, t, n):
            return None
        lo, hi = -1, self.count - 1                            # lo good (or -1), hi bad
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if self.good(mid, t, n) else (lo, mid)
        return hi


def n_samples(x):
    return sum(e.count if isinstance(e, Run) else 1 for e in x["samples"])


def read_moof(b, seg_off, at, pay, end, prm):
    """-> dict(sequence, tfdt, samples=[(begin, before, size, duration, flags, cts)]): offset = begin + before, exact integers"""
    seq, chosen, traf_i = None, None, 0
    for kind, _, p, e in boxes(b, pay, end):
        if kind == b"mfhd" and seq is None:
            if e - p < 8 or b[p] != 0:
                raise Malformed("mfhd")
            seq = be(b, p + 4, 4)
        elif kind == b"traf":
            if chosen is None:
                h, kids = read_traf(b, p, e)
                if prm["track_id"] in (0, h["track_id"]):
                    chosen = (h, kids, traf_i)
            traf_i += 1
    if seq is None:
        raise Malformed("no mfhd")
    out = dict(sequence=seq, tfdt=0, samples=[])
    if chosen is None:
        return out
    h, kids, traf_i = chosen
    dt = [k for k in kids if k[0] == b"tfdt"]
    if not dt:
        raise Malformed("no tfdt")
    _, _, p, e = dt[0]
    if e - p < 4 or b[p] > 1 or e - p < (12 if b[p] else 8):
        raise Malformed("tfdt")
    out["tfdt"] = be(b, p + 4, 8 if b[p] else 4)
    if h["flags"] & 1:
        base = seg_off + h["base"]
    elif (h["flags"] & 0x020000) or traf_i == 0:
        base = at
    else:
        raise Malformed("base = end of the previous traf's data")
    ddur, dsize, dflags = h.get("dur", prm["trex_duration"]), h.get("size", prm["trex_size"]), h.get("sflags", prm["trex_flags"])
    nxt = base                                             # where a trun without a data_offset begins
    for kind, _, p, e in kids:
        if kind != b"trun":
            continue
        if e - p < 8:
            raise Malformed("trun too short")
        ver, fl, count = b[p], be(b, p, 4) & 0xFFFFFF, be(b, p + 4, 4)
        if ver > 1:
            raise Malformed("trun version")
        q = p + 8
        per = 4 * bin(fl & 0xF00).count("1")
        if 8 + (4 if fl & 1 else 0) + (4 if fl & 4 else 0) + count * per > e - p:
            raise Malformed("trun entries leave the box")
        begin = nxt
        if fl & 1:
            begin = base + be(b, q, 4, signed=True)
            q += 4
        first = None
        if fl & 4:
            first = be(b, q, 4)
            q += 4
        if per == 0 and count > RUN:
            # entries of no bytes: the count is bounded by nothing in the box, so the samples are not listed one by one
            out["samples"].append(Run(begin, count, dsize, ddur, first if first is not None else dflags, dflags))
            nxt = begin + count * dsize
            continue
        before = 0
        for i in range(count):
            dur, size, sfl, cts = ddur, dsize, (first if (i == 0 and first is not None) else dflags), 0
            if fl & 0x100:
                dur = be(b, q, 4)
                q += 4
            if fl & 0x200:
                size = be(b, q, 4)
                q += 4
            if fl & 0x400:
                sfl = be(b, q, 4)
                q += 4
            if fl & 0x800:
                cts = be(b, q, 4, signed=(ver == 1))
                q += 4
            out["samples"].append((begin, before, size, dur, sfl, cts))
            before += size
        nxt = begin + before
    return out


def summary(error=0, n=0, m=0, size=0, total=0, bad=(0, 0, 0)):
    return dict(error=error, nal_count=n, nal_found=m, rbsp_bytes=size, stream_bytes=total, stop_reason=0, reserved=list(bad))


TABLE_MAX = 1 << 24          # more samples than this are counted and checked, not listed


def samples(data, segs, prm, moof_cap=None, sample_cap=None, in_bytes=None, tables=True):
    """segs: None (the buffer) or [(off, size)].  -> (off, size, dts, pts, flags, frags, summary dict): arrays, None on an
    error (and the five sample tables None with tables=False or above TABLE_MAX samples).  moof_cap / sample_cap None: no limit."""
    b = bytes(data) if not isinstance(data, np.ndarray) else data.tobytes()
    n = len(b) if in_bytes is None else in_bytes
    fail = lambda s: (None, None, None, None, None, None, s)          # noqa: E731
    if segs is None:
        segs = [(0, n)]
    moofs, bad_seg = [], 0
    for i, (off, size) in enumerate(segs):
        try:
            if off + size > n:
                raise Malformed("segment leaves the buffer")
            found = [(k, s, p, e) for k, s, p, e in boxes(b, off, off + size) if k == b"moof"]
        except Malformed:
            bad_seg = bad_seg or i + 1
            continue
        for j, (_, s, p, e) in enumerate(found):
            span = (found[j + 1][1] if j + 1 < len(found) else off + size) - s
            moofs.append((off, s, p, e, span))
    if bad_seg:
        return fail(summary(E_ARG, total=n, bad=(bad_seg, 0, 0)))
    M = len(moofs)
    if moof_cap is not None and M > moof_cap:
        return fail(summary(E_CAPACITY, m=M, total=n))
    parsed, bad_moof = [], 0
    for i, (off, s, p, e, span) in enumerate(moofs):
        try:
            parsed.append(read_moof(b, off, s, p, e, prm))
        except Malformed:
            bad_moof = bad_moof or i + 1
    if bad_moof:
        return fail(summary(E_ARG, m=M, total=n, bad=(0, bad_moof, 0)))
    N = sum(n_samples(x) for x in parsed)
    if sample_cap is not None and N > sample_cap:
        return fail(summary(E_CAPACITY, n=N, m=M, total=n))
    cols, frags, bad_sample, k, total = [[] for _ in range(5)], [], 0, 0, 0
    listed = tables and N <= TABLE_MAX
    for (off, s, p, e, span), x in zip(moofs, parsed):
        t = x["tfdt"]
        first = x["samples"][0] if x["samples"] else None
        first_flags = first.first_flags if isinstance(first, Run) else first[4] if first else 0x00010000
        frags.append((s, span, k, x["tfdt"], n_samples(x) & 0xFFFFFFFF, x["sequence"], 0 if first_flags & 0x00010000 else AU_IRAP, 0))
        for item in x["samples"]:
            if isinstance(item, Run):
                low = item.lowest_bad(t, n)
                if low is not None:
                    bad_sample = bad_sample or k + low + 1
                if listed and not bad_sample:
                    ar = np.arange(item.count, dtype=np.uint64)
                    fl = np.full(item.count, item.flags, dtype=np.uint64)
                    fl[0] = item.first_flags
                    d = np.uint64(t) + np.uint64(item.dur) * ar
                    for c, v in zip(cols, (np.uint64(max(item.begin, 0)) + np.uint64(item.size) * ar, np.full(item.count, item.size, np.uint64), d, d, fl)):
                        c.append(v)
                total += item.count * item.size
                t += item.count * item.dur
                k += item.count
                continue
            begin, before, size, dur, sfl, cts = item
            o = begin + before
            ok = begin >= 0 and o + size <= n and t < TIME_LIMIT and 0 <= t + cts < TIME_LIMIT
            if not ok:
                bad_sample = bad_sample or k + 1
            if listed and not bad_sample:
                for c, v in zip(cols, (o, size, t, t + cts, sfl)):
                    c.append(np.array([v], dtype=np.uint64))
            total += size
            t += dur
            k += 1
    if bad_sample:
        return fail(summary(E_ARG, n=N, m=M, total=n, bad=(0, 0, bad_sample)))
    fr = np.array(frags, dtype=R.FRAG) if frags else np.zeros(0, R.FRAG)
    if not listed:
        return (None, None, None, None, None, fr, summary(0, N, M, total, n))
    cat = lambda c: np.concatenate(c) if c else np.zeros(0, np.uint64)          # noqa: E731
    return (cat(cols[0]), cat(cols[1]), cat(cols[2]), cat(cols[3]), cat(cols[4]).astype(np.uint32), fr, summary(0, N, M, total, n))


# ---- the writer ---------------------------------------------------------------------------------------------------------------

def box(kind, payload=b"", large=False, zero=False):
    """large: a 64-bit largesize; zero: size 0, "to the container's end" (only right for a container's last box)"""
    if zero:
        return struct.pack(">I4s", 0, kind) + payload
    if large:
        return struct.pack(">I4sQ", 1, kind, 16 + len(payload)) + payload
    return struct.pack(">I4s", 8 + len(payload), kind) + payload


def full(kind, version, flags, payload=b"", **kw):
    return box(kind, struct.pack(">I", version << 24 | flags) + payload, **kw)


def mfhd(sequence, **kw):
    return full(b"mfhd", 0, 0, struct.pack(">I", sequence), **kw)


def tfhd(track_id, flags=0x020000, base=0, sdi=1, dur=0, size=0, sflags=0, **kw):
    p = struct.pack(">I", track_id)
    if flags & 1:
        p += struct.pack(">Q", base)
    for bit, v in ((2, sdi), (8, dur), (0x10, size), (0x20, sflags)):
        if flags & bit:
            p += struct.pack(">I", v)
    return full(b"tfhd", 0, flags, p, **kw)


def tfdt(time, version=1, **kw):
    return full(b"tfdt", version, 0, struct.pack(">Q" if version else ">I", time), **kw)


def trun(flags, entries, version=0, data_offset=0, first_flags=0, count=None, **kw):
    """entries: [(duration, size, flags, cts)]; only the fields that `flags` names are written"""
    p = struct.pack(">I", len(entries) if count is None else count)
    if flags & 1:
        p += struct.pack(">i", data_offset)
    if flags & 4:
        p += struct.pack(">I", first_flags)
    for dur, size, sfl, cts in entries:
        if flags & 0x100:
            p += struct.pack(">I", dur)
        if flags & 0x200:
            p += struct.pack(">I", size)
        if flags & 0x400:
            p += struct.pack(">I", sfl)
        if flags & 0x800:
            p += struct.pack(">i" if version else ">I", cts)
    return full(b"trun", version, flags, p, **kw)


FOREIGN_TOP = (b"styp", b"sidx", b"prft", b"emsg", b"free")
FOREIGN_TRAF = (b"senc", b"saiz", b"saio", b"sbgp", b"sgpd", b"uuid")


def junk(rng, kinds):
    return box(kinds[int(rng.integers(len(kinds)))], rng.integers(0, 256, size=int(rng.integers(0, 24)), dtype=np.uint8).tobytes(),
               large=bool(rng.integers(4) == 0))


def random_moof(rng, moof_at, seg_off, prm, counts=None, sequence=None, first_sample=0, plain=False, tflags=None):
    """One moof and its mdat for the file position moof_at of a segment that begins at seg_off, read with prm.  counts: the
    sample count of each trun (None: random).  plain: no foreign boxes, no gaps (for shapes whose size matters).  tflags: the
    flags of each trun (None: random).
    -> (bytes, [(off, size, dts, pts, flags)], frag tuple without out_bytes)"""
    track = prm["track_id"] or int(rng.integers(1, 9))
    if counts is None:
        counts = [int(rng.integers(0, 7)) for _ in range(int(rng.integers(1, 5)))]
        if rng.integers(8) == 0:
            counts = []
    hfl = 0
    for bit in (1, 2, 8, 0x10, 0x20, 0x010000, 0x020000):
        if rng.integers(2):
            hfl |= bit
    foreign_first = (not plain) and bool(rng.integers(3) == 0)
    if foreign_first and not (hfl & 0x020001):
        hfl |= 0x020000
    hd, hs, hf = int(rng.integers(1, 5000)), int(rng.integers(0, 40)), int(rng.integers(0, 1 << 32))
    ddur = hd if hfl & 8 else prm["trex_duration"]
    dsize = hs if hfl & 0x10 else prm["trex_size"]
    dflags = hf if hfl & 0x20 else prm["trex_flags"]
    tver = int(rng.integers(2))
    time = int(rng.integers(0, 1 << 32)) if tver == 0 else int(rng.integers(0, 1 << 50))
    seq = int(rng.integers(0, 1 << 32)) if sequence is None else sequence
    plan = []
    for ti, c in enumerate(counts):
        fl = 0
        for bit in (1, 4, 0x100, 0x200, 0x400, 0x800):
            if rng.integers(2):
                fl |= bit
        if tflags is not None:
            fl = tflags[ti]
        ver, first = int(rng.integers(2)), int(rng.integers(0, 1 << 32))
        ent = []
        for i in range(c):
            dur = int(rng.integers(0, 6000)) if fl & 0x100 else ddur
            size = int(rng.integers(0, 60)) if fl & 0x200 else dsize
            sfl = int(rng.integers(0, 1 << 32)) if fl & 0x400 else (first if (i == 0 and fl & 4) else dflags)
            cts = 0
            if fl & 0x800:
                cts = int(rng.integers(-3000, 9000)) if ver else int(rng.integers(0, 9000))
            ent.append((dur, size, sfl, cts))
        plan.append(dict(flags=fl, version=ver, first=first, entries=ent, gap=0 if plain else int(rng.integers(0, 9)), data_offset=0))

    def build(base_field):
        kids = []
        if not plain and rng_state["junk"][0]:
            kids.append(rng_state["junk_boxes"][0])
        kids.append(tfhd(track, hfl, base=base_field, dur=hd, size=hs, sflags=hf, large=rng_state["large"][0]))
        if not plain and rng_state["junk"][1]:
            kids.append(rng_state["junk_boxes"][1])
        kids.append(tfdt(time, tver))
        for i, t in enumerate(plan):
            kids.append(trun(t["flags"], t["entries"], t["version"], t["data_offset"], t["first"], large=rng_state["large"][1] and i == 0))
            if not plain and rng_state["junk"][2] and i == 0:
                kids.append(rng_state["junk_boxes"][2])
        traf = box(b"traf", b"".join(kids), large=rng_state["large"][2])
        top = []
        if foreign_first:
            top.append(rng_state["other_traf"])
        if not plain and rng_state["junk"][3]:
            top.append(rng_state["junk_boxes"][3])
        top.append(mfhd(seq))
        top.append(traf)
        if not plain and rng_state["junk"][4]:
            top.append(rng_state["other_traf"])            # a foreign traf behind ours
        return box(b"moof", b"".join(top), large=rng_state["large"][3])

    other = (track % 8) + 1 if prm["track_id"] else track + 1
    rng_state = dict(junk=[bool(rng.integers(3) == 0) for _ in range(5)], junk_boxes=[junk(rng, FOREIGN_TRAF) for _ in range(4)],
                     large=[(not plain) and bool(rng.integers(5) == 0) for _ in range(4)],
                     other_traf=box(b"traf", tfhd(other, 0x020000) + tfdt(7, 0) + trun(0x200, [(0, 5, 0, 0)] * 2)))
    if prm["track_id"] == 0:
        foreign_first = False                              # (track 0 reads the first traf: ours must be it)
        rng_state["junk"][4] = rng_state["junk"][4]        # a traf behind ours is ignored either way
    moof = build(0)
    mdat_head = 8
    pay_at = moof_at + len(moof) + mdat_head               # the mdat's payload in the file
    lead = 0 if plain else int(rng.integers(0, 16))        # mdat bytes in front of the first sample
    if hfl & 1:
        base = pay_at                                      # base_data_offset points at the mdat's payload
        base_field = base - seg_off
    else:
        base, base_field = moof_at, 0
    # where each trun's data begins: with a data_offset anywhere we like (behind the previous, with a gap); without, where
    # the rule puts it
    want, nxt, expect, t, k = pay_at + lead, base, [], time, first_sample
    for tr in plan:
        if tr["flags"] & 1:
            begin = max(want, nxt if nxt >= pay_at else want) + tr["gap"]
            tr["data_offset"] = begin - base
        else:
            begin = nxt
        o = begin
        for dur, size, sfl, cts in tr["entries"]:
            expect.append((o, size, t, t + cts, sfl))
            o += size
            t += dur
        nxt = o
        want = max(want, o) if o >= pay_at else want
    if any(p < 0 for _, _, _, p, _ in expect):
        # (a negative composition offset in front of the tfdt time: shift the time)
        return random_moof(rng, moof_at, seg_off, prm, counts, sequence, first_sample, plain, tflags)
    moof2 = build(base_field)
    assert len(moof2) == len(moof)
    reach = max([pay_at + lead] + [o + s for o, s, _, _, _ in expect])
    payload = rng.integers(0, 256, size=reach - pay_at + (0 if plain else int(rng.integers(0, 5))), dtype=np.uint8).tobytes()
    sync = bool(expect) and not (expect[0][4] & 0x00010000)
    frag = (moof_at, first_sample, time, len(expect), seq, AU_IRAP if sync else 0)
    return moof2 + box(b"mdat", payload), expect, frag


def random_segments(rng, n_segs, prm, moofs_per_seg=(1, 4), lead=0, zero_last=True):
    """-> (buffer bytes, [(off, size)], expected samples [(off, size, dts, pts, flags)], expected ndarray[FRAG])"""
    buf, segs, expect, frags = bytearray(rng.integers(0, 256, size=lead, dtype=np.uint8).tobytes()), [], [], []
    for _ in range(n_segs):
        seg_off = len(buf)
        seg = bytearray()
        marks = []
        for _ in range(int(rng.integers(moofs_per_seg[0], moofs_per_seg[1] + 1))):
            while rng.integers(3) == 0:
                seg += junk(rng, FOREIGN_TOP)
            b, e, f = random_moof(rng, seg_off + len(seg), seg_off, prm, first_sample=len(expect))
            marks.append((seg_off + len(seg), f))
            seg += b
            expect += e
        if zero_last and rng.integers(2):
            seg += box(b"free", rng.integers(0, 256, size=int(rng.integers(0, 9)), dtype=np.uint8).tobytes(), zero=True)
        elif rng.integers(3) == 0:
            seg += junk(rng, FOREIGN_TOP)
        for j, (at, f) in enumerate(marks):
            end = marks[j + 1][0] if j + 1 < len(marks) else seg_off + len(seg)
            frags.append((f[0], end - at, f[1], f[2], f[3], f[4], f[5], 0))
        segs.append((seg_off, len(seg)))
        buf += seg
        buf += rng.integers(0, 256, size=int(rng.integers(0, 3)) * 8, dtype=np.uint8).tobytes()       # between segments
    return bytes(buf), segs, expect, (np.array(frags, dtype=R.FRAG) if frags else np.zeros(0, R.FRAG))


def expected_tables(expect):
    u64 = lambda i: np.array([e[i] for e in expect], dtype=np.uint64)          # noqa: E731
    return u64(0), u64(1), u64(2), u64(3), np.array([e[4] for e in expect], dtype=np.uint32)


# ---- the init segment ---------------------------------------------------------------------------------------------------------

def init_read(b, track_id=0):
    """-> (dict of hbs_mp4_track's fields, [(off, size)] of the hvcC's NALs); Malformed for what the call refuses"""
    b = bytes(b)

    def child(lo, hi, kind):
        for k, _, p, e in boxes(b, lo, hi):
            if k == kind:
                return p, e
        return None

    moov = child(0, len(b), b"moov")
    if moov is None:
        raise Malformed("no moov")
    got = None
    for k, _, p, e in boxes(b, *moov):
        if k != b"trak" or got is not None:
            continue
        tk = child(p, e, b"tkhd")
        if tk is None or tk[1] - tk[0] < 4 or b[tk[0]] > 1 or tk[1] - tk[0] < (96 if b[tk[0]] else 84):
            raise Malformed("tkhd")
        v = b[tk[0]]
        t = dict(track_id=be(b, tk[0] + (20 if v else 12), 4), width=be(b, tk[0] + (88 if v else 76), 4) >> 16,
                 height=be(b, tk[0] + (92 if v else 80), 4) >> 16)
        mdia = child(p, e, b"mdia")
        if mdia is None:
            raise Malformed("no mdia")
        md = child(*mdia, b"mdhd")
        if md is None or md[1] - md[0] < 4 or b[md[0]] > 1 or md[1] - md[0] < (32 if b[md[0]] else 20):
            raise Malformed("mdhd")
        t["timescale"] = be(b, md[0] + (20 if b[md[0]] else 12), 4)
        at, video = mdia, None
        for depth, kind in enumerate((b"minf", b"stbl", b"stsd")):
            at = child(*at, kind)
            if at is None:
                if depth == 0:
                    break
                raise Malformed("no %r" % kind)
        if at is not None:
            if at[1] - at[0] < 8:
                raise Malformed("stsd")
            count = be(b, at[0] + 4, 4)
            for k2, _, sp, se in stsd_entries(b, at[0], at[1], count):
                if k2 in (b"hvc1", b"hev1"):
                    if se - sp < 78:
                        raise Malformed("sample entry")
                    hv = child(sp + 78, se, b"hvcC")
                    if hv is not None:
                        video = (k2, hv)
                        break
        mine = (video is not None) if track_id == 0 else t["track_id"] == track_id
        if not mine:
            continue
        if video is None:
            raise Malformed("the track has no hvcC")
        kind, (hp, he) = video
        if he - hp < 23 or b[hp] != 1:
            raise Malformed("hvcC")
        t.update(entry=be(kind, 0, 4), length_size=(b[hp + 21] & 3) + 1, hvcc_off=hp, hvcc_bytes=he - hp)
        nals, q = [], hp + 23
        for _ in range(b[hp + 22]):
            if he - q < 3:
                raise Malformed("hvcC array")
            cnt = be(b, q + 1, 2)
            q += 3
            for _ in range(cnt):
                if he - q < 2 or he - q - 2 < be(b, q, 2):
                    raise Malformed("hvcC NAL")
                nals.append((q + 2, be(b, q, 2)))
                q += 2 + be(b, q, 2)
        t["n_nals"] = len(nals)
        got = (t, nals)
    if got is None:
        raise Malformed("no such track")
    t, nals = got
    mvex = child(*moov, b"mvex")
    if mvex is None:
        raise Malformed("no mvex")
    for k, _, p, e in boxes(b, *mvex):
        if k == b"trex":
            if e - p < 24:
                raise Malformed("trex")
            if be(b, p + 4, 4) == t["track_id"]:
                t.update(trex_duration=be(b, p + 12, 4), trex_size=be(b, p + 16, 4), trex_flags=be(b, p + 20, 4))
                return t, nals
    raise Malformed("no trex for the track")
