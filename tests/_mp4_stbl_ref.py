"""hbs_mp4_stbl_samples and hbs_mp4_stbl_find_host restated in plain Python (include/hevcbitstream_amd.h is the specification): a
writer of progressive files (one moov whose stbl describes every sample, one mdat), a finder and a reader that know nothing of
the writer, written from the header's rules and not from the C, and random tracks.  Test infrastructure: numpy and struct only,
no GPU, nothing of the library."""
import struct

import numpy as np

from tests import _mp4_ref as R
from tests._mp4_read_ref import Malformed, be, boxes, stsd_entries

STBL = np.dtype([("stsz", "<u8", (2,)), ("stco", "<u8", (2,)), ("stsc", "<u8", (2,)), ("stts", "<u8", (2,)), ("ctts", "<u8", (2,)),
                 ("stss", "<u8", (2,)), ("flags", "<u4"), ("reserved0", "<u4"), ("file_bytes", "<u8"), ("reserved", "<u8", (2,))])
CO64 = 1
BOXES = ("stsz", "stco", "stsc", "stts", "ctts", "stss")          # the order of the table errors
E_ARG, E_CAPACITY = -3, -4
TIME_LIMIT = 1 << 62
M32 = (1 << 32) - 1
NON_SYNC = 0x00010000


# ---- the writer ---------------------------------------------------------------------------------------------------------------

def runs(values):
    """run-length encoding: [(count, value)]"""
    out = []
    for v in values:
        if out and out[-1][1] == v:
            out[-1][0] += 1
        else:
            out.append([1, v])
    return [(c, v) for c, v in out]


def p_stsz(sizes, constant=None, count=None, version=0):
    if constant is not None:
        return struct.pack(">III", version << 24, constant, len(sizes) if count is None else count)
    return struct.pack(">III", version << 24, 0, len(sizes) if count is None else count) + b"".join(struct.pack(">I", s) for s in sizes)


def p_stco(offsets, co64=False, count=None, version=0):
    return struct.pack(">II", version << 24, len(offsets) if count is None else count) + b"".join(struct.pack(">Q" if co64 else ">I", o) for o in offsets)


def p_stsc(entries, count=None, version=0):
    """entries: [(first_chunk, samples_per_chunk)]"""
    return struct.pack(">II", version << 24, len(entries) if count is None else count) + b"".join(struct.pack(">III", f, s, 1) for f, s in entries)


def p_pairs(entries, version=0, count=None, signed=False):
    """stts / ctts: [(sample_count, value)]"""
    return struct.pack(">II", version << 24, len(entries) if count is None else count) + b"".join(
        struct.pack(">Ii" if signed else ">II", c, v) for c, v in entries)


def p_stss(numbers, count=None, version=0):
    return struct.pack(">II", version << 24, len(numbers) if count is None else count) + b"".join(struct.pack(">I", x) for x in numbers)


def stsc_of(chunk_lens):
    """the stsc entries of chunks of these lengths"""
    out = []
    for i, n in enumerate(chunk_lens):
        if not out or out[-1][1] != n:
            out.append((i + 1, n))
    return out


def payloads(sizes, chunk_lens, chunk_offs, deltas, cts=None, sync=None, co64=False, constant=None, ctts_version=None):
    """the six payloads (None: no such box) of a track: sample sizes, samples per chunk, chunk offsets, a delta a sample, a
    composition offset a sample (None: no ctts), the 0-based sync samples (None: no stss)"""
    if ctts_version is None:
        ctts_version = 1 if cts is not None and min(cts, default=0) < 0 else 0
    return dict(stsz=p_stsz(sizes, constant), stco=p_stco(chunk_offs, co64), stsc=p_stsc(stsc_of(chunk_lens)), stts=p_pairs(runs(deltas)),
                ctts=None if cts is None else p_pairs(runs(cts), ctts_version, signed=ctts_version == 1),
                stss=None if sync is None else p_stss([s + 1 for s in sync]))


def layout(pay, lead=0, align=None, order=BOXES):
    """-> (buffer bytes, STBL record): the payloads one behind the other in `order`, `lead` junk bytes in front; with `align` every
    payload begins at an address that is `align` mod 16; the last payload ends on the buffer's last byte"""
    buf = bytearray(b"\xA5" * lead)
    rec = np.zeros(1, dtype=STBL)
    for name in order:
        if pay.get(name) is None:
            continue
        if align is not None:
            buf += b"\x5A" * ((align - len(buf)) % 16)
        rec[name][0] = (len(buf), len(pay[name]))
        buf += pay[name]
    return bytes(buf), rec


def progressive_file(samples, chunk_lens, deltas, cts=None, sync=None, nals=None, track_id=1, timescale=90000, length_size=4, co64=False,
                     constant=None, moov_first=True, gaps=0):
    """a whole file: ftyp, moov (with the hvcC of `nals`) and mdat, in either order; the chunks lie in the mdat in order with
    `gaps` junk bytes between them.  -> (bytes, [sample offset])"""
    assert sum(chunk_lens) == len(samples)
    sizes = [len(s) for s in samples]

    def moov_of(chunk_offs):
        pay = payloads(sizes, chunk_lens, chunk_offs, deltas, cts, sync, co64, constant)
        seg = R.init_segment(nals, track_id=track_id, timescale=timescale, length_size=length_size)
        assert not isinstance(seg, int)
        # the init segment's writer gives every box of the moov but the tables: its stbl is rebuilt around its stsd
        ftyp_end = be(seg, 0, 4)
        found = {}

        def descend(lo, hi, path):
            for k, s, p, e in boxes(seg, lo, hi):
                found[path + (k,)] = (s, p, e)
                if k in (b"moov", b"trak", b"mdia", b"minf", b"stbl"):
                    descend(p, e, path + (k,))
        descend(0, len(seg), ())
        trak, mdia, minf = (b"moov", b"trak"), (b"moov", b"trak", b"mdia"), (b"moov", b"trak", b"mdia", b"minf")
        s, p, e = found[minf + (b"stbl", b"stsd")]
        kinds = dict(stsz=b"stsz", stco=b"co64" if co64 else b"stco", stsc=b"stsc", stts=b"stts", ctts=b"ctts", stss=b"stss")
        stbl = R.box(b"stbl", seg[s:e], *[R.box(kinds[k], pay[k]) for k in ("stts", "ctts", "stss", "stsc", "stsz", "stco") if pay[k] is not None])

        def rebuild(path, inner_kind, inner):
            s, p, e = found[path]
            kids = b"".join(inner if k == inner_kind else seg[cs:ce] for k, cs, _, ce in boxes(seg, p, e))
            return R.box(path[-1], kids)
        new_minf = rebuild(minf, b"stbl", stbl)
        new_mdia = rebuild(mdia, b"minf", new_minf)
        new_trak = rebuild(trak, b"mdia", new_mdia)
        s, p, e = found[(b"moov",)]
        kids = b"".join(new_trak if k == b"trak" else b"" if k == b"mvex" else seg[cs:ce] for k, cs, _, ce in boxes(seg, p, e))
        return seg[:ftyp_end], R.box(b"moov", kids)

    ftyp, moov = moov_of([0] * len(chunk_lens))
    at = len(ftyp) + (len(moov) if moov_first else 0) + 8
    chunk_offs, sample_offs, body, k = [], [], bytearray(), 0
    for n in chunk_lens:
        body += b"\xEE" * gaps
        chunk_offs.append(at + len(body))
        for s in samples[k:k + n]:
            sample_offs.append(at + len(body))
            body += s
        k += n
    ftyp, moov2 = moov_of(chunk_offs)
    assert len(moov2) == len(moov)
    mdat = R.box(b"mdat", bytes(body))
    return (ftyp + moov2 + mdat if moov_first else ftyp + mdat + moov2), sample_offs


# ---- the finder ---------------------------------------------------------------------------------------------------------------

def walk(b, track_id=0):
    """the moov's trak that is asked for -> (dict of hbs_mp4_track's fields, [(off, size)] of the hvcC's NALs, the stbl's children
    (payload begin, end)); Malformed for what the calls refuse"""
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
                 height=be(b, tk[0] + (92 if v else 80), 4) >> 16, trex_duration=0, trex_size=0, trex_flags=0)
        mdia = child(p, e, b"mdia")
        if mdia is None:
            raise Malformed("no mdia")
        md = child(*mdia, b"mdhd")
        if md is None or md[1] - md[0] < 4 or b[md[0]] > 1 or md[1] - md[0] < (32 if b[md[0]] else 20):
            raise Malformed("mdhd")
        t["timescale"] = be(b, md[0] + (20 if b[md[0]] else 12), 4)
        minf = child(*mdia, b"minf")
        nals, stbl = None, None
        if minf is not None:
            stbl = child(*minf, b"stbl")
            if stbl is None:
                raise Malformed("no stbl")
            stsd = child(*stbl, b"stsd")
            if stsd is None or stsd[1] - stsd[0] < 8:
                raise Malformed("stsd")
            for k2, _, sp, se in stsd_entries(b, stsd[0], stsd[1], be(b, stsd[0] + 4, 4)):
                if k2 in (b"hvc1", b"hev1"):
                    if se - sp < 78:
                        raise Malformed("sample entry")
                    hv = child(sp + 78, se, b"hvcC")
                    if hv is not None:
                        nals = hvcc_nals(b, *hv)
                        t.update(entry=be(k2, 0, 4), length_size=(b[hv[0] + 21] & 3) + 1, hvcc_off=hv[0], hvcc_bytes=hv[1] - hv[0], n_nals=len(nals))
                        break
        if not (nals is not None if track_id == 0 else t["track_id"] == track_id):
            continue
        if nals is None:
            raise Malformed("the track has no hvcC")
        got = (t, nals, stbl)
    if got is None:
        raise Malformed("no such track")
    return got


def track_read(b, track_id=0):
    """hbs_mp4_track_read_host -> (dict of hbs_mp4_track's fields, the trex ones 0; [(off, size)] of the hvcC's NALs)"""
    return walk(b, track_id)[:2]


def find(b, base=0, track_id=0):
    """hbs_mp4_stbl_find_host -> STBL record; Malformed for what the call refuses"""
    b = bytes(b)
    got = walk(b, track_id)[2]
    rec = np.zeros(1, dtype=STBL)
    kinds = {b"stsz": "stsz", b"stco": "stco", b"co64": "stco", b"stsc": "stsc", b"stts": "stts", b"ctts": "ctts", b"stss": "stss"}
    for k, _, p, e in boxes(b, *got):
        name = kinds.get(k)
        if name is None or rec[name][0][1]:
            continue
        if e == p:
            raise Malformed("a table box without a payload")
        rec[name][0] = (p + base, e - p)
        if name == "stco":
            rec["flags"][0] = CO64 if k == b"co64" else 0
    if any(not rec[name][0][1] for name in ("stsz", "stco", "stsc", "stts")):
        raise Malformed("a required box is missing")
    return rec


def hvcc_nals(b, hp, he):
    if he - hp < 23 or b[hp] != 1:
        raise Malformed("hvcC")
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
    return nals


# ---- the reader ---------------------------------------------------------------------------------------------------------------

def summary(error=0, n=0, c=0, size=0, total=0, bad=(0, 0, 0)):
    return dict(error=error, nal_count=n, nal_found=c, rbsp_bytes=size, stream_bytes=total, stop_reason=0, reserved=list(bad))


def counted(b, fixed, entry, max_version=0):
    """the count of a payload whose fixed part has `fixed` bytes; None: the version or the length is wrong"""
    if len(b) < fixed or b[0] > max_version:
        return None
    count = be(b, fixed - 4, 4)
    return count if fixed + count * entry <= len(b) else None


def words(b, at, count, width=4):
    return np.frombuffer(b, dtype=">u%d" % width, count=count, offset=at).astype(np.uint64).tolist() if count else []


def read(data, rec, sample_cap=None, in_bytes=None, outputs=True):
    """-> (off, size, dts, pts, flags, summary dict): numpy arrays; None in their place on an error or without outputs"""
    data = bytes(data) if not isinstance(data, np.ndarray) else data.tobytes()
    total = len(data) if in_bytes is None else in_bytes
    rec = rec[0] if getattr(rec, "shape", ()) else rec
    limit = int(rec["file_bytes"]) or total
    co64 = bool(int(rec["flags"]) & CO64)
    pay = {}
    for name in BOXES:
        off, n = int(rec[name][0]), int(rec[name][1])
        pay[name] = data[off:off + n] if n else None
    none = (None,) * 5

    def table_error(name):
        return none + (summary(E_ARG, total=total, bad=(1 + BOXES.index(name), 0, 0)),)

    # stsz
    b = pay["stsz"]
    if len(b) < 12:
        return table_error("stsz")
    ssz = be(b, 4, 4)
    N = counted(b, 12, 0 if ssz else 4)
    if N is None:
        return table_error("stsz")
    # stco / co64
    b = pay["stco"]
    C = counted(b, 8, 8 if co64 else 4)
    if C is None:
        return table_error("stco")
    # stsc: the first_chunk rule, then whether the chunks hold N samples
    b = pay["stsc"]
    E = counted(b, 8, 12)
    if E is None:
        return table_error("stsc")
    w = words(b, 8, 3 * E)
    first_chunk, per_chunk = w[0::3], w[1::3]
    for e in range(E):
        if (first_chunk[e] != 1 if e == 0 else first_chunk[e] <= first_chunk[e - 1]) or first_chunk[e] > C:
            return table_error("stsc")
    run_chunks = [(first_chunk[e + 1] if e + 1 < E else C + 1) - first_chunk[e] for e in range(E)]
    if sum(n * s for n, s in zip(run_chunks, per_chunk)) < N:
        return table_error("stsc")
    # stts
    b = pay["stts"]
    T = counted(b, 8, 8)
    if T is None:
        return table_error("stts")
    w = words(b, 8, 2 * T)
    stts = list(zip(w[0::2], w[1::2]))
    if sum(c for c, _ in stts) < N:
        return table_error("stts")
    # ctts
    ctts = []
    if pay["ctts"] is not None:
        b = pay["ctts"]
        K = counted(b, 8, 8, max_version=1)
        if K is None:
            return table_error("ctts")
        w = words(b, 8, 2 * K)
        ctts = [(c, v - (1 << 32) if b[0] == 1 and v >= 1 << 31 else v) for c, v in zip(w[0::2], w[1::2])]
    # stss
    stss = None
    if pay["stss"] is not None:
        b = pay["stss"]
        S = counted(b, 8, 4)
        if S is None:
            return table_error("stss")
        stss = words(b, 8, S)
        if any(x == 0 or (i and stss[i - 1] >= x) for i, x in enumerate(stss)):
            return table_error("stss")
    if not outputs:
        size = N * ssz if ssz else sum(words(pay["stsz"], 12, N))
        return none + (summary(0, N, C, size, total),)
    if sample_cap is not None and N > sample_cap:
        return none + (summary(E_CAPACITY, N, C, 0, total),)
    # the samples, in table order
    sizes = [ssz] * N if ssz else words(pay["stsz"], 12, N)
    chunk_offs = words(pay["stco"], 8, C, 8 if co64 else 4)
    off = []
    for e in range(E):
        for c in range(run_chunks[e]):
            at = chunk_offs[first_chunk[e] - 1 + c]
            for _ in range(min(per_chunk[e], N - len(off))):
                off.append(at)
                at += sizes[len(off) - 1]
            if len(off) == N:
                break
        if len(off) == N:
            break
    dts, t = [], 0
    for c, d in stts:
        for _ in range(min(c, N - len(dts))):
            dts.append(t)
            t += d
        if len(dts) == N:
            break
    cts = []
    for c, v in ctts:
        cts += [v] * min(c, N - len(cts))
        if len(cts) == N:
            break
    cts += [0] * (N - len(cts))
    pts = [d + c for d, c in zip(dts, cts)]
    for s in range(N):
        if off[s] + sizes[s] > limit or dts[s] >= TIME_LIMIT or not 0 <= pts[s] < TIME_LIMIT:
            return none + (summary(E_ARG, N, C, 0, total, bad=(0, 0, s + 1)),)
    flags = np.zeros(N, dtype=np.uint32)
    if stss is not None:
        flags[:] = NON_SYNC
        flags[[x - 1 for x in stss if x <= N]] = 0
    u64 = lambda x: np.array(x, dtype=np.uint64)          # noqa: E731
    return u64(off), u64(sizes), u64(dts), u64(pts), flags, summary(0, N, C, sum(sizes), total)


# ---- random tracks ------------------------------------------------------------------------------------------------------------

def random_track(rng, n, max_size=40, max_chunk=7, reorder=True, constant=None):
    """-> dict(samples, chunk_lens, deltas, cts, sync): n samples of random bytes in chunks of uneven length (some chunks hold
    none), deltas and composition offsets in runs, some sync samples"""
    samples = [bytes(rng.integers(0, 256, size=constant if constant is not None else int(rng.integers(0, max_size + 1)), dtype=np.uint8)) for _ in range(n)]
    chunk_lens, left = [], n
    while left:
        c = int(rng.integers(0, max_chunk + 1))
        for _ in range(int(rng.integers(1, 4))):           # (runs of equal chunks, so that stsc has fewer entries than chunks)
            chunk_lens.append(min(c, left))
            left -= chunk_lens[-1]
            if not left:
                break
    deltas = []
    while len(deltas) < n:
        deltas += [int(rng.integers(0, 5000))] * int(rng.integers(1, 6))
    deltas = deltas[:n]
    cts = None
    if reorder:
        lead = 2 * max(deltas, default=0)
        cts = []
        while len(cts) < n:
            cts += [int(rng.integers(-lead, 3 * lead + 1))] * int(rng.integers(1, 4))
        cts = cts[:n]
        t = 0
        for i in range(n):                                 # (pts must not be negative)
            if t + cts[i] < 0:
                cts[i] = -t
            t += deltas[i]
    sync = sorted(set(int(x) for x in rng.integers(0, max(n, 1), size=max(n // 5, 1)))) if n else []
    return dict(samples=samples, chunk_lens=chunk_lens, deltas=deltas, cts=cts, sync=sync)
