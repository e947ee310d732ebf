"""hbs_mp4_stbl_write and hbs_mp4_moov_host restated in plain Python (include/hevcbitstream_amd.h is the specification): one loop
over the samples, exact integers, written from the header's rules and not from the C.  The payloads are packed by the p_*
packers of tests/_mp4_stbl_ref.py, which the reader's tests hold.  Test infrastructure: numpy and struct only, no GPU, nothing of
the library."""
import struct

import numpy as np

from tests import _mp4_ref as R
from tests import _mp4_stbl_ref as S

STBL = S.STBL
CO64 = S.CO64
E_ARG, E_CAPACITY = S.E_ARG, S.E_CAPACITY
LIMIT = 1 << 62
M32 = S.M32
NON_SYNC = S.NON_SYNC
ORDER = ("stts", "ctts", "stss", "stsc", "stsz", "stco")          # the output's order, and that of the box size error
PARAMS = np.dtype([("flags", "<u4"), ("max_chunk_samples", "<u4"), ("sample_duration", "<u4"), ("reserved0", "<u4"), ("base_time", "<u8"),
                   ("data_offset", "<u8")])


def summary(error=0, n=0, c=0, size=0, total=0, duration=0, bad_box=0, bad_sample=0):
    return dict(error=error, nal_count=n, nal_found=c, rbsp_bytes=size, stream_bytes=total, stop_reason=0, reserved=[bad_box, duration, bad_sample])


def box_bytes(name, entries, constant=False, co64=False):
    """the size of a box, header included"""
    per = dict(stts=8, ctts=8, stss=4, stsc=12, stsz=0 if constant else 4, stco=8 if co64 else 4)[name]
    return (20 if name == "stsz" else 16) + per * entries


def bytes_bound(n, with_ctts, with_stss, flags=0):
    """hbs_mp4_stbl_write_bytes_host"""
    if n > M32:
        return 0
    return sum(box_bytes(name, n, co64=bool(flags & CO64)) for name in ORDER if (name != "ctts" or with_ctts) and (name != "stss" or with_stss))


def write(off, size, dts=None, pts=None, flags=None, co64=False, max_chunk_samples=0, sample_duration=0, base_time=0, data_offset=0,
          out_cap=None, entries_override=None):
    """-> (blob or None, STBL record or None, summary dict).  The tables are sequences of ints (None: absent); out_cap None: plan
    only, which gives the blob all the same.  entries_override: box name -> entry count, for the box size rule alone."""
    N = len(size)
    off, size = [int(x) for x in off], [int(x) for x in size]
    dts = None if dts is None else [int(x) for x in dts]
    pts = None if pts is None else [int(x) for x in pts]
    chunk_first, deltas, cts, sync = [], [], [], []
    bad = None
    s = 0
    for k in range(N):
        wrong = False
        o = off[k] + data_offset
        if size[k] > M32 or o >= 1 << 64 or o + size[k] >= LIMIT:
            wrong = True
        contiguous = k > 0 and off[k] == off[k - 1] + size[k - 1]
        if not contiguous:
            s = k
        if k == s or (max_chunk_samples > 0 and (k - s) % max_chunk_samples == 0):
            chunk_first.append(k)
            if not co64 and o > M32:
                wrong = True
        t = dts[k] if dts is not None else base_time + k * sample_duration
        if t >= LIMIT:
            wrong = True
        d = sample_duration if dts is None or k == N - 1 else dts[k + 1] - t
        if not 0 <= d <= M32:
            wrong = True
        deltas.append(d)
        if pts is not None:
            c = pts[k] - t
            if pts[k] >= LIMIT or not -(1 << 31) <= c < 1 << 31:
                wrong = True
            cts.append(c)
        if flags is not None and not int(flags[k]) & NON_SYNC:
            sync.append(k)
        if wrong and bad is None:
            bad = k
    if bad is not None:
        return None, None, summary(E_ARG, N, bad_sample=bad + 1)
    chunk_lens = [(chunk_first[c + 1] if c + 1 < len(chunk_first) else N) - chunk_first[c] for c in range(len(chunk_first))]
    constant = size[0] if N > 0 and size[0] != 0 and all(z == size[0] for z in size) else None
    version = 1 if any(c < 0 for c in cts) else 0
    pay = dict(stts=S.p_pairs(S.runs(deltas)),
               ctts=None if pts is None else S.p_pairs(S.runs(cts), version, signed=version == 1),
               stss=None if flags is None else S.p_stss([k + 1 for k in sync]),
               stsc=S.p_stsc(S.stsc_of(chunk_lens)),
               stsz=S.p_stsz(size, constant),
               stco=S.p_stco([off[f] + data_offset for f in chunk_first], co64))
    kinds = dict(stts=b"stts", ctts=b"ctts", stss=b"stss", stsc=b"stsc", stsz=b"stsz", stco=b"co64" if co64 else b"stco")
    blob = bytearray()
    rec = np.zeros(1, dtype=STBL)
    for i, name in enumerate(ORDER):
        if pay[name] is None:
            continue
        n = 8 + len(pay[name])
        if entries_override and name in entries_override:
            n = box_bytes(name, entries_override[name], constant is not None, co64)
        if n > M32:
            return None, None, summary(E_ARG, N, bad_box=i + 1)
        rec[name][0] = (len(blob) + 8, len(pay[name]))
        blob += struct.pack(">I", n) + kinds[name] + pay[name]
    rec["flags"] = CO64 if co64 else 0
    s = summary(0, N, len(chunk_first), sum(size), len(blob), sum(deltas))
    if out_cap is not None and out_cap < len(blob):
        s["error"] = E_CAPACITY
        return None, None, s
    return bytes(blob), rec, s


def moov_prefix(nals, duration, tables_bytes, track_id=1, timescale=90000, width=1920, height=1080, length_size=4, chroma_format_idc=1,
                bit_depth_luma=8, bit_depth_chroma=8, flags=0):
    """hbs_mp4_moov_host -> bytes, or E_ARG: ftyp and the moov up to and including the stsd; the boxes that hold the stbl count
    tables_bytes more than they hold here"""
    nals = [bytes(x) for x in nals]
    if R.init_segment(nals, track_id, timescale, width, height, length_size, chroma_format_idc, bit_depth_luma, bit_depth_chroma, flags) == R.E_ARG:
        return E_ARG                                       # (everything hbs_mp4_init_host refuses)
    if not 0 <= duration <= M32 or tables_bytes % 4 or tables_bytes < 0:
        return E_ARG
    if tables_bytes:                                       # the moov's size has 32 bits
        bare = moov_prefix(nals, duration, 0, track_id, timescale, width, height, length_size, chroma_format_idc, bit_depth_luma, bit_depth_chroma, flags)
        if len(bare) - int.from_bytes(bare[:4], "big") + tables_bytes > M32:
            return E_ARG

    def open_box(kind, *payload):
        body = b"".join(payload)
        return struct.pack(">I", 8 + len(body) + tables_bytes) + kind + body

    hev1 = bool(flags & R.HEV1)
    pre = R.strip_epb([x for x in nals if (x[0] >> 1) & 0x3F == 33][0], 15)
    arrays = []
    for t in (32, 33, 34):
        of = [x for x in nals if (x[0] >> 1) & 0x3F == t]
        if of:
            arrays.append(struct.pack(">BH", (0 if hev1 else 0x80) | t, len(of)) + b"".join(struct.pack(">H", len(x)) + x for x in of))
    hvcc = R.box(b"hvcC", b"\x01", pre[3:15], b"\xF0\x00\xFC", bytes([0xFC | chroma_format_idc, 0xF8 | (bit_depth_luma - 8), 0xF8 | (bit_depth_chroma - 8)]),
                 b"\x00\x00", bytes([(((pre[2] >> 1) & 7) + 1) << 3 | (pre[2] & 1) << 2 | (length_size - 1), len(arrays)]), *arrays)
    matrix = struct.pack(">9I", 0x10000, 0, 0, 0, 0x10000, 0, 0, 0, 0x40000000)
    entry = R.box(b"hev1" if hev1 else b"hvc1", bytes(6), struct.pack(">H", 1), bytes(16), struct.pack(">HHIIIH", width, height, 0x480000, 0x480000, 0, 1),
                  bytes(32), struct.pack(">HH", 0x18, 0xFFFF), hvcc)
    stbl = open_box(b"stbl", R.full(b"stsd", 0, 0, struct.pack(">I", 1), entry))
    minf = open_box(b"minf", R.full(b"vmhd", 0, 1, bytes(8)), R.box(b"dinf", R.full(b"dref", 0, 0, struct.pack(">I", 1), R.full(b"url ", 0, 1))), stbl)
    mdia = open_box(b"mdia", R.full(b"mdhd", 0, 0, struct.pack(">IIIIHH", 0, 0, timescale, duration, 0x55C4, 0)),
                    R.full(b"hdlr", 0, 0, bytes(4), b"vide", bytes(12), b"VideoHandler\0"), minf)
    trak = open_box(b"trak", R.full(b"tkhd", 0, 3, struct.pack(">IIIII", 0, 0, track_id, 0, duration), bytes(8), bytes(8), matrix,
                                    struct.pack(">II", width << 16, height << 16)), mdia)
    mvhd = R.full(b"mvhd", 0, 0, struct.pack(">IIII", 0, 0, timescale, duration), struct.pack(">IH", 0x10000, 0x100), bytes(10), matrix, bytes(24),
                  struct.pack(">I", track_id + 1))
    if 8 + len(mvhd) + len(trak) + tables_bytes > M32:
        return E_ARG
    return R.box(b"ftyp", b"iso6", bytes(4), b"iso6", b"mp41") + open_box(b"moov", mvhd, trak)


def assemble(prefix, blob, body, moov_first):
    """the file: ftyp is the prefix's first box, the mdat header the caller's 8 bytes"""
    ftyp = int.from_bytes(prefix[:4], "big")
    mdat = struct.pack(">I", 8 + len(body)) + b"mdat" + bytes(body)
    return prefix + blob + mdat if moov_first else prefix[:ftyp] + mdat + prefix[ftyp:] + blob


# ---- case builders (the CPU reference test and the GPU test draw from the same) ---------------------------------------------------

def tables_of(sizes, chunk_lens, deltas, cts=None, sync=None, first=0, gap=3, dts0=0):
    """-> dict(off, size, dts, pts, flags): the samples of chunks of these lengths one behind the other, `gap` bytes apart (a gap
    of 0 joins chunks); dts from the deltas (the last delta is the call's sample_duration)"""
    assert sum(chunk_lens) == len(sizes) and all(chunk_lens)
    off, at, k = [], first, 0
    for c in chunk_lens:
        for z in sizes[k:k + c]:
            off.append(at)
            at += z
        at += gap
        k += c
    n = len(sizes)
    dts, t = [], dts0
    for d in deltas:
        dts.append(t)
        t += d
    pts = None if cts is None else [d + c for d, c in zip(dts, cts)]
    flags = None
    if sync is not None:
        flags = [0x01010000] * n
        for k in sync:
            flags[k] = 0x02000000
    return dict(off=off, size=list(sizes), dts=dts, pts=pts, flags=flags)


def random_tables(rng, n, **kw):
    """a random track of S.random_track without its empty chunks -> (tables, the track, its sample_duration)"""
    t = S.random_track(rng, n, **kw)
    t["chunk_lens"] = [c for c in t["chunk_lens"] if c]
    sizes = [len(x) for x in t["samples"]]
    return tables_of(sizes, t["chunk_lens"], t["deltas"], t["cts"], t["sync"]), t, (t["deltas"][-1] if n else 0)


W = 256                         # samples, chunks and runs of a workgroup (kSwLanes: hbs_mp4stblw.h)
PASS = 256 * 8                  # workgroups scan_parts takes in one pass (kPlanLanes * kPlanPer: hbs_plan.h)


def case(name, t, **params):
    """a call: the tables and the keyword arguments of write()"""
    params.setdefault("sample_duration", 0)
    return dict(name=name, t=t, params=params)


def call(c, **more):
    t = c["t"]
    return write(t["off"], t["size"], t["dts"], t["pts"], t["flags"], **dict(c["params"], **more))


def valid_cases():
    """the calls of tests/test_gpu_mp4_stbl_write.py that end without an error"""
    out = []
    rng = np.random.default_rng(2100)
    for n in (0, 1, W - 1, W, W + 1, 2 * W + 1):
        t, _, dur = random_tables(rng, n)
        out.append(case("random %d" % n, t, sample_duration=dur))

    def plain(n, chunk_lens, gap=3, sizes=None, deltas=None, cts="none", sync="none", **kw):
        sizes = [int(x) for x in rng.integers(1, 50, size=n)] if sizes is None else sizes
        deltas = [3000] * n if deltas is None else deltas
        return tables_of(sizes, chunk_lens, deltas, None if cts == "none" else cts, None if sync == "none" else sync, gap=gap, **kw)

    n = 3 * W + 1
    out.append(case("breaks on lanes 0 and 255", plain(n, [W - 1, 1, W - 1, 1 + W + 1]), sample_duration=3000))
    out.append(case("a chunk longer than two workgroups", plain(2 * W + 300, [100, 2 * W + 150, 50]), sample_duration=3000))
    out.append(case("every sample its own chunk", plain(W + 5, [1] * (W + 5)), sample_duration=3000))
    out.append(case("one chunk", plain(W + 5, [W + 5]), sample_duration=3000))
    for m in (1, 3, W, W + 1):
        stretches = [100, 3 * W + 7, 77, 2 * W]
        out.append(case("max_chunk_samples %d" % m, plain(sum(stretches), stretches), sample_duration=3000, max_chunk_samples=m))
    out.append(case("equal chunk lengths across a chunk workgroup's edge", plain(2 * 300 + 3 * 10, [2] * 300 + [3] * 10), sample_duration=3000))
    out.append(case("an stsc entry a chunk", plain(3 * 150, [1, 2] * 150), sample_duration=3000))
    n = 2 * W + 9
    out.append(case("stts and ctts of one entry", plain(n, [n], deltas=[40] * n, cts=[80] * n), sample_duration=40))
    alt, alt2 = [10 + (k & 1) for k in range(n)], [5 * (k & 1) for k in range(n)]
    out.append(case("stts and ctts of an entry a sample", plain(n, [n], deltas=alt, cts=alt2), sample_duration=alt[-1]))
    across = [5] * 200 + [7] * 200 + [5] * (n - 400)
    out.append(case("runs across a workgroup's edge", plain(n, [n], deltas=across, cts=[2 * x for x in across]), sample_duration=5))
    out.append(case("negative cts", plain(n, [n], deltas=[10] * n, cts=[-3 if k % 5 == 4 else 5 for k in range(n)], dts0=100), sample_duration=10))
    out.append(case("all cts 0", plain(n, [n], cts=[0] * n), sample_duration=3000))
    t = plain(n, [n])
    t["dts"] = None
    out.append(case("no d_dts", t, sample_duration=1001, base_time=90000))
    t = plain(n, [n])
    t["dts"], t["pts"] = None, [90000 + k * 1001 + (2002 if k % 3 else 0) for k in range(n)]
    out.append(case("no d_dts, with d_pts", t, sample_duration=1001, base_time=90000))
    for kind, sync in (("none", []), ("all", list(range(n))), ("every 32nd", list(range(0, n, 32))), ("absent", "none")):
        out.append(case("stss " + kind, plain(n, [100, n - 100], sync=sync), sample_duration=3000))
    out.append(case("constant sizes", plain(n, [n], sizes=[33] * n), sample_duration=3000))
    out.append(case("all sizes 0", plain(n, [7, n - 7], sizes=[0] * n), sample_duration=3000))
    out.append(case("all sizes equal but one", plain(n, [n], sizes=[33] * (n - 2) + [34, 33]), sample_duration=3000))
    out.append(case("co64 above 4 GiB", plain(n, [50, n - 50], first=5 << 32), sample_duration=3000, co64=True))
    out.append(case("data_offset", plain(n, [50, n - 50]), sample_duration=3000, data_offset=123456))
    out.append(case("a chunk that crosses 4 GiB", plain(n, [n], first=(1 << 32) - 1000), sample_duration=3000))
    out.append(case("co64 by data_offset", plain(n, [50, n - 50]), sample_duration=3000, data_offset=(1 << 40) + 4, co64=True))
    # more sample workgroups, and more chunk workgroups, than one scan pass takes
    n = PASS * W + 1
    t = dict(off=list(range(0, 9 * n, 9)), size=[8 - (k & 1) for k in range(n)], dts=None, pts=None, flags=None)
    out.append(case("more workgroups than one scan pass", t, sample_duration=512, base_time=7))
    return out


def error_cases():
    """[(case, the sample the error is reported at)]: every sample error, once in the first workgroup and once beyond it"""
    out = []
    n = 2 * W + 3
    rng = np.random.default_rng(2101)
    for p in (100, W + 100):
        def base(dts0=0):
            sizes = [int(x) for x in rng.integers(1, 50, size=n)]
            return tables_of(sizes, [60, n - 60], [10] * n, [20] * n, list(range(0, n, 7)), dts0=dts0)
        t = base()
        t["size"][p] = 1 << 32
        out.append((case("a size above 2^32 - 1", t, sample_duration=10), p))
        t = base()
        t["off"][p] = (1 << 64) - 8
        out.append((case("an offset that wraps", t, sample_duration=10, data_offset=16), p))
        t = base()
        t["off"][p] = (1 << 62) - 1
        t["size"][p] = 1
        out.append((case("a sample that ends at 2^62", t, sample_duration=10, co64=True), p))
        t = base()
        t["off"] = [o + (1 << 32) if k >= p else o for k, o in enumerate(t["off"])]
        out.append((case("a chunk offset above 2^32 - 1 in a stco", t, sample_duration=10), p))
        t = base(dts0=(1 << 62) - 10 * p)
        t["pts"] = None
        out.append((case("a dts of 2^62", t, sample_duration=10), p))
        t = base()
        t["dts"][p + 1] = t["dts"][p] - 1
        out.append((case("a negative delta", t, sample_duration=10), p))
        t = base()
        t["dts"] = [d + (1 << 32) if k > p else d for k, d in enumerate(t["dts"])]
        t["pts"] = None
        out.append((case("a delta above 2^32 - 1", t, sample_duration=10), p))
        t = base()
        t["pts"][p] = 1 << 62
        out.append((case("a pts of 2^62", t, sample_duration=10), p))
        t = base()
        t["pts"][p] = t["dts"][p] + (1 << 31)
        out.append((case("a cts of 2^31", t, sample_duration=10), p))
        t = base(dts0=1 << 32)
        t["pts"][p] = t["dts"][p] - (1 << 31) - 1
        out.append((case("a cts below -2^31", t, sample_duration=10), p))
        t = base()
        t["size"][p + 50] = 1 << 33
        t["pts"][p] = 1 << 62
        t["dts"][p + 9] = 1 << 62
        out.append((case("three bad samples", t, sample_duration=10), p))
    return out
