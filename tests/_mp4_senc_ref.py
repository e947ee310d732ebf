"""hbs_mp4_senc_samples and hbs_mp4_init_unprotect_host restated in plain Python (include/hevcbitstream_amd.h is the
specification): the device call as one loop over the fragments that reads every senc serially, record behind record, and never
looks at a saiz; the host function as one walk down the boxes.  Also the writers of the hand-made fragments that the CPU and the
GPU tests share.  Test infrastructure: numpy and struct only, no GPU, nothing of the library, and nothing of the writer's
reference (tests/_mp4_protect_ref.py) in the reading direction."""
import struct

import numpy as np

from tests import _mp4_read_ref as RR
from tests import _mp4_ref as R

E_ARG, E_CAPACITY = -3, -4
M32 = (1 << 32) - 1
SUB_LIMIT = 1 << 48
CLEAR_IF_ABSENT = 1
SUBSAMPLE = np.dtype([("clear", "<u4"), ("protect", "<u4")])
PARAMS = np.dtype([("iv_size", "<u4"), ("track_id", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (5,))])
TENC = np.dtype([("scheme", "<u4"), ("crypt_byte_block", "u1"), ("skip_byte_block", "u1"), ("iv_size", "u1"), ("constant_iv_size", "u1"),
                 ("kid", "u1", (16,)), ("constant_iv", "u1", (16,)), ("reserved", "<u4", (6,))])
CENC, CBCS = 0x63656E63, 0x63626373

be = RR.be


def summary(error=0, entries=0, samples=0, protect=0, in_bytes=0, bad_sample=0, bad_frag=0, senc_read=0):
    return dict(error=error, nal_count=entries, nal_found=samples, rbsp_bytes=protect, stream_bytes=in_bytes, stop_reason=0,
                reserved=[bad_sample, bad_frag, senc_read])


def clear_entries(z):
    """hbs_cenc_subsamples' EMIT(z, 0)"""
    out = []
    while z > 65535:
        out.append((65535, 0))
        z -= 65535
    return out + [(z, 0)] if z else out


# ---- the device call ------------------------------------------------------------------------------------------------------------

class Bad(Exception):
    """a fragment error"""


def read_fragment(b, n, off, size, S, sizes, V, track_id, flags):
    """one fragment of S samples whose sizes are `sizes` (None: no d_sample_size) -> ([(iv 16 bytes, [(clear, protect)])], whether a
    senc was read, 1 + the first of its samples whose size cannot be an entry or 0); Bad for a fragment error"""
    if off + size > n:
        raise Bad("leaves the buffer")
    if S == 0:
        return [], False, 0
    try:
        (kind, _, pay, end), = RR.boxes(b, off, off + size)[:1]
        if kind != b"moof":
            raise Bad("no moof")
        chosen = None
        for k, _, p, e in RR.boxes(b, pay, end):
            if k == b"traf" and chosen is None:
                h, kids = RR.read_traf(b, p, e)
                if track_id in (0, h["track_id"]):
                    chosen = kids
    except RR.Malformed as x:
        raise Bad(str(x))
    if chosen is None:
        raise Bad("no traf of the track")
    senc = [k for k in chosen if k[0] == b"senc"]
    bad_sample = 0
    if not senc:
        if not flags & CLEAR_IF_ABSENT or sizes is None:
            raise Bad("no senc")
        for i, z in enumerate(sizes):
            if z > M32 and not bad_sample:
                bad_sample = i + 1
        return [(bytes(16), clear_entries(z) if z <= M32 else []) for z in sizes], False, bad_sample
    _, _, p, e = senc[0]
    if e - p < 8 or be(b, p, 4) not in (0, 2) or be(b, p + 4, 4) != S:
        raise Bad("senc header")
    subs, at, out = be(b, p, 4) == 2, p + 8, []
    if not subs and sizes is None:
        raise Bad("no d_sample_size")
    for i in range(S):                      # THE SERIAL WALK: sample i + 1 begins where sample i says it ends
        if e - at < V + (2 if subs else 0):
            raise Bad("sample %d leaves the senc" % i)
        iv = bytes(b[at:at + V]) + bytes(16 - V)
        at += V
        if subs:
            cnt = be(b, at, 2)
            at += 2
            if e - at < 6 * cnt:
                raise Bad("sample %d leaves the senc" % i)
            ent = [struct.unpack(">HI", b[at + 6 * j:at + 6 * j + 6]) for j in range(cnt)]
            at += 6 * cnt
        else:
            z = sizes[i]
            if z > M32 and not bad_sample:
                bad_sample = i + 1
            ent = [(0, z)] if 0 < z <= M32 else []
        out.append((iv, ent))
    return out, True, bad_sample


def senc_samples(data, frags, sizes, V, track_id=0, flags=0, sub_cap=None, in_bytes=None, n_samples=None):
    """-> (sub_first uint64 [N + 1], sub ndarray[SUBSAMPLE], iv uint8 [16 N], summary dict); on an error the first three are None.
    frags: ndarray[FRAG]; sizes: None or the samples' sizes; sub_cap None: plan only."""
    b = data if isinstance(data, (bytes, bytearray)) else np.asarray(data).tobytes()
    n = len(b) if in_bytes is None else in_bytes
    Rn = len(frags)
    Ss = frags["samples"].tolist() if Rn else []
    N = sum(Ss) if n_samples is None else n_samples
    sizes = None if sizes is None else [int(z) for z in sizes]
    offs, lens, firsts = (frags[k].tolist() for k in ("out_off", "out_bytes", "first_au")) if Rn else ([], [], [])
    fail = lambda **kw: (None, None, None, summary(samples=N, in_bytes=n, **kw))          # noqa: E731
    below, samples, read, bad_sample = 0, [], 0, 0
    for r in range(Rn):                     # ONE LOOP OVER THE FRAGMENTS
        S = Ss[r]
        numbered = (firsts[r] - firsts[0]) % (1 << 64) == below and below + S <= N and (r + 1 < Rn or below + S == N)
        try:
            got, was_read, bs = read_fragment(b, n, offs[r], lens[r], S, None if sizes is None or not numbered else sizes[below:below + S], V,
                                              track_id, flags)
        except Bad:
            return fail(error=E_ARG, bad_frag=r + 1)
        if not numbered:
            return fail(error=E_ARG, bad_frag=r + 1)
        if bs and not bad_sample:
            bad_sample = below + bs
        samples += got
        read += was_read
        below += S
    if bad_sample:
        return fail(error=E_ARG, bad_sample=bad_sample)
    first = np.zeros(N + 1, dtype=np.uint64)
    first[1:] = np.cumsum([len(e) for _, e in samples], dtype=np.uint64) if N else 0
    total = int(first[N])
    if total >= SUB_LIMIT:
        return fail(error=E_CAPACITY)
    sub = np.array([x for _, e in samples for x in e], dtype=SUBSAMPLE).reshape(-1)
    s = summary(0, total, N, int(sub["protect"].astype(np.uint64).sum()), n, senc_read=read)
    if sub_cap is not None and sub_cap < total:
        return None, None, None, dict(s, error=E_CAPACITY)
    iv = np.frombuffer(b"".join(i for i, _ in samples), dtype=np.uint8) if N else np.zeros(0, np.uint8)
    return first, sub, iv, s


# ---- hand-made fragments ----------------------------------------------------------------------------------------------------------

def senc_box(V, samples, flags=2, trailing=b"", version=0, count=None, **kw):
    """samples: [(iv bytes, [(clear, protect)])]"""
    p = struct.pack(">I", len(samples) if count is None else count)
    for iv, ent in samples:
        p += bytes(iv[:V])
        if flags & 2:
            p += struct.pack(">H", len(ent)) + b"".join(struct.pack(">HI", c, q) for c, q in ent)
    return RR.full(b"senc", version, flags, p + trailing, **kw)


def saiz_box(V, samples, typed=False, default=0, count=None, sizes=None):
    sizes = [V + 2 + 6 * len(e) for _, e in samples] if sizes is None else sizes
    p = (struct.pack(">II", CENC, 0) if typed else b"") + bytes([default]) + struct.pack(">I", len(samples) if count is None else count)
    return RR.full(b"saiz", 0, 1 if typed else 0, p + (b"" if default else bytes(sizes)))


def traf(track_id, sample_sizes, *extra, front=(), large=False):
    """tfhd, tfdt and a trun of these sizes with `extra` boxes behind the trun and `front` ones in front of it"""
    trun = RR.trun(0x201, [(0, z, 0, 0) for z in sample_sizes], data_offset=0)
    return RR.box(b"traf", RR.tfhd(track_id) + RR.tfdt(0) + b"".join(front) + trun + b"".join(extra), large=large)


def fragment(trafs, payload=b"", sequence=1):
    """moof (mfhd and the trafs) and an mdat"""
    return RR.box(b"moof", RR.mfhd(sequence) + b"".join(trafs)) + RR.box(b"mdat", payload)


def frag_table(blobs, counts, gap=0):
    """the fragments back to back (gap bytes of 0xEE in front of each) -> (bytes, ndarray[FRAG])"""
    fr = np.zeros(len(blobs), dtype=R.FRAG)
    out, s = b"", 0
    for r, (x, c) in enumerate(zip(blobs, counts)):
        out += b"\xEE" * gap
        fr[r]["out_off"], fr[r]["out_bytes"], fr[r]["first_au"], fr[r]["samples"], fr[r]["sequence"] = len(out), len(x), s, c, r + 1
        out += x
        s += c
    return out, fr


# ---- the init segment -------------------------------------------------------------------------------------------------------------

def box_at(b, lo, hi):
    """the one box at lo of a container that ends at hi -> (kind, begin, payload, end, header bytes); Malformed"""
    if hi - lo < 8:
        raise RR.Malformed("header leaves the container")
    size, kind, head = be(b, lo, 4), bytes(b[lo + 4:lo + 8]), 8
    if size == 1:
        if hi - lo < 16:
            raise RR.Malformed("largesize leaves the container")
        size, head = be(b, lo + 8, 8), 16
        if size < 16:
            raise RR.Malformed("largesize below 16")
    elif size == 0:
        size = hi - lo
    elif size < 8:
        raise RR.Malformed("size below 8")
    if size > hi - lo:
        raise RR.Malformed("box leaves the container")
    return kind, lo, lo + head, lo + size, head


def first_child(b, lo, hi, kind):
    """the first box of `kind`; what lies behind it is not looked at.  None: none, or a box in front of it is malformed"""
    try:
        while lo < hi:
            x = box_at(b, lo, hi)
            if x[0] == kind:
                return x
            lo = x[3]
    except RR.Malformed:
        pass
    return None


def whole_child(b, lo, hi, kind):
    """the first box of `kind` of a container all of whose boxes are well-formed -> (payload, end) or None"""
    try:
        for k, _, p, e in RR.boxes(b, lo, hi):
            if k == kind:
                return p, e
    except RR.Malformed:
        pass
    return None


def plain_size(b, x):
    """an 8-byte header whose size field is the box's size"""
    return x is not None and x[4] == 8 and be(b, x[1], 4) == x[3] - x[1]


def read_sinf(b, lo, hi):
    """-> (frma fourcc, tenc record) or None"""
    t = np.zeros(1, dtype=TENC)
    x = whole_child(b, lo, hi, b"frma")
    if x is None or x[1] - x[0] < 4 or bytes(b[x[0]:x[0] + 4]) not in (b"hvc1", b"hev1"):
        return None
    fmt = be(b, x[0], 4)
    x = whole_child(b, lo, hi, b"schm")
    if x is None or x[1] - x[0] < 8:
        return None
    t["scheme"] = be(b, x[0] + 4, 4)
    x = whole_child(b, lo, hi, b"schi")
    x = whole_child(b, *x, b"tenc") if x is not None else None
    if x is None or x[1] - x[0] < 24:
        return None
    a, z = x
    if b[a] > 1 or b[a + 6] != 1:
        return None
    if b[a] == 1:
        t["crypt_byte_block"], t["skip_byte_block"] = b[a + 5] >> 4, b[a + 5] & 15
    t["iv_size"] = b[a + 7]
    t["kid"][0] = np.frombuffer(bytes(b[a + 8:a + 24]), dtype=np.uint8)
    if b[a + 7] == 0:
        if z - a < 25 or b[a + 24] not in (8, 16) or z - a < 25 + b[a + 24]:
            return None
        t["constant_iv_size"] = b[a + 24]
        t["constant_iv"][0][:b[a + 24]] = np.frombuffer(bytes(b[a + 25:a + 25 + b[a + 24]]), dtype=np.uint8)
    c, k, V, scheme = int(t["crypt_byte_block"][0]), int(t["skip_byte_block"][0]), int(t["iv_size"][0]), int(t["scheme"][0])
    if scheme not in (CENC, CBCS) or (scheme == CENC and (c or k)) or V not in (0, 8, 16):
        return None
    return fmt, t


def init_unprotect(init, track_id=0):
    """-> (bytes, tenc ndarray[TENC] of one, frma fourcc, [(off, size)] of the moov's pssh boxes), or E_ARG"""
    b = bytes(init)
    moov = first_child(b, 0, len(b), b"moov")
    if not plain_size(b, moov):
        return E_ARG
    path, cuts, pssh, found = [moov], [], [], None
    try:
        kids = [box_at(b, at, moov[3]) for _, at, _, _ in RR.boxes(b, moov[2], moov[3])]
    except RR.Malformed:
        return E_ARG
    for x in kids:
        kind, at, pay, end, head = x
        if kind == b"pssh":
            cuts.append((at, end - at))
            pssh.append((at, end - at))
        elif kind == b"trak" and found is None and plain_size(b, x):
            tk = whole_child(b, pay, end, b"tkhd")
            if tk is None or tk[1] - tk[0] < 4 or b[tk[0]] > 1 or tk[1] - tk[0] < (96 if b[tk[0]] else 84):
                return E_ARG
            tid = be(b, tk[0] + (20 if b[tk[0]] else 12), 4)
            if track_id not in (0, tid):
                continue
            down, lo, hi = [x], pay, end
            for k in (b"mdia", b"minf", b"stbl", b"stsd"):
                y = first_child(b, lo, hi, k)
                if not plain_size(b, y):
                    down = None
                    break
                down.append(y)
                lo, hi = y[2], y[3]
            if down is None or hi - lo < 8:
                continue
            count, e = be(b, lo + 4, 4), lo + 8
            for _ in range(count):
                if e >= hi or found is not None:
                    break
                try:
                    y = box_at(b, e, hi)
                except RR.Malformed:
                    break
                if y[0] == b"encv" and plain_size(b, y) and y[3] - y[2] >= 78:
                    ca, ce = y[2] + 78, y[3]
                    sinf = first_child(b, ca, ce, b"sinf")
                    if whole_child(b, ca, ce, b"hvcC") is not None and sinf is not None:
                        got = read_sinf(b, sinf[2], sinf[3])
                        if got is not None:
                            found = (got, tid, sinf)
                            path += down + [y]
                            cuts.append((sinf[1], sinf[3] - sinf[1]))
                e = y[3]
    if found is None:
        return E_ARG
    (fmt, tenc), tid, sinf = found
    out, at = bytearray(), 0
    for c_at, c_n in cuts:
        out += b[at:c_at]
        at = c_at + c_n
    out += b[at:]
    sinf_n, pssh_n = sinf[3] - sinf[1], sum(z for _, z in pssh)
    for depth, x in enumerate(path):
        where = x[1] - sum(z for a, z in cuts if a < x[1])
        out[where:where + 4] = struct.pack(">I", x[3] - x[1] - sinf_n - (pssh_n if depth == 0 else 0))
        if depth == 6:
            out[where + 4:where + 8] = struct.pack(">I", fmt)
    try:
        if RR.init_read(bytes(out), tid)[0]["entry"] != fmt:
            return E_ARG
    except RR.Malformed:
        return E_ARG
    return bytes(out), tenc, fmt, pssh
