"""hbs_mp4_protect and hbs_mp4_init_protect_host restated in plain Python (include/hevcbitstream_amd.h is the specification): the
device call as one loop over the fragments and their samples, the host function as a walk down the boxes that hold the hvcC,
and a walker that knows nothing of the writer: it finds the auxiliary data of a protected fragment only through saio's offset
and saiz's sizes.  Test infrastructure: numpy and struct only, no GPU, nothing of the library."""
import struct

import numpy as np

from tests import _mp4_read_ref as RR
from tests import _mp4_ref as R

E_ARG, E_CAPACITY = -3, -4
M32 = (1 << 32) - 1
MOOF_MAX = (1 << 31) - 9
SUB_LIMIT = 1 << 48
SUBSAMPLE = np.dtype([("clear", "<u4"), ("protect", "<u4")])
PARAMS = np.dtype([("iv_size", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (6,))])
TENC = np.dtype([("scheme", "<u4"), ("crypt_byte_block", "u1"), ("skip_byte_block", "u1"), ("iv_size", "u1"), ("constant_iv_size", "u1"),
                 ("kid", "u1", (16,)), ("constant_iv", "u1", (16,)), ("reserved", "<u4", (6,))])
CENC, CBCS = 0x63656E63, 0x63626373


def growth(S, E, V):
    return 53 + (V + 3) * S + 6 * E


def moof_size(S, E, V):
    return 141 + (19 + V) * S + 6 * E


def max_entries(V):
    return (253 - V) // 6


def u32(b, at):
    return int.from_bytes(b[at:at + 4], "big")


def summary(error=0, frags=0, samples=0, entries=0, total=0, bad_sample=0, bad_frag=0):
    return dict(error=error, nal_count=frags, nal_found=samples, rbsp_bytes=entries, stream_bytes=total, stop_reason=0,
                reserved=[bad_sample, bad_frag, 0])


# ---- the device call ------------------------------------------------------------------------------------------------------------

def frag_ok(b, n, off, size, S):
    """the fragment rule but for the numbering: b[off, off + size) of a buffer of n bytes is a fragment of S samples in the form
    hbs_mp4_fragment states"""
    if off + size > n or S > R.SAMPLES_MAX:
        return False
    head = 88 + 16 * S
    if size < head + 8 or size - head > M32:
        return False
    tag = lambda at: bytes(b[off + at:off + at + 4])          # noqa: E731
    return (u32(b, off) == head and tag(4) == b"moof" and u32(b, off + 24) == 64 + 16 * S and tag(28) == b"traf" and tag(36) == b"tfhd"
            and tag(52) == b"tfdt" and u32(b, off + 68) == 20 + 16 * S and tag(72) == b"trun" and u32(b, off + 76) == 0x01000F01
            and u32(b, off + 80) == S and u32(b, off + 84) == 96 + 16 * S and u32(b, off + head) == size - head and tag(head + 4) == b"mdat")


def new_moof(head, V, counts, entries, ivs):
    """the moof of the protected fragment from the old one's bytes `head` (88 + 16 S of them) and, a sample, its entry count in
    counts, its entries [(clear, protect)] in order in `entries`, its 16 IV bytes in ivs"""
    S, E = len(counts), len(entries)
    M = moof_size(S, E, V)
    saiz = R.full(b"saiz", 0, 0, b"\0", struct.pack(">I", S), bytes(V + 2 + 6 * c for c in counts))
    saio = R.full(b"saio", 0, 0, struct.pack(">II", 1, 141 + 17 * S))
    aux, e = [], 0
    for i, c in enumerate(counts):
        aux.append(bytes(ivs[16 * i:16 * i + V]) + struct.pack(">H", c) + b"".join(struct.pack(">HI", a, p) for a, p in entries[e:e + c]))
        e += c
    senc = R.full(b"senc", 0, 2, struct.pack(">I", S), *aux)
    out = bytearray(head) + saiz + saio + senc
    assert len(out) == M and len(saiz) == 17 + S and len(saio) == 20 and len(senc) == 16 + (V + 2) * S + 6 * E
    out[0:4] = struct.pack(">I", M)
    out[24:28] = struct.pack(">I", M - 24)
    out[84:88] = struct.pack(">I", M + 8)
    return bytes(out)


def protect(data, frags, sub_first, sub, iv, V, out_cap=None, in_bytes=None, n_samples=None, build=True):
    """-> (output uint8 array, sample_off, sample_size, ndarray[FRAG], summary dict); on an error the first four are None.
    frags: ndarray[FRAG]; sub_first: uint64, n_samples + 1; sub: ndarray[SUBSAMPLE]; iv: 16 bytes a sample (None with V 0).
    build=False: everything but the output's bytes (None)."""
    b = data if isinstance(data, (bytes, bytearray)) else np.asarray(data).tobytes()
    n = len(b) if in_bytes is None else in_bytes
    sf = [int(x) for x in sub_first] if sub_first is not None else [0]
    N = len(sf) - 1 if n_samples is None else n_samples
    Rn = len(frags)
    fail = lambda s: (None, None, None, None, s)          # noqa: E731
    if Rn == 0:
        assert N == 0
        return np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, R.FRAG), summary()
    clear, prot = (sub["clear"].tolist(), sub["protect"].tolist()) if sub is not None else ([], [])
    ivb = bytes(np.asarray(iv, dtype=np.uint8)) if iv is not None else b""
    # the fragment rule, the numbering with it
    offs, sizes, Ss, firsts = frags["out_off"].tolist(), frags["out_bytes"].tolist(), frags["samples"].tolist(), frags["first_au"].tolist()
    bad_frag, below, first = 0, 0, []
    for r in range(Rn):
        numbered = (firsts[r] - firsts[0]) % (1 << 64) == below and below + Ss[r] <= N and (r + 1 < Rn or below + Ss[r] == N)
        if not (numbered and frag_ok(b, n, offs[r], sizes[r], Ss[r])) and not bad_frag:
            bad_frag = r + 1
        first.append(below)
        below += Ss[r]
    if bad_frag:
        return fail(summary(E_ARG, Rn, N, bad_frag=bad_frag))
    # the sample rule: what the tables say
    for s in range(N):
        ok = (s or sf[0] == 0) and sf[s] <= sf[s + 1] < SUB_LIMIT and sf[s + 1] - sf[s] <= max_entries(V)
        if ok and V == 8 and any(ivb[16 * s + 8:16 * s + 16]):
            ok = False
        if not ok:
            return fail(summary(E_ARG, Rn, N, bad_sample=s + 1))
    # ONE LOOP OVER THE FRAGMENTS AND THEIR SAMPLES: the entries against the trun's size words, the new bytes, the tables
    pieces, new_frags, sample_off, sample_size, at, big = [], [], [], [], 0, 0
    for r in range(Rn):
        off, S, s0 = offs[r], Ss[r], first[r]
        counts = [sf[s0 + i + 1] - sf[s0 + i] for i in range(S)]
        E = sum(counts)
        M = moof_size(S, E, V)
        body = at + M + 8
        for i in range(S):
            size = u32(b, off + 88 + 16 * i + 4)
            e0 = sf[s0 + i]
            if max(clear[e0:e0 + counts[i]], default=0) > 65535 or sum(clear[e0:e0 + counts[i]]) + sum(prot[e0:e0 + counts[i]]) != size:
                return fail(summary(E_ARG, Rn, N, bad_sample=s0 + i + 1))
            sample_off.append(body)
            sample_size.append(size)
            body += size
        if M > MOOF_MAX and not big:
            big = r + 1
        head = 88 + 16 * S
        if build and not big:
            e0 = sf[s0] if S else 0
            pieces.append(new_moof(b[off:off + head], V, counts, list(zip(clear[e0:e0 + E], prot[e0:e0 + E])), ivb[16 * s0:16 * (s0 + S)]))
            pieces.append(bytes(b[off + head:off + sizes[r]]))
        grown = sizes[r] + growth(S, E, V)
        new_frags.append((at, grown) + tuple(frags[r].tolist()[2:]))
        at += grown
    if big:
        return fail(summary(E_ARG, Rn, N, bad_frag=big))
    if sum(z >> 20 for z in sizes) + Rn >= 1 << 41:
        return fail(summary(E_CAPACITY, Rn, N))
    E_total = sf[N] if N else 0
    assert at == sum(sizes) + 53 * Rn + (V + 3) * N + 6 * E_total
    s = summary(0, Rn, N, E_total, at)
    if out_cap is not None and out_cap < at:
        return fail(dict(s, error=E_CAPACITY))
    out = np.frombuffer(b"".join(pieces), dtype=np.uint8) if build else None
    assert out is None or len(out) == at
    return out, np.array(sample_off, dtype=np.uint64), np.array(sample_size, dtype=np.uint64), np.array(new_frags, dtype=R.FRAG), s


# ---- the independent walker -----------------------------------------------------------------------------------------------------

def walk_protected(b, V):
    """b: protected fragments back to back.  -> [dict(off, bytes, samples=[(iv bytes, [(clear, protect)])])], a fragment each.
    The auxiliary data is found the way a player finds it: saio's one offset, from the moof's first byte, and saiz's sizes; that
    it lies in the senc, and that the senc says the same, is checked."""
    b = bytes(b)
    top = R.walk(b, 0, len(b))
    assert len(top) % 2 == 0 and all(k == (b"moof", b"mdat")[i % 2] for i, (k, _, _) in enumerate(top)), [k for k, _, _ in top]
    found = []
    for (_, mp, me), (_, dp, de) in zip(top[0::2], top[1::2]):
        moof_at = mp - 8
        t = R.tree(b, mp, me)
        assert sorted(t) == [b"mfhd", b"saio", b"saiz", b"senc", b"tfdt", b"tfhd", b"traf", b"trun"], sorted(t)
        tp, te = R.only(t, b"traf")
        assert [k for k, _, _ in R.walk(b, tp, te)] == [b"tfhd", b"tfdt", b"trun", b"saiz", b"saio", b"senc"]
        p, e = R.only(t, b"trun")
        count = u32(b, p + 4)
        assert moof_at + u32(b, p + 8) == dp, "data_offset does not land behind the mdat header"
        p, e = R.only(t, b"saiz")
        assert u32(b, p) == 0 and b[p + 4] == 0 and u32(b, p + 5) == count and e - p == 9 + count
        sizes = list(b[p + 9:e])
        p, e = R.only(t, b"saio")
        assert u32(b, p) == 0 and u32(b, p + 4) == 1 and e - p == 12
        at = moof_at + u32(b, p + 8)
        sp, se = R.only(t, b"senc")
        assert u32(b, sp) == 2 and u32(b, sp + 4) == count and at == sp + 8 and at + sum(sizes) == se
        samples = []
        for z in sizes:
            iv, n = b[at:at + V], int.from_bytes(b[at + V:at + V + 2], "big")
            assert z == V + 2 + 6 * n
            samples.append((iv, [struct.unpack(">HI", b[at + V + 2 + 6 * i:at + V + 8 + 6 * i]) for i in range(n)]))
            at += z
        found.append(dict(off=moof_at, bytes=de - moof_at, samples=samples))
    return found


# ---- the init segment -------------------------------------------------------------------------------------------------------------

def tenc_record(scheme=CENC, kid=bytes(16), iv_size=8, constant_iv=b"", crypt_byte_block=0, skip_byte_block=0):
    t = np.zeros(1, dtype=TENC)
    t["scheme"], t["crypt_byte_block"], t["skip_byte_block"], t["iv_size"], t["constant_iv_size"] = scheme, crypt_byte_block, skip_byte_block, iv_size, len(constant_iv)
    t["kid"][0] = np.frombuffer(bytes(kid), dtype=np.uint8)
    t["constant_iv"][0][:len(constant_iv)] = np.frombuffer(bytes(constant_iv), dtype=np.uint8)
    return t


def sinf(fourcc, t):
    t = t[0]
    c, k, V, cz = int(t["crypt_byte_block"]), int(t["skip_byte_block"]), int(t["iv_size"]), int(t["constant_iv_size"])
    pattern = bool(c or k)
    tenc = R.full(b"tenc", 1 if pattern else 0, 0, bytes([0, (c << 4 | k) if pattern else 0, 1, V]), bytes(t["kid"]),
                  bytes([cz]) + bytes(t["constant_iv"][:cz]) if V == 0 else b"")
    return R.box(b"sinf", R.box(b"frma", fourcc), R.full(b"schm", 0, 0, struct.pack(">II", int(t["scheme"]), 0x00010000)), R.box(b"schi", tenc))


def tenc_ok(t):
    t = t[0]
    c, k, V, cz = int(t["crypt_byte_block"]), int(t["skip_byte_block"]), int(t["iv_size"]), int(t["constant_iv_size"])
    if int(t["scheme"]) not in (CENC, CBCS) or c > 15 or k > 15 or (int(t["scheme"]) == CENC and (c or k)) or V not in (0, 8, 16):
        return False
    return (cz in (8, 16) if V == 0 else cz == 0) and not t["reserved"].any()


def init_protect(init, t, pssh=(), track_id=0):
    """-> bytes, or E_ARG"""
    b = bytes(init)
    if not tenc_ok(t):
        return E_ARG
    for x in pssh:
        if len(x) < 8 or u32(x, 0) != len(x) or bytes(x[4:8]) != b"pssh":
            return E_ARG
    extra = sum(len(x) for x in pssh)
    try:
        hvcc = RR.init_read(b, track_id)[0]["hvcc_off"]
        lo, hi, path = 0, len(b), []
        for depth in range(7):              # moov, trak, mdia, minf, stbl, stsd, the entry: the box that holds the hvcC
            if depth == 6:                  # (like the reader, the walk looks at nothing behind the stsd entry that it takes)
                kind, at, pay, end = next(x for x in RR.each_box(b, lo, hi) if x[1] <= hvcc < x[3])
            else:
                (kind, at, pay, end), = [x for x in RR.boxes(b, lo, hi) if x[1] <= hvcc < x[3]]
            if pay - at != 8 or u32(b, at) != end - at:
                return E_ARG
            path.append((kind, at, end))
            lo, hi = pay + (8 if depth == 5 else 0), end
    except RR.Malformed:
        return E_ARG
    assert [k for k, _, _ in path[:6]] == [b"moov", b"trak", b"mdia", b"minf", b"stbl", b"stsd"] and path[6][0] in (b"hvc1", b"hev1")
    box = sinf(path[6][0], t)
    if path[0][2] - path[0][1] + len(box) + extra > M32 or extra > M32:
        return E_ARG
    entry_end, moov_end = path[6][2], path[0][2]
    out = bytearray(b[:entry_end] + box + b[entry_end:moov_end] + b"".join(bytes(x) for x in pssh) + b[moov_end:])
    for depth, (kind, at, end) in enumerate(path):
        out[at:at + 4] = struct.pack(">I", end - at + len(box) + (extra if depth == 0 else 0))
    out[path[6][1] + 4:path[6][1] + 8] = b"encv"
    return bytes(out)
