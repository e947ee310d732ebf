"""hbs_cenc_subsamples and hbs_cenc_crypt on the GPU against tests/_cenc_ref.py.  Every crypt case compares every byte of the
buffer with the reference -- the canary bytes between and around the samples included -- and every summary field; no
tolerances.  The crypt kernel takes 64 KiB of protected bytes a workgroup and walks the entries 256 a step in 1 024 ranges
(kCencTileBytes, kCencRanges: hbs_cenc.h); the plan takes 2 048 NALs a workgroup."""
import numpy as np
import pytest

from tests import _carve as K
from tests import _cenc_ref as R

pytestmark = pytest.mark.gpu
CAN = 0xC3
RANGES, STEP, TILE = 1024, 256, 64 * 1024
H = bytes.fromhex
KEY_38A = H("2b7e151628aed2a6abf7158809cf4f3c")
STRADDLE = [(5, 7), (3, 30), (0, 1), (65535, 0), (2, 11), (0, 0), (1, 16)]
NAL_ENTRY = np.dtype([("start", "<u8"), ("end", "<u8"), ("rbsp_off", "<u8"), ("rbsp_len", "<u4"), ("status", "<i4")])


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).cuda() if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")


def fresh_summary():
    import torch
    from hevcbitstream_amd.api import SUMMARY
    return torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")


def summary_dict(s):
    return dict(error=int(s["error"]), nal_count=int(s["nal_count"]), nal_found=int(s["nal_found"]), rbsp_bytes=int(s["rbsp_bytes"]),
                stream_bytes=int(s["stream_bytes"]), stop_reason=int(s["stop_reason"]), reserved=[int(x) for x in s["reserved"]])


def summary_matches(s, want):
    """every field the reference gives: under HBS_E_ARG hbs_cenc_subsamples' "counts mean nothing", and the reference leaves them out
    (a None in its reserved[])"""
    got = summary_dict(s)
    for k, v in want.items():
        if k == "reserved":
            assert all(x is None or g == x for g, x in zip(got[k], v)), (got, want)
        else:
            assert got[k] == v, (k, got, want)


def layout(entries_per_sample, gaps, lead=0):
    """samples laid one behind the other with `gaps` bytes between them -> (data_bytes, off, size, first, sub)"""
    off, size, first, subs, at = [], [], [0], [], lead
    for e, gap in zip(entries_per_sample, gaps):
        z = sum(a + b for a, b in e)
        off.append(at)
        size.append(z)
        subs += list(e)
        first.append(len(subs))
        at += z + gap
    return (at, np.array(off, dtype=np.uint64), np.array(size, dtype=np.uint64), np.array(first, dtype=np.uint64),
            np.array(subs, dtype=R.SUBSAMPLE).reshape(-1))


class Crypt:
    """one set of device buffers for hbs_cenc_crypt (the call wants d_data itself aligned: the samples' offsets carry the odd
    addresses), and the reference's answer for them"""

    def __init__(self, data, off, size, first, sub, key, iv=None, iv0=None, mode=None, scheme=R.SCHEME_CENC):
        import hevcbitstream_amd as hbs
        import torch
        self.host = (np.array(data, dtype=np.uint8), off, size, first, sub)
        self.key, self.iv, self.iv0 = key, iv, iv0
        self.n = len(off)
        self.d_data = dev(self.host[0])
        self.d_off, self.d_size, self.d_first, self.d_sub = dev(off), dev(size), dev(first), dev(sub)
        self.d_iv = dev(iv) if iv is not None else torch.full((max(self.n, 1) * 16,), CAN, dtype=torch.uint8, device="cuda")
        self.prm = hbs.cenc_params(key, iv0=iv0, iv_mode=mode, scheme=scheme)
        self.summary = fresh_summary()

    def launch(self, ctx, iv="own"):
        return ctx.cenc_crypt_async(self.d_data, len(self.host[0]), self.d_off, self.d_size, self.n, self.d_first, self.d_sub,
                                    self.d_iv if iv == "own" else iv, self.prm, self.summary)

    def data(self):
        return self.d_data[: len(self.host[0])].cpu().numpy()

    def want(self, data=None):
        data, off, size, first, sub = (self.host[0] if data is None else data,) + self.host[1:]
        return R.crypt(data, off, size, first, sub, self.key, iv=self.iv, iv0=self.iv0 if self.iv is None else None)

    def check(self, ctx, before=None):
        """the buffer and the summary behind one successful call on `before` (default: what was uploaded)"""
        want, done, used = self.want(before)
        assert summary_dict(ctx.read_summary(self.summary)) == dict(error=0, nal_count=len(self.host[4]), nal_found=self.n, rbsp_bytes=done,
                                                                    stream_bytes=len(self.host[0]), stop_reason=0, reserved=[0, 0, 0])
        got = self.data()
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        return want, used


# ---- known answers -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,ctr,nbytes,expect", (
    (bytes(range(16)), H("00112233445566778899aabbccddeeff"), 32, "69c4e0d86a7b0430d8cdb78070b4c55a"),
    (KEY_38A, H("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff"), 64, "874d6191b620e3261bef6864990db6ce" "9806f66b7970fdff8617187bb9fffdff"
                                                         "5ae4df3edbd5d35e5b4f09020db03eab" "1e031dda2fbe03d1792170a0f3009cee"),
    (KEY_38A, H("00000000000000" "01" + "ff" * 8), 32, "9e582c699ddc0085c0d36b60e14c06d0" "dc0a3bc38609c26f6f2a63a39cf7ee93")), ids=("fips197", "sp800-38a", "no-carry"))
def test_known_answers(ctx, key, ctr, nbytes, expect):
    plain = np.frombuffer(H("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51" "30c81c46a35ce411e5fbc1191a0a52ef"
                            "f69f2445df4f9b17ad2b417be66c3710"), dtype=np.uint8) if nbytes == 64 else np.zeros(nbytes, dtype=np.uint8)
    n, off, size, first, sub = layout([[(0, nbytes)]], [48], lead=48)
    data = np.full(n, CAN, dtype=np.uint8)
    data[48:48 + nbytes] = plain
    c = Crypt(data, off, size, first, sub, key, iv=np.frombuffer(ctr, dtype=np.uint8))
    assert c.launch(ctx) == 0
    got, _ = c.check(ctx)
    assert bytes(got[48:48 + len(expect) // 2]).hex() == expect
    assert (got[:48] == CAN).all() and (got[48 + nbytes:] == CAN).all()


# ---- straddling and splits -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", range(16))
def test_keystream_straddles_entries_at_every_offset(ctx, shift):
    rng = np.random.default_rng(100 + shift)
    n, off, size, first, sub = layout([STRADDLE], [40], lead=32 + shift)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    c = Crypt(data, off, size, first, sub, bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv=rng.integers(0, 256, 16, dtype=np.uint8))
    assert c.launch(ctx) == 0
    got, _ = c.check(ctx)
    # the bytes next to every protected range, by hand: the ranges of STRADDLE begin at these offsets of the sample
    p, ranges = int(off[0]), []
    for clear, protect in STRADDLE:
        p += clear
        ranges.append((p, p + protect))
        p += protect
    assert [b - a for a, b in ranges] == [7, 30, 1, 0, 11, 0, 16]
    inside = np.zeros(n, dtype=bool)
    for a, b in ranges:
        inside[a:b] = True
    assert inside.sum() == 65 and np.array_equal(got[~inside], data[~inside])
    ks = R.keystream(c.key, bytes(c.iv), 65)
    assert np.array_equal(got[inside], data[inside] ^ ks)          # one keystream, no byte of it skipped


# ---- scale ---------------------------------------------------------------------------------------------------------------------

def scale_case():
    rng = np.random.default_rng(4242)
    entries = []
    for _ in range(3000):
        k, left, e = int(rng.integers(0, 7)), int(rng.integers(0, 601)), []
        for i in range(k):
            a = int(rng.integers(0, left + 1)) if i + 1 < k else left
            c = int(rng.integers(0, a + 1)) if rng.integers(0, 4) else a
            e.append((c, a - c))
            left -= a
        entries.append(e)
    entries.insert(1500, [(9, 3 * (1 << 20) + 5)])
    entries.insert(2200, [(int(rng.integers(0, 9)), int(rng.integers(0, 40))) for _ in range(5000)])
    gaps = rng.integers(0, 50, len(entries)).tolist()
    n, off, size, first, sub = layout(entries, gaps, lead=int(rng.integers(1, 30)))
    if (int(off[1500]) + 9) % 2 == 0:                       # the large range starts at an odd address
        off[1500:] += np.uint64(1)
        n += 1
    return n, off, size, first, sub, rng


def test_scale_and_the_same_call_again_restores(ctx):
    n, off, size, first, sub, rng = scale_case()
    assert (int(off[1500]) + 9) % 2 == 1 and len(sub) > 8000
    data = rng.integers(0, 256, n, dtype=np.uint8)
    c = Crypt(data, off, size, first, sub, bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv=rng.integers(0, 256, 16 * len(off), dtype=np.uint8))
    assert c.launch(ctx) == 0
    got, _ = c.check(ctx)
    assert not np.array_equal(got, data)
    c.summary.fill_(0x5A)
    assert c.launch(ctx) == 0
    c.check(ctx, before=got)
    assert np.array_equal(c.data(), data)


# ---- sequential IVs ------------------------------------------------------------------------------------------------------------

def test_sequential_ivs_wrap_and_d_iv_is_optional(ctx):
    rng = np.random.default_rng(77)
    n, off, size, first, sub = layout([[(3, 40)], [(0, 17), (5, 0)], [(1, 33)], [], [(2, 64)]], [5, 0, 9, 3, 11], lead=7)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    iv0 = H("ff" * 7 + "fe") + H("1234567890abcdef")
    c = Crypt(data, off, size, first, sub, bytes(range(16)), iv0=iv0)
    assert c.launch(ctx) == 0
    got, used = c.check(ctx)
    assert bytes(used[2]) == bytes(16) and bytes(used[1]) == H("ff" * 8) + bytes(8)
    assert np.array_equal(c.d_iv.cpu().numpy()[: 16 * 5].reshape(5, 16), used)
    d = Crypt(data, off, size, first, sub, bytes(range(16)), iv0=iv0)
    assert d.launch(ctx, iv=None) == 0
    d.check(ctx)
    assert (d.d_iv.cpu().numpy() == CAN).all()


# ---- each error alone ----------------------------------------------------------------------------------------------------------

def error_base():
    rng = np.random.default_rng(31)
    entries = [[(int(rng.integers(0, 20)), int(rng.integers(1, 50))) for _ in range(int(rng.integers(1, 5)))] for _ in range(600)]
    n, off, size, first, sub = layout(entries, rng.integers(1, 9, 600).tolist(), lead=3)
    return dict(data=rng.integers(0, 256, n, dtype=np.uint8), off=off, size=size, first=first, sub=sub, key=bytes(range(16)),
                iv=rng.integers(0, 256, 16 * 600, dtype=np.uint8))


@pytest.mark.parametrize("what", ("short", "overlap", "past", "clear"))
def test_each_error_alone(ctx, what):
    b = error_base()
    j = 311
    if what == "short":
        b["size"][j] += 1                                   # (the gap behind it is at least one byte)
    elif what == "overlap":
        b["off"][j + 1] = b["off"][j] + b["size"][j] - np.uint64(1)
    elif what == "past":
        j = 599
        b["data"] = b["data"][: int(b["off"][j] + b["size"][j]) - 1]
    else:
        e = int(b["first"][j])
        b["size"][j] += np.uint64(65536 - int(b["sub"]["clear"][e]))
        b["off"][j + 1:] += np.uint64(65536)
        b["data"] = np.concatenate([b["data"], np.zeros(65536, dtype=np.uint8)])
        b["sub"]["clear"][e] = 65536
    assert R.crypt_check(len(b["data"]), b["off"], b["size"], b["first"], b["sub"]) == j + 1
    c = Crypt(**b)
    assert c.launch(ctx) == 0
    assert summary_dict(ctx.read_summary(c.summary)) == dict(error=R.E_ARG, nal_count=0, nal_found=600, rbsp_bytes=0, stream_bytes=len(b["data"]),
                                                             stop_reason=0, reserved=[j + 1, 0, 0])
    assert np.array_equal(c.data(), b["data"])


def test_refused_at_once_and_no_samples(ctx):
    import torch
    b = error_base()
    c = Crypt(scheme=0x63626373, **b)                       # 'cbcs'
    assert c.launch(ctx) == R.E_ARG
    odd = torch.zeros(16 * 600 + 16, dtype=torch.uint8, device="cuda")[1:]
    d = Crypt(**b)
    assert d.launch(ctx, iv=odd) == R.E_ARG
    assert d.launch(ctx, iv=None) == R.E_ARG                # iv_mode 0 reads d_iv
    for x in (c, d):
        assert (x.summary.cpu().numpy() == 0x5A).all() and np.array_equal(x.data(), b["data"])
    e = Crypt(b["data"], b["off"][:0], b["size"][:0], b["first"][:1], b["sub"][:0], b["key"], iv0=bytes(8))
    assert e.launch(ctx) == 0
    assert summary_dict(ctx.read_summary(e.summary)) == dict(error=0, nal_count=0, nal_found=0, rbsp_bytes=0, stream_bytes=len(b["data"]),
                                                             stop_reason=0, reserved=[0, 0, 0])
    assert np.array_equal(e.data(), b["data"])


# ---- hbs_cenc_subsamples -------------------------------------------------------------------------------------------------------

def build_stream(seed, L, n_nals=400, n_aus=None):
    """a few hundred small NALs of types 1, 19, 32..34, 39, 35 behind 3-byte gaps, AUs with nothing kept, and for L = 4 a 70 000-byte
    and a 131 070-byte SEI in front of a slice -> dict(stream, starts, ends, nal_au, n_aus, keep, payload_off)"""
    rng = np.random.default_rng(seed)
    types = rng.choice([1, 19, 32, 33, 34, 39, 35], n_nals)
    sizes = rng.integers(0, 90 if L > 1 else 60, n_nals)
    keep = (rng.integers(0, 5, n_nals) > 0).astype(np.uint8)
    big = ((50, 70000), (200, 131070 - 4)) if L == 4 else ()
    for k, z in big:                                       # an SEI, then a slice of the same AU
        types[k], sizes[k], keep[k] = 39, z, 1
        types[k + 1], sizes[k + 1], keep[k + 1] = 1, 50, 1
    # the AU number rises by one in front of n_aus - 1 of the NALs (never between an SEI above and its slice)
    n_aus = n_nals // 2 if n_aus is None else n_aus
    inc = np.zeros(n_nals, dtype=np.uint32)
    inc[rng.permutation([k for k in range(1, n_nals) if k - 1 not in [b for b, _ in big]])[: n_aus - 1]] = 1
    nal_au = (np.cumsum(inc) + 3).astype(np.uint32)
    sizes[(types < 32) & (sizes == 1)] = 2
    for a in (nal_au[30], nal_au[120]):                    # AUs with nothing kept
        keep[nal_au == a] = 0
    starts = np.cumsum(sizes + 3) - sizes
    ends = starts + sizes
    stream = rng.integers(0, 256, int(ends[-1]) + 9, dtype=np.uint8)
    for k in range(n_nals):
        if sizes[k]:
            stream[starts[k]] = (types[k] << 1) | (stream[starts[k]] & 0x81)
    po = np.full(n_nals, R.M64, dtype=np.uint64)
    for k in range(n_nals):
        if types[k] < 32 and sizes[k] >= 2:
            po[k] = starts[k] + rng.integers(2, sizes[k] + 1)
    return dict(stream=stream, starts=starts.astype(np.uint64), ends=ends.astype(np.uint64), nal_au=nal_au, n_aus=n_aus,
                keep=keep, payload_off=po)


class Plan:
    def __init__(self, st, L, flags, clear_lead, with_off):
        import hevcbitstream_amd as hbs
        import torch
        self.st, self.L, self.flags, self.lead = st, L, flags, clear_lead
        n = len(st["starts"])
        idx = np.zeros(n, dtype=NAL_ENTRY)
        idx["start"], idx["end"] = st["starts"], st["ends"]
        self.d_stream, self.d_idx, self.d_au, self.d_keep = dev(st["stream"]), dev(idx), dev(st["nal_au"]), dev(st["keep"])
        self.d_po = dev(st["payload_off"]) if with_off else None
        self.prm = hbs.cenc_plan_params(length_size=L, flags=flags, clear_lead=clear_lead)
        self.d_first = torch.full(((st["n_aus"] + 1) * 8 + 64,), CAN, dtype=torch.uint8, device="cuda")
        self.summary = fresh_summary()

    def launch(self, ctx, sub, cap=None):
        st = self.st
        return ctx.cenc_subsamples_async(self.d_stream, len(st["stream"]), self.d_idx, len(st["starts"]), self.d_au, st["n_aus"], self.prm, self.d_first,
                                         sub, self.summary, keep=self.d_keep, payload_off=self.d_po, sub_cap=cap)

    def want(self, sub_cap=None):
        st = self.st
        return R.subsamples(st["stream"], st["starts"].astype(np.int64), st["ends"].astype(np.int64), st["nal_au"], st["n_aus"], self.L, keep=st["keep"],
                            payload_off=st["payload_off"] if self.d_po is not None else None, flags=self.flags, clear_lead=self.lead, sub_cap=sub_cap)

    def summary_of(self, w):
        return dict(error=w["error"], nal_count=len(w["sub"]), nal_found=len(self.st["starts"]), rbsp_bytes=w["protected"], stream_bytes=w["sample_bytes"],
                    stop_reason=0, reserved=[0, 0, w["kept"]])


@pytest.mark.parametrize("with_off,clear_lead", ((True, 96), (False, 2), (False, 96)), ids=("payload_off", "lead2", "lead96"))
@pytest.mark.parametrize("flags", (0, R.ALIGN16), ids=("bytes", "align16"))
@pytest.mark.parametrize("L", (1, 2, 4))
def test_subsamples_against_the_reference(ctx, L, flags, with_off, clear_lead):
    import torch
    p = Plan(build_stream(500 + L, L), L, flags, clear_lead, with_off)
    w = p.want()
    assert w["error"] == 0 and len(w["sub"]) > 50 and (np.diff(w["sub_first"].astype(np.int64)) == 0).sum() >= 2
    if L == 4:
        assert (w["sub"]["clear"] == 65535).sum() >= 3
    total = len(w["sub"])
    # plan only: the counts and d_sub_first
    assert p.launch(ctx, None) == 0
    assert summary_dict(ctx.read_summary(p.summary)) == p.summary_of(w)
    first = p.d_first.cpu().numpy()
    assert np.array_equal(first[: 8 * len(w["sub_first"])].view(np.uint64), w["sub_first"]) and (first[8 * len(w["sub_first"]):] == CAN).all()
    # one entry short: the counts are right, nothing else is written
    sub = torch.full((total * 8 + 64,), CAN, dtype=torch.uint8, device="cuda")
    p.d_first.fill_(CAN)
    assert p.launch(ctx, sub, cap=total - 1) == 0
    assert summary_dict(ctx.read_summary(p.summary)) == p.summary_of(p.want(sub_cap=total - 1)) and p.want(sub_cap=total - 1)["error"] == R.E_CAPACITY
    assert (sub.cpu().numpy() == CAN).all() and (p.d_first.cpu().numpy() == CAN).all()
    # the table
    assert p.launch(ctx, sub, cap=total) == 0
    assert summary_dict(ctx.read_summary(p.summary)) == p.summary_of(w)
    got = sub.cpu().numpy()
    assert np.array_equal(got[: 8 * total].view(R.SUBSAMPLE), w["sub"]) and (got[8 * total:] == CAN).all()
    assert np.array_equal(p.d_first.cpu().numpy()[: 8 * len(w["sub_first"])].view(np.uint64), w["sub_first"])


@pytest.mark.parametrize("value", ("none", "start+1", "end+1"))
def test_a_slice_the_parse_did_not_read_is_an_error(ctx, value):
    import torch
    st = build_stream(900, 4)
    k = [i for i in range(len(st["starts"])) if st["payload_off"][i] != R.M64 and st["keep"][i]][40]
    st["payload_off"][k] = dict(none=R.M64, **{"start+1": int(st["starts"][k]) + 1, "end+1": int(st["ends"][k]) + 1})[value]
    p = Plan(st, 4, 0, 96, True)
    assert p.want() == dict(error=R.E_ARG, bad=k + 1)
    sub = torch.full((8 * 4096,), CAN, dtype=torch.uint8, device="cuda")
    assert p.launch(ctx, sub) == 0
    s = summary_dict(ctx.read_summary(p.summary))
    assert s["error"] == R.E_ARG and s["reserved"][0] == k + 1
    assert (sub.cpu().numpy() == CAN).all() and (p.d_first.cpu().numpy() == CAN).all()


def test_more_nals_than_one_plan_workgroup(ctx):
    """5 000 NALs: three workgroups of 2 048, runs and AUs that cross their edges"""
    p = Plan(build_stream(77, 2, n_nals=5000), 2, R.ALIGN16, 96, True)
    w = p.want()
    _, sub, s = ctx.cenc_subsamples(p.d_stream, p.d_idx, p.d_au, p.st["n_aus"], keep=p.d_keep, payload_off=p.d_po, length_size=2, flags=R.ALIGN16)
    assert summary_dict(s) == p.summary_of(w)
    assert np.array_equal(sub.cpu().numpy().view(R.SUBSAMPLE), w["sub"])


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def test_end_to_end_on_a_live_context(ctx):
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import COMPACT, PARSED, SUMMARY
    from tests.hevc_synth import stream_4k30
    stream, n = stream_4k30(9, n_pictures=36, slices_per_picture=2, idr_every=12, payload_bytes=(60, 400))
    d = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    cap = n + 8
    index, parsed, cc = (torch.zeros(cap * z, dtype=torch.uint8, device="cuda") for z in (32, PARSED.itemsize, COMPACT.itemsize))
    structs = torch.zeros(8 << 20, dtype=torch.uint8, device="cuda")
    po = torch.zeros(cap * 8, dtype=torch.uint8, device="cuda")
    ss, ps = (torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2))
    got = ctx.index_parse_compact_async(d, index, cap, parsed, cc, structs, ss, ps, payload_off=po)
    assert got == n and int(ctx.read_summary(ps)["error"]) == 0
    au, nal_au, s, _ = ctx.access_units(index, parsed, cc, structs, got)
    n_aus = len(au)
    assert n_aus == 36
    idx = index[: got * 32]
    out, so, sz, frags, _ = ctx.mp4_fragment(d, idx, nal_au, au, flags=hbs.MP4_CUT_AT_IRAP, sample_duration=3003, track_id=1)
    assert len(frags) == 3
    plain = out.cpu().numpy().copy()
    sub_first, sub, s = ctx.cenc_subsamples(d, idx, nal_au, n_aus, payload_off=po[: got * 8], length_size=4)
    h_idx = idx.cpu().numpy().view(NAL_ENTRY)
    h_po = po[: got * 8].cpu().numpy().view(np.uint64)
    src = np.frombuffer(stream, dtype=np.uint8)
    w = R.subsamples(src, h_idx["start"].astype(np.int64), h_idx["end"].astype(np.int64), nal_au, n_aus, 4, payload_off=h_po)
    assert w["error"] == 0 and w["protected"] > 36 * 2 * 40
    assert np.array_equal(sub.cpu().numpy().view(R.SUBSAMPLE), w["sub"]) and np.array_equal(sub_first.cpu().numpy().view(np.uint64), w["sub_first"])
    assert int(s["stream_bytes"]) == int(sz.sum()) and int(s["rbsp_bytes"]) == w["protected"]
    key, iv0 = bytes(range(16, 32)), H("0011223344556677")
    iv, s = ctx.cenc_crypt(out, so, sz, sub_first, sub, key, iv0=iv0)
    want, done, used = R.crypt(plain, so, sz, w["sub_first"], w["sub"], key, iv0=iv0)
    enc = out.cpu().numpy()
    assert int(s["rbsp_bytes"]) == done == w["protected"] and np.array_equal(enc, want) and np.array_equal(iv.cpu().numpy().reshape(-1, 16), used)
    # what must stay clear, record by record: moof and mdat headers (outside every sample), length fields, NAL headers, slice headers
    clear = np.ones(len(plain), dtype=bool)
    for a in range(n_aus):
        p = int(so[a])
        for k in np.flatnonzero(nal_au - nal_au[0] == a):
            size = int(h_idx["end"][k] - h_idx["start"][k])
            assert int.from_bytes(bytes(plain[p:p + 4]), "big") == size
            if h_po[k] != R.M64:
                clear[p + 4 + int(h_po[k] - h_idx["start"][k]): p + 4 + size] = False
            p += 4 + size
        assert p == int(so[a] + sz[a])
    assert (~clear).sum() == done and np.array_equal(enc[clear], plain[clear]) and (enc[~clear] != plain[~clear]).any()
    # and back: the same call, then the samples as Annex-B are the source's NALs
    ctx.cenc_crypt(out, so, sz, sub_first, sub, key, iv0=iv0)
    assert np.array_equal(out.cpu().numpy(), plain)
    back, _, _ = ctx.lenpref_to_annexb(out, so, sz, length_size=4, startcode_bytes=4)
    assert bytes(back.cpu().numpy()) == b"".join(b"\x00\x00\x00\x01" + bytes(src[int(e["start"]):int(e["end"])]) for e in h_idx)


# ---- HIP graphs ----------------------------------------------------------------------------------------------------------------

def replay(launch, load, check, ctx):
    """captured on a side stream after one warm-up call on contents 0, replayed on contents 1 and 0 of the same buffers"""
    import torch
    side = torch.cuda.Stream()
    load(0)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert launch() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    check(0)
    held = ctx.device_bytes()
    for which in (1, 0):
        load(which)
        g.replay()
        torch.cuda.synchronize()
        check(which)
    assert ctx.device_bytes() == held


def test_one_replay_of_crypt_from_a_graph(ctx):
    import torch
    rng = np.random.default_rng(808)
    shapes = []
    for _ in range(2):                                      # two tables of 300 samples and 900 entries over one buffer size
        entries = [[(int(rng.integers(0, 30)), int(rng.integers(0, 300))) for _ in range(3)] for _ in range(300)]
        shapes.append(layout(entries, [0] * 300, lead=int(rng.integers(0, 16))))
    n = max(s[0] for s in shapes) + 16
    datas = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(2)]
    ivs = [rng.integers(0, 256, 16 * 300, dtype=np.uint8) for _ in range(2)]
    key = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    c = Crypt(datas[0], *shapes[0][1:], key, iv=ivs[0])

    def load(i):
        for t, a in zip((c.d_data, c.d_off, c.d_size, c.d_first, c.d_sub, c.d_iv), (datas[i],) + shapes[i][1:] + (ivs[i],)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        c.summary.fill_(0x5A)

    def check(i):
        want, done, _ = R.crypt(datas[i], *shapes[i][1:], key, iv=ivs[i])
        assert int(ctx.read_summary(c.summary)["rbsp_bytes"]) == done and int(ctx.read_summary(c.summary)["error"]) == 0
        assert np.array_equal(c.data(), want)
    replay(lambda: c.launch(ctx), load, check, ctx)


def test_one_replay_of_subsamples_from_a_graph(ctx):
    import torch
    sts = [build_stream(61, 2), build_stream(62, 2)]
    n_aus = sts[0]["n_aus"]
    assert n_aus == sts[1]["n_aus"]                         # equal host arguments: the same AU count, and the same stream size
    size = max(len(s["stream"]) for s in sts)
    for s in sts:
        s["stream"] = np.concatenate([s["stream"], np.zeros(size - len(s["stream"]), dtype=np.uint8)])
    p = Plan(sts[0], 2, 0, 96, True)
    wants = []
    for s in sts:
        p.st = s
        wants.append(p.want())
    assert wants[0]["error"] == wants[1]["error"] == 0 and len(wants[0]["sub"]) != len(wants[1]["sub"])
    sub = torch.full((8 * 2048,), CAN, dtype=torch.uint8, device="cuda")

    def load(i):
        s = sts[i]
        p.st = s
        idx = np.zeros(len(s["starts"]), dtype=NAL_ENTRY)
        idx["start"], idx["end"] = s["starts"], s["ends"]
        for t, a in zip((p.d_stream, p.d_idx, p.d_au, p.d_keep, p.d_po), (s["stream"], idx, s["nal_au"], s["keep"], s["payload_off"])):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        sub.fill_(CAN)
        p.summary.fill_(0x5A)

    def check(i):
        w = wants[i]
        assert summary_dict(ctx.read_summary(p.summary)) == p.summary_of(w)
        got = sub.cpu().numpy()
        assert np.array_equal(got[: 8 * len(w["sub"])].view(R.SUBSAMPLE), w["sub"]) and (got[8 * len(w["sub"]):] == CAN).all()
        assert np.array_equal(p.d_first.cpu().numpy()[: 8 * (n_aus + 1)].view(np.uint64), w["sub_first"])
    replay(lambda: p.launch(ctx, sub, cap=2048), load, check, ctx)


# ---- more entries than one step a range ------------------------------------------------------------------------------------------

def cut_table(rng, clear, protect, n_samples, lead, gaps):
    """samples cut at random entries of (clear, protect), `gaps` bytes between them -> (data_bytes, off, size, first, sub)"""
    E = len(clear)
    first = np.concatenate([[0], np.sort(rng.choice(np.arange(1, E), size=n_samples - 1, replace=False)), [E]])
    total = np.concatenate([[0], np.cumsum(clear + protect)])
    size = total[first[1:]] - total[first[:-1]]
    off = lead + np.concatenate([[0], np.cumsum(size + gaps)[:-1]])
    sub = np.zeros(E, dtype=R.SUBSAMPLE)
    sub["clear"], sub["protect"] = clear, protect
    return int(off[-1] + size[-1] + gaps[-1]), off.astype(np.uint64), size.astype(np.uint64), first.astype(np.uint64), sub


def steps_skipped(sub):
    """(the tiles of 64 KiB of protected bytes whose first byte lies behind the first 256 entries of its range, the tiles): for those
    the crypt kernel's first step ends in front of the tile and is skipped"""
    E = len(sub)
    K = np.concatenate([[0], np.cumsum(sub["protect"].astype(np.int64))])
    begin = np.array([E // RANGES * g + E % RANGES * g // RANGES for g in range(RANGES)])
    t0 = TILE * np.arange((int(K[-1]) + TILE - 1) // TILE)
    first = begin[np.searchsorted(K[begin], t0, side="right") - 1]
    return int((K[np.minimum(first + STEP, E)] <= t0).sum()), len(t0)


@pytest.mark.parametrize("per_range,clear_hi,protect_hi", ((STEP, 8, 40), (700, 2, 3)), ids=("257-a-range", "701-a-range"))
def test_more_entries_than_one_step_a_range(ctx, per_range, clear_hi, protect_hi):
    """more than 256 entries in a range, in 64 samples cut at random entries: the crypt kernel's walk goes on step after step to the
    tile's end (13 steps a tile, and 170), skips a first step that ends in front of the tile -- 2 of the 81 tiles with 256 or 257
    entries a range, 11 of 17 with 700 or 701 -- and a keystream block's byte walk goes on into the entries of the next step"""
    rng = np.random.default_rng(5151 + per_range - STEP)
    E = RANGES * per_range + 1000
    n, off, size, first, sub = cut_table(rng, rng.integers(0, clear_hi + 1, E), rng.integers(0, protect_hi + 1, E), 64, 5, rng.integers(0, 9, 64))
    protected = int(sub["protect"].astype(np.int64).sum())
    skipped, tiles = steps_skipped(sub)
    assert (skipped, tiles, n) == ((2, 81, 6328795) if per_range == STEP else (11, 17, 1796337)) and (sub["protect"] == 0).sum() > 1000
    data = rng.integers(0, 256, n, dtype=np.uint8)
    c = Crypt(data, off, size, first, sub, bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv=rng.integers(0, 256, 16 * len(off), dtype=np.uint8))
    assert c.launch(ctx) == 0
    got, _ = c.check(ctx)
    assert int(ctx.read_summary(c.summary)["rbsp_bytes"]) == protected and not np.array_equal(got, data)
    c.summary.fill_(0x5A)
    assert c.launch(ctx) == 0
    c.check(ctx, before=got)
    assert np.array_equal(c.data(), data)


# ---- tile edges --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lead", (32, 45))
@pytest.mark.parametrize("k", (0, 1, 15, 16, 17))
def test_a_sample_begins_k_bytes_in_front_of_a_tile(ctx, k, lead):
    """sample 0 protects 65 536 - k bytes in one entry, so the protected bytes of sample 1 -- the short ranges and the fillers of
    STRADDLE -- begin k bytes in front of the second tile; sample 2 protects nothing, sample 3 40 bytes"""
    rng = np.random.default_rng(600 + 32 * k + lead)
    samples = [[(3, TILE - k)], STRADDLE, [(9, 0), (4, 0)], [(2, 40)]]
    n, off, size, first, sub = layout(samples, [5, 0, 7, 3], lead=lead)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    c = Crypt(data, off, size, first, sub, bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv=rng.integers(0, 256, 16 * 4, dtype=np.uint8))
    assert c.launch(ctx) == 0
    got, _ = c.check(ctx)
    inside = np.zeros(n, dtype=bool)                        # by hand: the protected ranges, entry by entry
    for s, entries in enumerate(samples):
        p = int(off[s])
        for clear, protect in entries:
            inside[p + clear: p + clear + protect] = True
            p += clear + protect
    assert inside.sum() == TILE - k + 65 + 40 == int(ctx.read_summary(c.summary)["rbsp_bytes"])
    assert np.array_equal(got[~inside], data[~inside])
    for s, total in ((0, TILE - k), (1, 65), (3, 40)):       # one keystream a sample, no byte of it skipped
        mine = inside & (np.arange(n) >= int(off[s])) & (np.arange(n) < int(off[s] + size[s]))
        assert np.array_equal(got[mine], data[mine] ^ R.keystream(c.key, bytes(c.iv[16 * s: 16 * s + 16]), total)), s


# ---- offsets above 2^32 ------------------------------------------------------------------------------------------------------------

def test_samples_around_offset_4gib(ctx):
    """as tests/test_gpu_cbcs.py::test_samples_around_offset_4gib: the same allocation, the same first and last window; the middle
    window begins 68 KiB earlier, so that the sample with a (65535, 0) filler lies inside what is compared.  Both iv_modes; the
    second call of each restores the windows"""
    import torch
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(4097)
    G, total = 1 << 32, (1 << 32) + (64 << 20)
    big = torch.empty(total, dtype=torch.uint8, device="cuda")
    mid = G - 8192 - 69632
    windows = [(0, 4096), (mid, 69632 + 16384), (total - 4096, 4096)]
    placed = [(0, 100, [(9, 16 * 21 + 5)]), (1, 11, [(65535, 0), (7, 100), (0, 0), (3, 29)]), (1, 69632 + 1000, [(3, 160), (0, 75)]),
              (1, 69632 + 8192 - 1500, [(11, 16 * 180 + 2)]),                                              # lies across 2^32
              (1, 69632 + 8192 + 1500, [(0, 16 * 70)]), (1, 69632 + 8192 + 3000, [(5, 33)]), (2, 4096 - 16 * 30 - 7, [(7, 16 * 30)])]
    off = np.array([windows[w][0] + o for w, o, _ in placed], dtype=np.uint64)
    _, _, size, first, sub = layout([e for _, _, e in placed], [0] * len(placed))
    assert int(off[3]) < G < int(off[3] + size[3]) and int(off[-1] + size[-1]) == total and int(off[1] + size[1]) <= int(off[2])
    plain = [rng.integers(0, 256, z, dtype=np.uint8) for _, z in windows]
    for (lo, z), h in zip(windows, plain):
        big[lo: lo + z] = torch.from_numpy(h).cuda()
    key, iv = bytes(rng.integers(0, 256, 16, dtype=np.uint8)), rng.integers(0, 256, 16 * len(off), dtype=np.uint8)
    iv0 = H("fffffffffffffffd")
    d_off, d_size, d_first, d_sub, d_iv = dev(off), dev(size), dev(first), dev(sub), dev(iv)
    for mode in (0, 1):
        host = plain
        d_ivo = torch.full((16 * len(off),), CAN, dtype=torch.uint8, device="cuda")
        for again in (False, True):
            want, used = [], {}
            for w in range(len(windows)):                   # the reference, window by window, on offsets rebased to the window
                mine = [i for i, (pw, _, _) in enumerate(placed) if pw == w]
                _, _, wsize, wfirst, wsub = layout([placed[i][2] for i in mine], [0] * len(mine))
                woff = np.array([placed[i][1] for i in mine], dtype=np.uint64)
                ivs = np.concatenate([np.frombuffer(R.sample_ctr(i, iv, None if mode == 0 else iv0), dtype=np.uint8) for i in mine])
                out, done, _ = R.crypt(host[w], woff, wsize, wfirst, wsub, key, iv=ivs)
                want.append((out, done))
                used.update({i: ivs[16 * j: 16 * j + 16] for j, i in enumerate(mine)})
            summary = fresh_summary()
            prm = hbs.cenc_params(key, iv0=None if mode == 0 else iv0)
            assert ctx.cenc_crypt_async(big, total, d_off, d_size, len(off), d_first, d_sub, d_iv if mode == 0 else d_ivo, prm, summary) == 0
            assert summary_dict(ctx.read_summary(summary)) == dict(error=0, nal_count=len(sub), nal_found=len(off), rbsp_bytes=sum(d for _, d in want),
                                                                   stream_bytes=total, stop_reason=0, reserved=[0, 0, 0])
            for (lo, z), (out, _) in zip(windows, want):
                got = big[lo: lo + z].cpu().numpy()
                assert np.array_equal(got, out), (mode, again, lo, np.flatnonzero(got != out)[:8])
            if mode == 1:
                assert np.array_equal(d_ivo.cpu().numpy(), np.concatenate([used[i] for i in range(len(off))]))
            if not again:
                assert not np.array_equal(want[1][0], host[1])
                host = [out for out, _ in want]
        assert all(np.array_equal(out, p) for (out, _), p in zip(want, plain)), mode


# ---- carved buffers ----------------------------------------------------------------------------------------------------------------

def small_table(rng, n_samples, lead):
    """a few dozen samples of 0 to 4 entries; data_bytes is no multiple of 16 and the last sample ends on the last byte"""
    entries = [[(int(rng.integers(0, 21)), int(rng.integers(0, 121))) for _ in range(int(rng.integers(0, 5)))] for _ in range(n_samples - 1)] + [[(4, 57)]]
    n, off, size, first, sub = layout(entries, rng.integers(0, 9, n_samples - 1).tolist() + [0], lead=lead)
    if n % 16 == 0:
        return small_table(rng, n_samples, lead + 1)
    assert int(off[-1] + size[-1]) == n
    return n, off, size, first, sub


def test_carved_buffers_at_each_accepted_alignment(ctx):
    """every pointer of hbs_cenc_crypt and hbs_cenc_subsamples inside a larger allocation, at each offset from a page boundary its
    alignment accepts -- each pointer goes through its whole set while the others rotate; 4 KiB of known bytes lie on both sides
    of every buffer and are looked at afterwards"""
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(66)
    for k in range(len(K.OFFS8)):
        o16 = lambda j: K.OFFS16[(k + j) % len(K.OFFS16)]          # noqa: E731
        o8 = lambda j: K.OFFS8[(k + j) % len(K.OFFS8)]             # noqa: E731
        n, off, size, first, sub = small_table(rng, 40, int(rng.integers(0, 16)))
        data, key, ns = rng.integers(0, 256, n, dtype=np.uint8), bytes(rng.integers(0, 256, 16, dtype=np.uint8)), len(off)
        mode = k % 2
        iv, iv0 = rng.integers(0, 256, 16 * ns, dtype=np.uint8), bytes(rng.integers(0, 256, 8, dtype=np.uint8))
        want, done, used = R.crypt(data, off, size, first, sub, key, iv=None if mode else iv, iv0=iv0 if mode else None)
        cd = K.Carved(n, o16(0), CAN, K.PAD, True).put(data)
        co = K.Carved(ns * 8, o8(1), 0xFF, K.PAD, True).put(off)
        cz = K.Carved(ns * 8, o8(4), 0xFF, K.PAD, True).put(size)
        cf = K.Carved((ns + 1) * 8, o8(7), 0xFF, K.PAD, True).put(first)
        cs = K.Carved(len(sub) * 8, o8(9), 0xFF, K.PAD, True).put(sub)
        ci = K.Carved(ns * 16, o16(3), CAN, K.PAD, True)
        if not mode:
            ci.put(iv)
        cm = K.Carved(64, o16(5), 0xEE, K.PAD, True)
        prm = hbs.cenc_params(key, iv0=iv0 if mode else None)
        assert ctx.cenc_crypt_async(cd.view, n, co.view, cz.view, ns, cf.view, cs.view, ci.view, prm, cm.view) == 0, k
        summary_matches(ctx.read_summary(cm.view), dict(error=0, nal_count=len(sub), nal_found=ns, rbsp_bytes=done, stream_bytes=n, stop_reason=0,
                                                        reserved=[0, 0, 0]))
        assert np.array_equal(cd.get(), want) and np.array_equal(ci.get(), used.reshape(-1)), k
        for name, c in (("data", cd), ("sample_off", co), ("sample_size", cz), ("sub_first", cf), ("sub", cs), ("iv", ci), ("summary", cm)):
            assert c.intact(), (k, name, c.damage())
    for k in range(16):                                     # hbs_cenc_subsamples: d_keep at 0 to 15, d_nal_au through OFFS4
        o16 = lambda j: K.OFFS16[(k + j) % len(K.OFFS16)]          # noqa: E731
        o8 = lambda j: K.OFFS8[(k + j) % len(K.OFFS8)]             # noqa: E731
        L = (1, 2, 4)[k % 3]
        st = build_stream(700 + k, L, n_nals=300)
        p = Plan(st, L, k % 2, 96, True)
        w = p.want()
        nn, total = len(st["starts"]), len(w["sub"])
        idx = np.zeros(nn, dtype=NAL_ENTRY)
        idx["start"], idx["end"] = st["starts"], st["ends"]
        cs = K.Carved(len(st["stream"]), o16(0), 0x3C, K.PAD, True).put(st["stream"])
        cx = K.Carved(nn * 32, o8(2), 0xFF, K.PAD, True).put(idx)
        ck = K.Carved(nn, k, 0xFF, K.PAD, True).put(st["keep"])
        ca = K.Carved(nn * 4, K.OFFS4[k % len(K.OFFS4)], 0xFF, K.PAD, True).put(st["nal_au"])
        cp = K.Carved(nn * 8, o8(5), 0xFF, K.PAD, True).put(st["payload_off"])
        cf = K.Carved((st["n_aus"] + 1) * 8, o8(8), CAN, K.PAD, True)
        cu = K.Carved(total * 8, o8(0), CAN, K.PAD, True)
        cm = K.Carved(64, o16(4), 0xEE, K.PAD, True)
        assert ctx.cenc_subsamples_async(cs.view, len(st["stream"]), cx.view, nn, ca.view, st["n_aus"], p.prm, cf.view, cu.view, cm.view, keep=ck.view,
                                         payload_off=cp.view, sub_cap=total) == 0, k
        assert summary_dict(ctx.read_summary(cm.view)) == p.summary_of(w), k
        assert np.array_equal(cu.get().view(R.SUBSAMPLE), w["sub"]) and np.array_equal(cf.get().view(np.uint64), w["sub_first"]), k
        for name, c in (("stream", cs), ("index", cx), ("keep", ck), ("nal_au", ca), ("payload_off", cp), ("sub_first", cf), ("sub", cu), ("summary", cm)):
            assert c.intact(), (k, name, c.damage())


def test_the_nearest_misalignment_of_each_pointer_is_refused(ctx):
    """+8 on a 16-byte pointer, +4 on an 8-byte one, +2 and +1 on d_nal_au: HBS_E_ARG at once, and every output and the summary hold
    what they were filled with"""
    import torch
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(67)
    n, off, size, first, sub = small_table(rng, 40, 3)
    x = Crypt(rng.integers(0, 256, n, dtype=np.uint8), off, size, first, sub, bytes(range(16)), iv0=bytes(8))
    x.d_data = torch.cat([x.d_data, torch.full((64,), CAN, dtype=torch.uint8, device="cuda")])
    prm = x.prm.ctypes.data
    base = dict(data=x.d_data.data_ptr(), off=x.d_off.data_ptr(), size=x.d_size.data_ptr(), first=x.d_first.data_ptr(), sub=x.d_sub.data_ptr(),
                iv=x.d_iv.data_ptr(), summary=x.summary.data_ptr())
    order = ("data", "off", "size", "first", "sub", "iv", "summary")

    def crypt(**shift):
        a = {name: base[name] + shift.get(name, 0) for name in order}
        return ctx.lib.hbs_cenc_crypt(ctx.h, a["data"], n - 16, a["off"], a["size"], 0 if shift else x.n, a["first"], a["sub"], a["iv"], prm, a["summary"])
    # (the shifted calls pass no samples and 16 bytes less, so that a call that were accepted would stay inside the buffers)
    for name, by in (("data", 8), ("iv", 8), ("summary", 8), ("off", 4), ("size", 4), ("first", 4), ("sub", 4)):
        assert crypt(**{name: by}) == R.E_ARG, name
    torch.cuda.synchronize()
    assert (x.summary.cpu().numpy() == 0x5A).all() and np.array_equal(x.data(), x.host[0]) and (x.d_iv.cpu().numpy() == CAN).all()
    st = build_stream(800, 4, n_nals=300)
    p = Plan(st, 4, 0, 96, True)
    total, nn = len(p.want()["sub"]), len(st["starts"])
    d_sub = torch.full((total * 8 + 64,), CAN, dtype=torch.uint8, device="cuda")
    base = dict(stream=p.d_stream.data_ptr(), index=p.d_idx.data_ptr(), keep=p.d_keep.data_ptr(), nal_au=p.d_au.data_ptr(), po=p.d_po.data_ptr(),
                first=p.d_first.data_ptr(), sub=d_sub.data_ptr(), summary=p.summary.data_ptr())

    def plan(**shift):
        a = {name: v + shift.get(name, 0) for name, v in base.items()}
        return ctx.lib.hbs_cenc_subsamples(ctx.h, a["stream"], len(st["stream"]) - 16, a["index"], nn - 1, a["keep"], a["nal_au"], st["n_aus"], a["po"],
                                           p.prm.ctypes.data, a["first"], a["sub"], total, a["summary"])
    for name, by in (("stream", 8), ("summary", 8), ("index", 4), ("po", 4), ("first", 4), ("sub", 4), ("nal_au", 2), ("nal_au", 1)):
        assert plan(**{name: by}) == R.E_ARG, (name, by)
    torch.cuda.synchronize()
    assert (p.summary.cpu().numpy() == 0x5A).all() and (d_sub.cpu().numpy() == CAN).all() and (p.d_first.cpu().numpy() == CAN).all()
    assert plan(keep=1) == 0                                # d_keep takes any address
