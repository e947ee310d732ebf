"""hbs_mp4_protect on the GPU against the plain loop of tests/_mp4_protect_ref.py, byte for byte: plan first, then a run into
outputs of exactly the planned capacity with canaries behind d_out, both sample tables and d_frag_out, every summary field
checked.  Inputs are made by hbs_mp4_fragment and hbs_cenc_subsamples on small synthetic streams.  A plan workgroup takes 256
fragments or samples (kProtLanes: hbs_mp4prot.h), scan_parts 2 048 workgroups a pass (hbs_plan.h), a copy workgroup 64 KiB of
output of which it stages up to 448 fragments."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import _mp4_protect_ref as P
from tests import _mp4_ref as R
from tests._mp4_ref import random_case

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
W = 256                         # fragments, and samples, of a plan workgroup
PASS = 256 * 8                  # plan workgroups scan_parts takes in one pass
TILE = 64 * 1024
FRAG = R.FRAG.itemsize


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).cuda() if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")


def canary(n):
    import torch
    return torch.full((n + PAD,), CAN, dtype=torch.uint8, device="cuda")


def summary_dict(s):
    return dict(error=int(s["error"]), nal_count=int(s["nal_count"]), nal_found=int(s["nal_found"]), rbsp_bytes=int(s["rbsp_bytes"]),
                stream_bytes=int(s["stream_bytes"]), stop_reason=int(s["stop_reason"]), reserved=[int(x) for x in s["reserved"]])


def ivs(rng, n, V):
    iv = rng.integers(0, 256, 16 * max(n, 1), dtype=np.uint8)
    if V == 8:
        iv.reshape(-1, 16)[:, 8:] = 0
    return iv


def build(ctx, rng, n_aus=200, L=4, max_nal=3000, case=None, **prm):
    """fragments and their subsample table, made by the library itself on a synthetic stream
    -> dict(d_in, data, frags, first, sub, so, ss, n): data the fragments' bytes on the host, so / ss hbs_mp4_fragment's sample tables"""
    if case is None:
        case = random_case(rng, n_aus, max_nal=max_nal if L > 1 else 255, keep_some=False)
    stream, index, keep, nal_au, au, dts, pts = case
    d = dev(stream)
    prm = dict(dict(flags=R.CUT_AT_IRAP, max_samples=40, sample_duration=1), **prm)
    out, so, ss, frags, _ = ctx.mp4_fragment(d, index, nal_au, au, keep=keep, dts=dts, pts=pts, length_size=L, **prm)
    first, sub, _ = ctx.cenc_subsamples(d, index, nal_au, len(au), keep=keep, length_size=L, clear_lead=int(rng.integers(2, 120)))
    first, sub = first.cpu().numpy().view(np.uint64).copy(), sub.cpu().numpy().view(P.SUBSAMPLE).copy()
    assert int(np.diff(first.astype(np.int64)).max()) <= 39
    return dict(d_in=out, data=out.cpu().numpy(), frags=frags, first=first, sub=sub, so=so, ss=ss, n=len(au))


def put(b, V, iv, d_in=None, nbytes=None, frags=None, first=None, sub=None, n_samples=None):
    import hevcbitstream_amd as hbs
    frags = b["frags"] if frags is None else frags
    first = b["first"] if first is None else first
    return dict(d_in=b["d_in"] if d_in is None else d_in, nbytes=len(b["data"]) if nbytes is None else nbytes, frag=dev(frags), R=len(frags),
                first=dev(first), sub=dev(b["sub"] if sub is None else sub), iv=dev(iv) if V else None, N=len(first) - 1 if n_samples is None else n_samples,
                prm=hbs.mp4_protect_params(iv_size=V))


def call(ctx, d, out, so, ss, fr, out_cap=None, fill=0x5A):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), fill, dtype=torch.uint8, device="cuda")
    rc = ctx.mp4_protect_async(d["d_in"], d["nbytes"], d["frag"], d["R"], d["first"], d["sub"], d["iv"], d["N"], d["prm"], out, summary,
                               sample_off=so, sample_size=ss, frag_out=fr, out_cap=out_cap)
    assert rc == 0, rc
    return ctx.read_summary(summary)


def check_outputs(out, so, ss, fr, want):
    want_out, want_off, want_size, want_frags, want_s = want
    need, n, R_ = want_s["stream_bytes"], len(want_off), want_s["nal_count"]
    o = out.cpu().numpy()
    bad = np.flatnonzero(o[:need] != want_out)
    if len(bad):
        r = int(np.searchsorted(want_frags["out_off"], bad[0], side="right")) - 1
        raise AssertionError("output differs at byte %d (fragment %d of %d samples, byte %d of it; %d bytes of %d differ; got %s want %s)" % (
            bad[0], r, int(want_frags["samples"][r]), bad[0] - int(want_frags["out_off"][r]), len(bad), need,
            o[bad[0]:bad[0] + 8].tolist(), want_out[bad[0]:bad[0] + 8].tolist()))
    assert (o[need:] == CAN).all(), "stored behind the output"
    for name, t, w in (("d_sample_off", so, want_off), ("d_sample_size", ss, want_size)):
        p = t.cpu().numpy()
        assert np.array_equal(p[: n * 8].view(np.uint64), w), name
        assert (p[n * 8:] == CAN).all(), "stored behind " + name
    p = fr.cpu().numpy()
    assert np.array_equal(p[: R_ * FRAG].view(R.FRAG), want_frags), "d_frag_out"
    assert (p[R_ * FRAG:] == CAN).all(), "stored behind d_frag_out"


def run(ctx, b, V, iv, want=None, **kw):
    """plan, then a run into outputs of exactly the planned capacity; everything against the plain loop.
    -> (out, the reference's results, summary, device inputs)"""
    d = put(b, V, iv, **kw)
    if want is None:
        want = P.protect(b["data"], kw.get("frags", b["frags"]), kw.get("first", b["first"]), kw.get("sub", b["sub"]), iv if V else None, V)
    want_s = want[4]
    assert want_s["error"] == 0, want_s
    s = call(ctx, d, None, None, None, None)
    assert summary_dict(s) == want_s
    need, n, frags = want_s["stream_bytes"], d["N"], d["R"]
    out, so, ss, fr = canary(need), canary(n * 8), canary(n * 8), canary(frags * FRAG)
    s2 = call(ctx, d, out, so, ss, fr, out_cap=need)
    assert summary_dict(s2) == want_s
    check_outputs(out, so, ss, fr, want)
    return out[:need], want, s2, d


def fails(ctx, b, V, iv, error, reserved, out_cap=None, **kw):
    """a run that must report `error` with these reserved words and store nothing but the summary -> the summary"""
    d = put(b, V, iv, **kw)
    n, frags = d["N"], d["R"]
    room = (1 << 20) if out_cap is None else out_cap
    out, so, ss, fr = canary(room), canary(n * 8), canary(n * 8), canary(frags * FRAG)
    for o in (None, out):
        s = call(ctx, d, o, so if o is not None else None, ss if o is not None else None, fr if o is not None else None, out_cap=room if o is not None else None)
        if o is None and error == P.E_CAPACITY:
            assert int(s["error"]) == 0
            continue
        assert int(s["error"]) == error and [int(x) for x in s["reserved"]] == reserved, s
        assert int(s["nal_count"]) == frags and int(s["nal_found"]) == n and int(s["stop_reason"]) == 0
    for t in (out, so, ss, fr):
        assert (t.cpu().numpy() == CAN).all(), "stored on an error"
    return s


# ---- 1. random mixes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", (1, 2, 4))
@pytest.mark.parametrize("V", (0, 8, 16))
def test_random_mixes(ctx, V, L):
    rng = np.random.default_rng(100 + 10 * V + L)
    b = build(ctx, rng, 200, L)
    assert 1 <= int(b["frags"]["samples"].min()) and int(b["frags"]["samples"].max()) <= 40 and len(b["frags"]) > 5
    _, want, s, _ = run(ctx, b, V, ivs(rng, b["n"], V))
    assert int(s["stream_bytes"]) == len(b["data"]) + 53 * len(b["frags"]) + (V + 3) * b["n"] + 6 * len(b["sub"])


# ---- 2. alignments and buffer ends ------------------------------------------------------------------------------------------------------

def test_fragments_at_each_byte_offset_and_the_end_of_the_allocation(ctx):
    """the fragments of one build, in another order, each at another byte offset mod 16 of a 12 MiB allocation of its own, junk of 0
    to 100 000 bytes between them; the last one ends with the allocation"""
    import torch
    rng = np.random.default_rng(52)
    b = build(ctx, rng, 200, 4)
    frags = b["frags"].copy()
    Rn = len(frags)
    assert Rn >= 6
    total = 12 << 20
    host = rng.integers(0, 256, size=total, dtype=np.uint8)
    gaps = [0, 1, 15, 17, 100000, 33]
    at, placed = 0, []
    for r in range(Rn):
        at += gaps[r % len(gaps)]
        at += (r % 16 - at) % 16                          # fragment r at r mod 16
        placed.append(at)
        at += int(frags["out_bytes"][r])
    shift = (total - at) // 16 * 16
    last = total - int(frags["out_bytes"][-1])            # the last one ends with the allocation, wherever that puts it
    for r in range(Rn):
        o = placed[r] + shift if r + 1 < Rn else last
        assert r + 1 == Rn or o % 16 == r % 16
        z, old = int(frags["out_bytes"][r]), int(frags["out_off"][r])
        host[o:o + z] = b["data"][old:old + z]
        frags["out_off"][r] = o
    assert int(frags["out_off"][-1] + frags["out_bytes"][-1]) == total and len({int(x) % 16 for x in frags["out_off"]}) >= min(Rn - 1, 16)
    torch.cuda.empty_cache()                              # (no cached block to cut the 12 MiB from)
    d_in = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_in.copy_(torch.from_numpy(host))
    placed_b = dict(b, data=host, frags=frags, d_in=d_in)
    for V in (8, 0):
        run(ctx, placed_b, V, ivs(rng, b["n"], V))


# ---- 3. tiles -----------------------------------------------------------------------------------------------------------------------

def test_tiles_inside_a_payload_and_inside_saiz_and_senc(ctx):
    rng = np.random.default_rng(53)
    big = 200 * 1024
    sizes = np.array([40, big, 7, 300])
    starts = np.cumsum(np.array([3, 5, 4, 3]) + np.concatenate([[0], sizes[:-1]]))
    stream = rng.integers(0, 256, size=int(starts[-1] + sizes[-1]), dtype=np.uint8)
    stream[starts] = 0x02                                 # VCL NALs: protected ranges
    case = (stream, R.entries(starts, starts + sizes), None, np.array([0, 1, 2, 2], np.uint32), R.au_records([1, 0, 0]), None, None)
    b = build(ctx, rng, case=case, max_samples=1)
    assert len(b["frags"]) == 3 and int(b["frags"]["out_bytes"][1]) > 3 * TILE
    run(ctx, b, 16, ivs(rng, 3, 16))
    n = 6000                                              # one fragment of 6 000 tiny samples: saiz 6 017 bytes, senc and trun 96 000 each
    starts = 5 * np.arange(n) + 3
    stream = rng.integers(0, 256, size=5 * n + 8, dtype=np.uint8)
    stream[starts] = np.where(np.arange(n) % 3 == 0, 0x40, 0x02)
    case = (stream, R.entries(starts, starts + 3), None, np.arange(n, dtype=np.uint32) + 9, R.au_records(np.zeros(n, np.uint32)), None, None)
    b = build(ctx, rng, case=case, flags=0, max_samples=0)
    assert len(b["frags"]) == 1 and 16 * n > TILE and (8 + 2) * n + 6 * len(b["sub"]) > TILE
    run(ctx, b, 8, ivs(rng, n, 8))


def uniform_case(n, rng):
    """n access units of one 3-byte VCL NAL, a fragment each"""
    starts = 5 * np.arange(n) + 3
    stream = rng.integers(0, 256, size=5 * n + 8, dtype=np.uint8)
    stream[starts] = 0x02
    return (stream, R.entries(starts, starts + 3), None, np.arange(n, dtype=np.uint32), R.au_records(np.zeros(n, np.uint32)), None, None)


def uniform_output(b, V, iv):
    """the output for fragments that all have one sample of one entry, as array arithmetic over the rows"""
    n = len(b["frags"])
    fin = int(b["frags"]["out_bytes"][0])
    assert (b["frags"]["out_bytes"] == fin).all() and (b["frags"]["samples"] == 1).all() and len(b["sub"]) == n and len(b["data"]) == n * fin
    rows = b["data"].reshape(n, fin)
    M = 141 + 19 + V + 6
    word = lambda v: np.frombuffer(struct.pack(">I", v), dtype=np.uint8)          # noqa: E731
    out = np.zeros((n, fin + 53 + V + 3 + 6), dtype=np.uint8)
    out[:, :104] = rows[:, :104]
    out[:, 0:4], out[:, 24:28], out[:, 84:88] = word(M), word(M - 24), word(M + 8)
    out[:, 104:122] = np.frombuffer(struct.pack(">I4sIBI", 18, b"saiz", 0, 0, 1) + bytes([V + 8]), dtype=np.uint8)
    out[:, 122:142] = np.frombuffer(struct.pack(">I4sIII", 20, b"saio", 0, 1, 158), dtype=np.uint8)
    out[:, 142:158] = np.frombuffer(struct.pack(">I4sII", 16 + V + 2 + 6, b"senc", 2, 1), dtype=np.uint8)
    out[:, 158:158 + V] = iv.reshape(-1, 16)[:n, :V]
    out[:, 158 + V:160 + V] = (0, 1)
    out[:, 160 + V:162 + V] = b["sub"]["clear"].astype(">u2").view(np.uint8).reshape(n, 2)
    out[:, 162 + V:166 + V] = b["sub"]["protect"].astype(">u4").view(np.uint8).reshape(n, 4)
    out[:, M:] = rows[:, 104:]
    fout = out.shape[1]
    fr = b["frags"].copy()
    fr["out_off"], fr["out_bytes"] = np.arange(n, dtype=np.uint64) * np.uint64(fout), fout
    so = (np.arange(n, dtype=np.uint64) * np.uint64(fout) + np.uint64(M + 8)).astype(np.uint64)
    return out.reshape(-1), so, np.full(n, fin - 112, dtype=np.uint64), fr, P.summary(0, n, n, n, n * fout)


def test_a_tile_of_slow_chunks_only_and_a_partial_last_chunk(ctx):
    """350 fragments of one 7-byte sample, iv_size 8: an mdat has 15 bytes, so no chunk lies wholly inside one.  All 4 096 chunks of
    the first tile are on the copy's slow list; the second tile has 614 bytes, 6 in its last chunk"""
    rng = np.random.default_rng(55)
    n = 350
    b = build(ctx, rng, case=uniform_case(n, rng), flags=0, max_samples=1)
    assert len(b["frags"]) == n and (b["frags"]["out_bytes"] == 112 + 7).all()
    iv = ivs(rng, n, 8)
    out, want, _, _ = run(ctx, b, 8, iv)
    assert len(out) == 189 * n == TILE + 614 and 614 % 16 == 6
    quick = uniform_output(b, 8, iv)
    assert all(np.array_equal(x, y) for x, y in zip(quick[:4], want[:4])) and quick[4] == want[4]


def test_more_fragment_blocks_than_one_scan_pass(ctx):
    """70 000 fragments of one sample against the plain loop, and against the same output as array arithmetic; then 525 000 of
    them, which is more plan workgroups (of fragments and of samples) than scan_parts takes in one pass, against the arithmetic"""
    rng = np.random.default_rng(54)
    n = 70000
    b = build(ctx, rng, case=uniform_case(n, rng), flags=0, max_samples=1)
    iv = ivs(rng, n, 8)
    _, want, _, _ = run(ctx, b, 8, iv)
    quick = uniform_output(b, 8, iv)
    assert all(np.array_equal(x, y) for x, y in zip(quick[:4], want[:4])) and quick[4] == want[4]
    n = PASS * W + 712
    b = build(ctx, rng, case=uniform_case(n, rng), flags=0, max_samples=1)
    iv = ivs(rng, n, 16)
    assert len(b["frags"]) == n > PASS * W
    run(ctx, b, 16, iv, want=uniform_output(b, 16, iv))


# ---- 4. the sample rule at its edges ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge_base(ctx):
    """600 samples; sample 300 is one NAL of 70 000 bytes"""
    rng = np.random.default_rng(55)
    case = list(random_case(rng, 600, max_nal=400, max_nals_per_au=2, keep_some=False))
    stream, index, _, nal_au, au, _, _ = case
    k = int(np.flatnonzero(nal_au - nal_au[0] == 300)[0])
    grow = 70000 - int(index["end"][k] - index["start"][k])
    stream = np.concatenate([stream[:int(index["end"][k])], rng.integers(0, 256, grow, dtype=np.uint8), stream[int(index["end"][k]):]])
    index["end"][k] += np.uint64(grow)
    index["start"][k + 1:] += np.uint64(grow)
    index["end"][k + 1:] += np.uint64(grow)
    stream[index["start"].astype(np.int64)[index["end"] > index["start"]]] = 0x02          # every NAL a VCL NAL: every sample has entries
    case[0], case[1] = stream, index
    b = build(ctx, rng, case=tuple(case))
    assert b["n"] == 600 and int(b["ss"][300]) >= 70000
    return b


@pytest.mark.parametrize("V", (0, 8, 16))
def test_entry_count_at_the_cap(ctx, edge_base, V):
    rng = np.random.default_rng(56 + V)
    b, cap = edge_base, P.max_entries(V)
    iv = ivs(rng, 600, V)
    for j in (0, 255, 256, 599):
        n = int(b["first"][j + 1] - b["first"][j])
        e = int(b["first"][j])
        for extra, good in ((cap - n, True), (cap + 1 - n, False)):
            sub = np.concatenate([b["sub"][:e], np.zeros(extra, dtype=P.SUBSAMPLE), b["sub"][e:]])
            first = b["first"].copy()
            first[j + 1:] += np.uint64(extra)
            if good:
                if j in (0, 599):
                    run(ctx, b, V, iv, first=first, sub=sub)
            else:
                fails(ctx, b, V, iv, P.E_ARG, [j + 1, 0, 0], first=first, sub=sub)


def test_each_sample_error_and_the_lowest(ctx, edge_base):
    rng = np.random.default_rng(57)
    b = edge_base
    iv = ivs(rng, 600, 8)
    e = int(b["first"][300])
    c, p = int(b["sub"]["clear"][e]), int(b["sub"]["protect"][e])
    assert c + p >= 65536
    sub = b["sub"].copy()
    sub["clear"][e], sub["protect"][e] = 65535, c + p - 65535
    run(ctx, b, 8, iv, sub=sub)
    sub["clear"][e], sub["protect"][e] = 65536, c + p - 65536
    fails(ctx, b, 8, iv, P.E_ARG, [301, 0, 0], sub=sub)
    for j in (0, 255, 256, 599):
        e = int(b["first"][j])
        for field, step in (("protect", 1), ("clear", 1), ("protect", -1 if int(b["sub"]["protect"][e]) else 2)):
            sub = b["sub"].copy()
            sub[field][e] = int(sub[field][e]) + step      # a sum off by one
            fails(ctx, b, 8, iv, P.E_ARG, [j + 1, 0, 0], sub=sub)
        bad = iv.copy()
        bad[16 * j + 8 + j % 8] = 1                        # a non-zero IV tail: an error with 8-byte IVs and with no others
        fails(ctx, b, 8, bad, P.E_ARG, [j + 1, 0, 0])
        if j == 255:
            run(ctx, b, 16, bad)
        if j:
            first = b["first"].copy()
            first[j] = first[j + 1] + np.uint64(1)         # d_sub_first falls behind sample j - 1 ... which then has too many entries or not
            want = P.protect(b["data"], b["frags"], first, b["sub"], iv, 8)[4]
            assert want["error"] == P.E_ARG and want["reserved"][0] in (j, j + 1)
            fails(ctx, b, 8, iv, P.E_ARG, want["reserved"], first=first)
    first = b["first"].copy()
    first[0] = 1
    fails(ctx, b, 8, iv, P.E_ARG, [1, 0, 0], first=first)
    # two offenders: the lowest; one of each group: the first group's, though it is the higher sample
    sub = b["sub"].copy()
    sub["protect"][int(b["first"][256])] += 1
    sub["protect"][int(b["first"][255])] += 1
    fails(ctx, b, 8, iv, P.E_ARG, [256, 0, 0], sub=sub)
    bad = iv.copy()
    bad[16 * 400 + 9] = 7
    fails(ctx, b, 8, bad, P.E_ARG, [401, 0, 0], sub=sub)


# ---- 5. the fragment rule -----------------------------------------------------------------------------------------------------------

def test_each_fragment_error_and_the_lowest(ctx, edge_base):
    import torch
    rng = np.random.default_rng(58)
    b = edge_base
    iv = ivs(rng, 600, 8)
    Rn = len(b["frags"])
    assert Rn > 12
    bad_sub = b["sub"].copy()
    bad_sub["protect"][0] += 1                             # a sample error in sample 0, which a fragment error hides

    def patched(r, at, bit=1):
        d = b["d_in"].clone()
        d[int(b["frags"]["out_off"][r]) + at] ^= bit
        return d

    for r in (0, 7, Rn - 1):
        S = int(b["frags"]["samples"][r])
        for at in (76 + 3, 80 + 3, 84 + 3, 88 + 16 * S + 3, 88 + 16 * S + 4, 4, 28, 36, 52, 72, 3, 27, 71):      # trun flags, count, data_offset, mdat size ...
            fails(ctx, b, 8, iv, P.E_ARG, [0, r + 1, 0], d_in=patched(r, at))
        fails(ctx, b, 8, iv, P.E_ARG, [0, r + 1, 0], d_in=patched(r, 80 + 3), sub=bad_sub)
    for at in (12, 20, 40, 44, 56, 60):                    # the mfhd, the tfhd's flags and track, the tfdt's version and time: as they are
        d = patched(5, at, 0x10)
        want = P.protect(d.cpu().numpy(), b["frags"], b["first"], b["sub"], iv, 8)
        run(ctx, b, 8, iv, want=want, d_in=d)
    # two broken fragments: the lowest
    d = patched(9, 83)
    d[int(b["frags"]["out_off"][4]) + 79] ^= 1
    fails(ctx, b, 8, iv, P.E_ARG, [0, 5, 0], d_in=d)
    # a fragment that leaves the buffer
    fails(ctx, b, 8, iv, P.E_ARG, [0, Rn, 0], nbytes=len(b["data"]) - 1)
    f = b["frags"].copy()
    f["out_off"][3] = np.uint64((1 << 64) - 8)
    fails(ctx, b, 8, iv, P.E_ARG, [0, 4, 0], frags=f)
    # the numbering rule
    f = b["frags"].copy()
    f["first_au"][6] += 1
    fails(ctx, b, 8, iv, P.E_ARG, [0, 7, 0], frags=f, sub=bad_sub)
    f = b["frags"].copy()
    f["first_au"] += 12345                                 # a pointer offset: only differences count
    run(ctx, b, 8, iv, frags=f, want=P.protect(b["data"], f, b["first"], b["sub"], iv, 8))
    more = np.concatenate([b["first"], b["first"][-1:]])   # a sample more than the fragments have
    fails(ctx, b, 8, np.concatenate([iv, np.zeros(16, np.uint8)]), P.E_ARG, [0, Rn, 0], first=more)
    fails(ctx, b, 8, iv, P.E_ARG, [0, Rn, 0], first=b["first"][:-1].copy())      # a sample fewer
    assert torch.equal(b["d_in"].cpu(), torch.from_numpy(b["data"]))


# ---- 6. capacity and refusals ----------------------------------------------------------------------------------------------------------

def test_capacity_plan_only_and_the_empty_call(ctx, edge_base):
    import torch
    rng = np.random.default_rng(59)
    b = edge_base
    iv = ivs(rng, 600, 16)
    want = P.protect(b["data"], b["frags"], b["first"], b["sub"], iv, 16)[4]
    s = fails(ctx, b, 16, iv, P.E_CAPACITY, [0, 0, 0], out_cap=want["stream_bytes"] - 1)
    assert summary_dict(s) == dict(want, error=P.E_CAPACITY)
    d = put(b, 16, iv)
    assert summary_dict(call(ctx, d, None, None, None, None)) == want                  # plan only: the summary alone
    e = dict(d, R=0, N=0)
    out = canary(64)
    for o in (None, out):
        assert summary_dict(call(ctx, e, o, None, None, None, out_cap=64)) == P.summary()
    assert (out.cpu().numpy() == CAN).all()
    none = dict(e, d_in=None, nbytes=0, frag=None, first=None, sub=None, iv=None)
    assert summary_dict(call(ctx, none, None, None, None, None)) == P.summary()
    torch.cuda.synchronize()


def test_refused_at_once(ctx, edge_base):
    import torch
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(60)
    b = edge_base
    d = put(b, 8, ivs(rng, 600, 8))
    n, Rn = d["N"], d["R"]
    out, so, ss, fr = canary(1 << 20), canary(n * 8), canary(n * 8), canary(Rn * FRAG)
    summary = torch.full((64,), 0x5A, dtype=torch.uint8, device="cuda")
    odd = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def raw(**change):
        """the C call itself with one argument changed: pointers as integers (None: NULL), params as a record or None"""
        a = dict(d_in=d["d_in"].data_ptr(), in_bytes=d["nbytes"], frag=d["frag"].data_ptr(), n_frags=Rn, first=d["first"].data_ptr(),
                 sub=d["sub"].data_ptr(), iv=d["iv"].data_ptr(), n_samples=n, params=hbs.mp4_protect_params(iv_size=8), out=out.data_ptr(),
                 out_cap=1 << 20, so=so.data_ptr(), ss=ss.data_ptr(), fr=fr.data_ptr(), summary=summary.data_ptr())
        a.update(change)
        prm = a["params"]
        vp = lambda v: None if v is None else C.c_void_p(v)      # noqa: E731
        return ctx.lib.hbs_mp4_protect(ctx.h, vp(a["d_in"]), a["in_bytes"], vp(a["frag"]), a["n_frags"], vp(a["first"]), vp(a["sub"]), vp(a["iv"]),
                                       a["n_samples"], None if prm is None else prm.ctypes.data_as(C.c_void_p), vp(a["out"]), a["out_cap"],
                                       vp(a["so"]), vp(a["ss"]), vp(a["fr"]), vp(a["summary"]))

    def params(**fields):
        p = hbs.mp4_protect_params(iv_size=8)
        for name, v in fields.items():
            p[name] = v
        return p

    refused = [dict(params=None), dict(params=params(iv_size=4)), dict(params=params(iv_size=24)), dict(params=params(iv_size=1)),
               dict(params=params(flags=1)), dict(params=params(reserved=(1, 0, 0, 0, 0, 0))), dict(params=params(reserved=(0, 0, 0, 0, 0, 9))),
               dict(iv=None), dict(n_frags=1 << 32), dict(n_samples=1 << 32), dict(n_frags=0), dict(so=None), dict(ss=None),
               dict(out_cap=(1 << 46) + 1), dict(frag=None), dict(d_in=None), dict(first=None), dict(sub=None), dict(summary=None),
               dict(d_in=d["d_in"].data_ptr() + 8), dict(out=out.data_ptr() + 8), dict(frag=d["frag"].data_ptr() + 8), dict(fr=fr.data_ptr() + 8),
               dict(iv=odd.data_ptr() + 8), dict(summary=odd.data_ptr() + 8), dict(first=d["first"].data_ptr() + 4), dict(sub=d["sub"].data_ptr() + 4),
               dict(so=so.data_ptr() + 4), dict(ss=ss.data_ptr() + 4)]
    for change in refused:
        assert raw(**change) == P.E_ARG, change
    torch.cuda.synchronize()
    for t in (out, so, ss, fr):
        assert (t.cpu().numpy() == CAN).all()
    assert (summary.cpu().numpy() == 0x5A).all() and (odd.cpu().numpy() == 0).all()
    assert raw() == 0 and int(ctx.read_summary(summary)["error"]) == 0                   # ... and unchanged it is accepted
    assert raw(params=params(iv_size=0), iv=None) == 0 and int(ctx.read_summary(summary)["error"]) == 0
    assert raw(out=None, out_cap=1 << 60, so=None, ss=None) == 0                          # (no d_out: out_cap is not looked at)


# ---- 7. round trips through existing calls ---------------------------------------------------------------------------------------------

def test_round_trips_and_crypt_on_either_side(ctx):
    import torch
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(61)
    b = build(ctx, rng, 200, 4)
    n, key = b["n"], bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    plain = b["d_in"].clone()
    # cenc: sequential 8-byte IVs, written by the first call
    enc_in = plain.clone()
    d_iv, _ = ctx.cenc_crypt(enc_in, b["so"], b["ss"], b["first"], b["sub"], key, iv0=bytes(range(8)))
    iv = d_iv.cpu().numpy()
    out_a, _, _, _ = run(ctx, b, 8, iv, d_in=enc_in, want=P.protect(enc_in.cpu().numpy(), b["frags"], b["first"], b["sub"], iv, 8))
    out_b, want, _, _ = run(ctx, b, 8, iv)
    out_b = out_b.clone()
    so, ss, fr = want[1], want[2], want[3]
    ctx.cenc_crypt(out_b, so, ss, b["first"], b["sub"], key, iv=iv)
    assert torch.equal(out_a, out_b) and not np.array_equal(out_b.cpu().numpy(), want[0])
    ctx.cenc_crypt(out_b, so, ss, b["first"], b["sub"], key, iv=iv)                      # and back: every mdat as it was
    assert np.array_equal(out_b.cpu().numpy(), want[0])
    # the independent walker on the device's output: the IVs and entries that went in
    got = [x for g in P.walk_protected(out_a.cpu().numpy(), 8) for x in g["samples"]]
    assert [bytes(v) for v, _ in got] == [bytes(iv[16 * s:16 * s + 8]) for s in range(n)]
    assert [e for _, e in got] == [[tuple(x) for x in b["sub"][int(b["first"][s]):int(b["first"][s + 1])].tolist()] for s in range(n)]
    # hbs_mp4_samples on the output: this call's sample tables, the times and flags of the input
    o2, z2, d2, p2, f2, fr2, _ = ctx.mp4_samples(out_a, seg=fr)
    o1, z1, d1, p1, f1, fr1, _ = ctx.mp4_samples(b["d_in"], seg=b["frags"])
    assert np.array_equal(o2, so) and np.array_equal(z2, ss) and np.array_equal(o1, b["so"]) and np.array_equal(z1, ss)
    assert np.array_equal(d1, d2) and np.array_equal(p1, p2) and np.array_equal(f1, f2)
    for name in ("out_off", "out_bytes", "decode_time", "samples", "sequence", "flags"):
        assert np.array_equal(fr2[name], fr[name]) and (name in ("out_off", "out_bytes") or np.array_equal(fr1[name], fr[name])), name
    # cbcs: no IV in the senc, the constant IV of the tenc
    civ = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    enc_in = plain.clone()
    ctx.cbcs_crypt(enc_in, b["so"], b["ss"], b["first"], b["sub"], key, iv0=civ)
    assert not torch.equal(enc_in, plain)
    out_a, _, _, _ = run(ctx, b, 0, None, d_in=enc_in, want=P.protect(enc_in.cpu().numpy(), b["frags"], b["first"], b["sub"], None, 0))
    out_b, want, _, _ = run(ctx, b, 0, None)
    out_b = out_b.clone()
    ctx.cbcs_crypt(out_b, want[1], want[2], b["first"], b["sub"], key, iv0=civ)
    assert torch.equal(out_a, out_b)
    ctx.cbcs_crypt(out_b, want[1], want[2], b["first"], b["sub"], key, iv0=civ, decrypt=True)
    assert np.array_equal(out_b.cpu().numpy(), want[0])
    assert hbs.mp4_protect_bytes(1, 2, 0) == 53 + 3 + 12


# ---- 8. large offsets -------------------------------------------------------------------------------------------------------------------

def test_fragments_around_input_offset_4gib(ctx):
    """the fragments of a small build copied to both sides of 2^32 of a 4.3 GiB buffer that is otherwise untouched; one lies across"""
    import torch
    rng = np.random.default_rng(62)
    b = build(ctx, rng, 60, 4, max_nal=900)
    G, total = 1 << 32, (1 << 32) + (300 << 20)
    big = torch.empty(total, dtype=torch.uint8, device="cuda")
    frags = b["frags"].copy()
    Rn = len(frags)
    sizes = frags["out_bytes"].astype(np.int64)
    mid = Rn // 2
    at = G - int(sizes[:mid].sum()) - 7 * mid - int(sizes[mid]) // 2        # fragment `mid` lies across 2^32
    for r in range(Rn):
        old, z = int(frags["out_off"][r]), int(sizes[r])
        o = at if r + 1 < Rn else total - z
        big[o:o + z] = b["d_in"][old:old + z]
        frags["out_off"][r] = o
        at = o + z + 7
    assert int(frags["out_off"][mid]) < G < int(frags["out_off"][mid] + frags["out_bytes"][mid]) and int(frags["out_off"][0]) > G - (64 << 20)
    iv = ivs(rng, b["n"], 8)
    want = P.protect(b["data"], b["frags"], b["first"], b["sub"], iv, 8)      # the same fragments where they were: the output is the same
    run(ctx, dict(b, d_in=big, frags=frags), 8, iv, want=want, nbytes=total)
    fails(ctx, dict(b, d_in=big, frags=frags), 8, iv, P.E_ARG, [0, Rn, 0], nbytes=total - 1)


def test_output_above_4gib(ctx):
    """two fragments of one sample of about 2.2 GiB: 2^32 of the input, and of the output, lies inside the second one's mdat; the
    moofs are compared on the host, the mdats on the device"""
    import torch
    rng = np.random.default_rng(63)
    pay = [(2200 << 20) + 5, (2200 << 20) + 77]
    head = 88 + 16 + 8
    offs = [3, 3 + head + pay[0] + 21]
    total = offs[1] + head + pay[1]
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    d_in = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda", generator=g)
    frags = np.zeros(2, dtype=R.FRAG)
    heads = []
    for r in range(2):
        h = R.one_fragment(40 + r, 1, 9000 * r, [(3000, 0x02000000, 0, b"")])
        h = bytearray(h[:head])
        h[92:96] = struct.pack(">I", pay[r])              # the trun entry's size word
        h[104:108] = struct.pack(">I", 8 + pay[r])        # the mdat's
        heads.append(bytes(h))
        d_in[offs[r]:offs[r] + head] = torch.from_numpy(np.frombuffer(bytes(h), dtype=np.uint8).copy()).cuda()
        frags[r] = (offs[r], head + pay[r], 70 + r, 9000 * r, 1, 40 + r, 1, 0)
    first = np.array([0, 2, 5], dtype=np.uint64)
    sub = np.array([(65535, 0), (100, pay[0] - 65635), (9, 1 << 31), (0, 7), (50, pay[1] - 66 - (1 << 31))], dtype=P.SUBSAMPLE)
    iv = ivs(rng, 2, 16)
    M = [P.moof_size(1, 2, 16), P.moof_size(1, 3, 16)]
    out_at = [0, M[0] + 8 + pay[0]]
    need = out_at[1] + M[1] + 8 + pay[1]
    assert out_at[1] < 1 << 32 < min(total, need) - (100 << 20) and need == total - 3 - 21 + 2 * 53 + 2 * 19 + 6 * 5
    b = dict(d_in=d_in, data=np.zeros(0, dtype=np.uint8), frags=frags, first=first, sub=sub)
    d = put(b, 16, iv, nbytes=total)
    want_s = P.summary(0, 2, 2, 5, need)
    assert summary_dict(call(ctx, d, None, None, None, None)) == want_s
    out, so, ss, fr = canary(need), canary(16), canary(16), canary(2 * FRAG)
    assert summary_dict(call(ctx, d, out, so, ss, fr, out_cap=need)) == want_s
    for r in range(2):
        moof = P.new_moof(heads[r][:104], 16, [2, 3][r:r + 1], [tuple(x) for x in sub[int(first[r]):int(first[r + 1])].tolist()], iv[16 * r:16 * r + 16])
        assert bytes(out[out_at[r]:out_at[r] + M[r]].cpu().numpy()) == moof
        assert torch.equal(out[out_at[r] + M[r]:out_at[r] + M[r] + 8 + pay[r]], d_in[offs[r] + 104:offs[r] + head + pay[r]])
    assert (out[need:].cpu().numpy() == CAN).all()
    assert so.cpu().numpy()[:16].view(np.uint64).tolist() == [out_at[r] + M[r] + 8 for r in range(2)] and ss.cpu().numpy()[:16].view(np.uint64).tolist() == pay
    got = fr.cpu().numpy()[:2 * FRAG].view(R.FRAG)
    assert got["out_off"].tolist() == out_at and got["out_bytes"].tolist() == [M[r] + 8 + pay[r] for r in range(2)]
    assert got[["first_au", "decode_time", "samples", "sequence", "flags", "reserved"]].tolist() == frags[["first_au", "decode_time", "samples", "sequence", "flags", "reserved"]].tolist()
    for t in (so, ss, fr):
        assert (t.cpu().numpy()[(16 if t is not fr else 2 * FRAG):] == CAN).all()
    # one byte short, at this size
    assert summary_dict(call(ctx, d, out, so, ss, fr, out_cap=need - 1)) == dict(want_s, error=P.E_CAPACITY)


# ---- 9. back to back on one context -----------------------------------------------------------------------------------------------------

def test_the_chain_twice_on_one_context():
    """fragment, subsample table, protect, crypt on one live context, twice: the second time with more of everything, so that the
    scratch grows between the calls"""
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    try:
        rng = np.random.default_rng(64)
        held = []
        for n_aus, V in ((40, 8), (700, 16)):
            b = build(c, rng, n_aus, 4)
            iv = ivs(rng, n_aus, V)
            out, want, _, _ = run(c, b, V, iv)
            out = out.clone()
            key = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
            c.cenc_crypt(out, want[1], want[2], b["first"], b["sub"], key, iv=iv)
            assert not np.array_equal(out.cpu().numpy(), want[0])
            c.cenc_crypt(out, want[1], want[2], b["first"], b["sub"], key, iv=iv)
            assert np.array_equal(out.cpu().numpy(), want[0])
            held.append(c.device_bytes())
        assert held[1] > held[0]
    finally:
        c.close()


# ---- 10. HIP graphs ---------------------------------------------------------------------------------------------------------------------

def test_one_replay_from_a_graph(ctx):
    """captured on a side stream after one warm-up call on contents 0, replayed on contents 1 and 0 of the same buffers: other
    fragments of the same counts"""
    import torch
    rng = np.random.default_rng(65)
    cases = []
    for i in range(2):
        case = random_case(rng, 210, max_nal=800, keep_some=False, irap_every=1000)
        cases.append(build(ctx, rng, case=case, flags=0, max_samples=7))
    assert len(cases[0]["frags"]) == len(cases[1]["frags"]) == 30 and len(cases[0]["data"]) != len(cases[1]["data"])
    iv = [ivs(rng, 210, 8) for _ in range(2)]
    want = [P.protect(b["data"], b["frags"], b["first"], b["sub"], iv[i], 8) for i, b in enumerate(cases)]
    nbytes = max(len(b["data"]) for b in cases)
    cap = max(w[4]["stream_bytes"] for w in want) + 100
    bufs = dict(d_in=torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), frag=torch.zeros(30 * FRAG, dtype=torch.uint8, device="cuda"),
                first=torch.zeros(211 * 8, dtype=torch.uint8, device="cuda"), sub=torch.zeros(max(len(b["sub"]) for b in cases) * 8, dtype=torch.uint8, device="cuda"),
                iv=torch.zeros(210 * 16, dtype=torch.uint8, device="cuda"))
    out, so, ss, fr = canary(cap), canary(210 * 8), canary(210 * 8), canary(30 * FRAG)
    from hevcbitstream_amd.api import SUMMARY
    import hevcbitstream_amd as hbs
    summary = torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device="cuda")
    prm = hbs.mp4_protect_params(iv_size=8)

    def launch():
        return ctx.mp4_protect_async(bufs["d_in"], nbytes, bufs["frag"], 30, bufs["first"], bufs["sub"], bufs["iv"], 210, prm, out, summary,
                                     sample_off=so, sample_size=ss, frag_out=fr, out_cap=cap)

    def load(i):
        b = cases[i]
        for name, a in (("d_in", b["data"]), ("frag", b["frags"]), ("first", b["first"]), ("sub", b["sub"]), ("iv", iv[i])):
            a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            bufs[name][:len(a)].copy_(torch.from_numpy(a.copy()))
        for t in (out, so, ss, fr):
            t.fill_(CAN)
        summary.fill_(0x5A)

    def check(i):
        assert summary_dict(ctx.read_summary(summary)) == want[i][4]
        check_outputs(out, so, ss, fr, want[i])

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
