"""hbs_mp4_senc_samples on the GPU against the plain loop of tests/_mp4_senc_ref.py, value for value: plan first, then a run into
outputs of exactly the planned size with canaries behind d_sub, d_sub_first and d_iv, every summary field checked.  Inputs are
made by hbs_mp4_fragment, hbs_cenc_subsamples and hbs_mp4_protect on small synthetic streams, or patched on the host from those,
or written by hand.  A plan workgroup takes 256 fragments or samples (kSencLanes: hbs_mp4senc.h), scan_parts 2 048 workgroups a
pass (hbs_plan.h), an entry workgroup 256 entries a step."""
import struct

import numpy as np
import pytest

from tests import _mp4_protect_ref as P
from tests import _mp4_read_ref as RR
from tests import _mp4_ref as R
from tests import _mp4_senc_ref as S
from tests._mp4_ref import random_case
from tests.test_gpu_mp4_protect import build, dev, ivs, summary_dict
from tests.test_mp4_senc_ref import error_cases, foreign

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
W = 256
PASS = 256 * 8


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


def canary(n):
    import torch
    return torch.full((n + PAD,), CAN, dtype=torch.uint8, device="cuda")


def call(ctx, d, first, sub, iv, sub_cap=None, fill=0x5A):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), fill, dtype=torch.uint8, device="cuda")
    rc = ctx.mp4_senc_samples_async(d["d_in"], d["nbytes"], d["frag"], d["R"], d["size"], d["N"], d["prm"], first, sub, iv, summary, sub_cap=sub_cap)
    assert rc == 0, rc
    return summary_dict(ctx.read_summary(summary))


def put(d_in, nbytes, frags, sizes, V, track_id=0, flags=0, n_samples=None):
    import hevcbitstream_amd as hbs
    N = int(frags["samples"].sum()) if n_samples is None else n_samples
    return dict(d_in=d_in, nbytes=nbytes, frag=dev(frags), R=len(frags), size=dev(np.asarray(sizes, dtype=np.uint64)) if sizes is not None else None,
                N=N, V=V, prm=hbs.mp4_senc_params(iv_size=V, track_id=track_id, flags=flags))


def check_tables(first, sub, iv, want, N, V):
    w_first, w_sub, w_iv, s = want
    E = s["nal_count"]
    p = first.cpu().numpy()
    assert np.array_equal(p[:(N + 1) * 8].view(np.uint64), w_first), "d_sub_first"
    assert (p[(N + 1) * 8:] == CAN).all(), "stored behind d_sub_first"
    if sub is not None:
        p = sub.cpu().numpy()
        got = p[:E * 8].view(S.SUBSAMPLE)
        bad = np.flatnonzero(got != w_sub)
        assert not len(bad), "d_sub differs at entry %d of %d: got %s want %s" % (bad[0], E, got[bad[0]], w_sub[bad[0]])
        assert (p[E * 8:] == CAN).all(), "stored behind d_sub"
    p = iv.cpu().numpy()
    if V:
        assert np.array_equal(p[:16 * N], w_iv), "d_iv"
        assert (p[16 * N:] == CAN).all(), "stored behind d_iv"
    else:
        assert (p == CAN).all(), "d_iv touched with iv_size 0"


def run(ctx, d, want):
    """plan, then a run into outputs of exactly the planned size; everything against `want` (the loop's results) -> the summary"""
    N, V = d["N"], d["V"]
    want_s = want[3]
    assert want_s["error"] == 0, want_s
    first, iv = canary((N + 1) * 8), canary(16 * N)
    s = call(ctx, d, first, None, iv)
    assert s == want_s
    check_tables(first, None, iv, want, N, V)
    E = s["nal_count"]
    first, sub, iv = canary((N + 1) * 8), canary(E * 8), canary(16 * N)
    s = call(ctx, d, first, sub, iv, sub_cap=E)
    assert s == want_s
    check_tables(first, sub, iv, want, N, V)
    return s


def fails(ctx, d, want_s, sub_cap=1 << 16):
    """a plan and a run that must report want_s and store nothing but the summary"""
    N = d["N"]
    first, sub, iv = canary((N + 1) * 8), canary(sub_cap * 8), canary(16 * N)
    for plan in (True, False):
        if plan and want_s["error"] == S.E_CAPACITY:
            continue
        assert call(ctx, d, first, None if plan else sub, iv, sub_cap=None if plan else sub_cap) == want_s
    for t in (first, sub, iv):
        assert (t.cpu().numpy() == CAN).all(), "stored on an error"


def protected(ctx, b, V, iv):
    """the protected fragments of a build, by the library -> (device bytes, host bytes, FRAG table, sample sizes)"""
    out, so, ss, fr, _ = ctx.mp4_protect(b["d_in"], b["frags"], b["first"], b["sub"], iv=iv if V else None, iv_size=V)
    return out, out.cpu().numpy(), fr, ss


def want_of(b, V, iv):
    """what went into hbs_mp4_protect, in the form the reader returns it"""
    N = len(b["first"]) - 1
    prot = int(b["sub"]["protect"].astype(np.uint64).sum())
    return b["first"], b["sub"], (iv[:16 * N] if V else np.zeros(16 * N, np.uint8)), None, prot


# ---- 1. round trips -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ("mixed", "a_fragment_a_sample", "one_fragment"))
@pytest.mark.parametrize("V", (8, 16, 0))
def test_round_trip(ctx, V, shape):
    rng = np.random.default_rng(700 + V + len(shape))
    prm = dict(mixed=dict(), a_fragment_a_sample=dict(max_samples=1), one_fragment=dict(flags=0, max_samples=0))[shape]
    case = random_case(rng, 300, max_nal=400, keep_some=False, irap_every=1000 if shape == "one_fragment" else 25)
    b = build(ctx, rng, case=case, **prm)
    Rn = len(b["frags"])
    assert dict(mixed=Rn > 5, a_fragment_a_sample=Rn == 300 > W, one_fragment=Rn == 1 and int(b["frags"]["samples"][0]) == 300 > W)[shape]
    iv = ivs(rng, b["n"], V)
    d_out, host, fr, ss = protected(ctx, b, V, iv)
    want = S.senc_samples(host, fr, ss, V)
    w = want_of(b, V, iv)
    assert np.array_equal(want[0], w[0]) and np.array_equal(want[1], w[1]) and np.array_equal(want[2], w[2]) and want[3]["rbsp_bytes"] == w[4]
    s = run(ctx, put(d_out, len(host), fr, None, V), want)
    assert s["reserved"] == [0, 0, Rn] and s["nal_found"] == 300 and s["stream_bytes"] == len(host)
    # the table hbs_mp4_samples writes for the protected bytes names the same fragments
    so2, ss2, _, _, _, fr2, _ = ctx.mp4_samples(d_out)
    assert np.array_equal(fr2["out_off"], fr["out_off"]) and np.array_equal(fr2["samples"], fr["samples"]) and np.array_equal(ss2, ss)
    run(ctx, put(d_out, len(host), fr2, ss2, V), want)


# ---- 2. the decrypt loop --------------------------------------------------------------------------------------------------------------

def test_decrypt_loop_cenc(ctx):
    rng = np.random.default_rng(720)
    b = build(ctx, rng, 200, 4)
    key, iv0 = bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, 8, dtype=np.uint8))
    clear = b["d_in"].clone()
    d_iv, _ = ctx.cenc_crypt(b["d_in"], b["so"], b["ss"], b["first"], b["sub"], key, iv0=iv0)
    iv = d_iv.cpu().numpy()[:16 * b["n"]]
    assert not np.array_equal(b["d_in"].cpu().numpy(), clear.cpu().numpy())
    d_out, so, ss, fr, _ = ctx.mp4_protect(b["d_in"], b["frags"], b["first"], b["sub"], iv=iv, iv_size=8)
    # a reader that has only the protected bytes
    so2, ss2, _, _, _, fr2, _ = ctx.mp4_samples(d_out)
    first, sub, riv, s = ctx.mp4_senc_samples(d_out, fr2, sample_size=ss2, iv_size=8)
    assert int(s["nal_count"]) == len(b["sub"]) and np.array_equal(riv.cpu().numpy(), iv)
    ctx.cenc_crypt(d_out, so2, ss2, first, sub, key, iv=riv)
    want = P.protect(clear.cpu().numpy(), b["frags"], b["first"], b["sub"], iv, 8)[0]
    assert np.array_equal(d_out.cpu().numpy(), want)


@pytest.mark.parametrize("V", (0, 16))
def test_decrypt_loop_cbcs(ctx, V):
    rng = np.random.default_rng(730 + V)
    b = build(ctx, rng, 200, 4)
    key, civ = bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    iv = ivs(rng, b["n"], 16)
    kw = dict(iv=iv) if V else dict(iv0=civ)
    clear = b["d_in"].clone()
    want = P.protect(clear.cpu().numpy(), b["frags"], b["first"], b["sub"], iv if V else None, V)[0]
    ctx.cbcs_crypt(b["d_in"], b["so"], b["ss"], b["first"], b["sub"], key, crypt_byte_block=1, skip_byte_block=9, **kw)
    d_out, _, _, _, _ = ctx.mp4_protect(b["d_in"], b["frags"], b["first"], b["sub"], iv=iv if V else None, iv_size=V)
    enc = d_out.cpu().numpy().copy()
    assert not np.array_equal(enc, want)
    so2, ss2, _, _, _, fr2, _ = ctx.mp4_samples(d_out)
    first, sub, riv, _ = ctx.mp4_senc_samples(d_out, fr2, sample_size=ss2, iv_size=V)
    back = dict(iv=riv) if V else dict(iv0=civ)
    ctx.cbcs_crypt(d_out, so2, ss2, first, sub, key, decrypt=True, crypt_byte_block=1, skip_byte_block=9, **back)
    assert np.array_equal(d_out.cpu().numpy(), want)
    # and the other direction with the tables read back: the encrypted bytes again
    ctx.cbcs_crypt(d_out, so2, ss2, first, sub, key, crypt_byte_block=1, skip_byte_block=9, **back)
    assert np.array_equal(d_out.cpu().numpy(), enc)


# ---- 3. the hint against the walk -------------------------------------------------------------------------------------------------------

def test_hint_against_walk(ctx):
    rng = np.random.default_rng(740)
    b = build(ctx, rng, 200, 4)
    V = 8
    iv = ivs(rng, b["n"], V)
    _, host, fr, ss = protected(ctx, b, V, iv)
    want = S.senc_samples(host, fr, ss, V)
    assert want[3]["error"] == 0 and len(fr) > 5
    saiz = [int(fr["out_off"][r]) + 88 + 16 * int(fr["samples"][r]) for r in range(len(fr))]
    assert all(bytes(host[a + 4:a + 8]) == b"saiz" for a in saiz)
    forms = [host.copy() for _ in range(4)]
    for a in saiz:
        forms[1][a + 4:a + 8] = np.frombuffer(b"free", dtype=np.uint8)          # the serial path everywhere
    mid = len(fr) // 2
    forms[2][saiz[mid] + 17 + int(fr["samples"][mid]) // 2] ^= 6                  # one size byte of a middle fragment
    forms[3][saiz[mid] + 16] ^= 1                                                 # a sample_count off by one
    got = [run(ctx, put(dev(x), len(x), fr, None, V), want) for x in forms]
    assert got[0] == got[1] == got[2] == got[3]


# ---- 4. other packagers' forms -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", (0, 8, 16))
def test_foreign_fragments(ctx, V):
    data, fr, sizes, _, read = foreign(V)
    want = S.senc_samples(data, fr, sizes, V, track_id=1)
    s = run(ctx, put(dev(np.frombuffer(data, dtype=np.uint8)), len(data), fr, sizes, V, track_id=1), want)
    assert s["reserved"] == [0, 0, read]
    # track_id 0 takes the first traf; without sizes the senc without flag 2 offends
    for kw, sz in ((dict(track_id=0), sizes), (dict(track_id=1), None)):
        ws = S.senc_samples(data, fr, sz, V, **kw)[3]
        assert ws["error"] == S.E_ARG
        fails(ctx, put(dev(np.frombuffer(data, dtype=np.uint8)), len(data), fr, sz, V, **kw), ws)


def test_clear_if_absent(ctx):
    sizes = [0, 1, 65535, 65536, 200000]
    data, fr = S.frag_table([S.fragment([S.traf(1, sizes[:2])]), S.fragment([S.traf(1, sizes[2:], RR.box(b"saio", bytes(12)))])], [2, 3])
    d_in = dev(np.frombuffer(data, dtype=np.uint8))
    want = S.senc_samples(data, fr, sizes, 8, flags=S.CLEAR_IF_ABSENT)
    assert want[0].tolist() == [0, 0, 1, 2, 4, 8]
    run(ctx, put(d_in, len(data), fr, sizes, 8, flags=S.CLEAR_IF_ABSENT), want)
    fails(ctx, put(d_in, len(data), fr, sizes, 8), S.senc_samples(data, fr, sizes, 8)[3])
    sizes[3] = 1 << 32
    ws = S.senc_samples(data, fr, sizes, 8, flags=S.CLEAR_IF_ABSENT)[3]
    assert ws["reserved"] == [4, 0, 0]
    fails(ctx, put(d_in, len(data), fr, sizes, 8, flags=S.CLEAR_IF_ABSENT), ws)


def test_a_sample_of_300_entries_among_ordinary_ones(ctx):
    """300 entries are more than a workgroup of entry lanes and more than a saiz byte can say: the fragment has no saiz"""
    rng = np.random.default_rng(750)
    V = 16
    mk = lambda n: (bytes(rng.integers(1, 256, 16, dtype=np.uint8)), [(int(rng.integers(0, 60)), int(rng.integers(0, 900))) for _ in range(n)])   # noqa: E731
    a = [mk(int(rng.integers(0, 5))) for _ in range(20)]
    b = [mk(2), mk(300), mk(1), mk(0), mk(3)]
    c = [mk(int(rng.integers(0, 5))) for _ in range(30)]
    size = lambda x: [sum(p + q for p, q in e) for _, e in x]          # noqa: E731
    blobs = [S.fragment([S.traf(1, size(x), *(() if x is b else (S.saiz_box(V, x),)), S.senc_box(V, x))]) for x in (a, b, c)]
    data, fr = S.frag_table(blobs, [20, 5, 30], gap=7)
    want = S.senc_samples(data, fr, None, V)
    first = want[0]
    assert want[3]["nal_count"] > W + 100 and int(first[21]) < W < int(first[22])          # the long sample crosses a workgroup of entry lanes
    run(ctx, put(dev(np.frombuffer(data, dtype=np.uint8)), len(data), fr, None, V), want)


def test_fragments_apart_out_of_order_and_at_the_end_of_the_allocation(ctx):
    import torch
    rng = np.random.default_rng(760)
    b = build(ctx, rng, 200, 4)
    V = 8
    iv = ivs(rng, b["n"], V)
    _, host, fr, ss = protected(ctx, b, V, iv)
    Rn = len(fr)
    total = 6 << 20
    buf = rng.integers(0, 256, size=total, dtype=np.uint8)
    fr2 = fr.copy()
    at = total
    for r in range(Rn):                                                  # fragment 0 ends with the allocation, the others lie in front of it, in reverse
        z, old = int(fr["out_bytes"][r]), int(fr["out_off"][r])
        at -= z + (0 if r == 0 else int(rng.integers(0, 50)))
        buf[at:at + z] = host[old:old + z]
        fr2["out_off"][r] = at
    assert int(fr2["out_off"][0] + fr2["out_bytes"][0]) == total and len({int(x) % 16 for x in fr2["out_off"]}) > 4
    torch.cuda.empty_cache()                                             # (no cached block to cut the allocation from)
    d_in = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_in.copy_(torch.from_numpy(buf))
    want = S.senc_samples(buf, fr2, ss, V)
    assert np.array_equal(want[1], b["sub"])
    run(ctx, put(d_in, total, fr2, None, V), want)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(error_cases())), ids=[c[0].replace(" ", "_") for c in error_cases()])
def test_errors(ctx, i):
    name, data, fr, sizes, kw, reserved = error_cases()[i]
    ws = S.senc_samples(data, fr, sizes, 8, **kw)[3]
    assert ws["error"] == S.E_ARG and ws["reserved"] == reserved
    fails(ctx, put(dev(np.frombuffer(data, dtype=np.uint8)), len(data), fr, sizes, 8, **kw), ws)


def test_capacity_one_short(ctx):
    rng = np.random.default_rng(770)
    b = build(ctx, rng, 200, 4)
    iv = ivs(rng, b["n"], 8)
    d_out, host, fr, ss = protected(ctx, b, 8, iv)
    E = len(b["sub"])
    ws = S.senc_samples(host, fr, None, 8, sub_cap=E - 1)[3]
    assert ws["error"] == S.E_CAPACITY and ws["nal_count"] == E and ws["rbsp_bytes"] == int(b["sub"]["protect"].sum())
    fails(ctx, put(d_out, len(host), fr, None, 8), ws, sub_cap=E - 1)


def test_refused_at_once(ctx):
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import SUMMARY
    data, fr, sizes, _, _ = foreign(8)
    d = put(dev(np.frombuffer(data, dtype=np.uint8)), len(data), fr, sizes, 8, track_id=1)
    first, iv = canary((d["N"] + 1) * 8), canary(16 * d["N"])
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    good = [d["d_in"], d["nbytes"], d["frag"], d["R"], d["size"], d["N"], d["prm"], first, None, iv, summary]

    def refused(**kw):
        names = ("data", "in_bytes", "frag", "n_frags", "sample_size", "n_samples", "params", "sub_first", "sub", "iv", "summary")
        args = [kw.get(n, g) for n, g in zip(names, good)]
        assert ctx.mp4_senc_samples_async(*args) == S.E_ARG, kw

    for prm in (hbs.mp4_senc_params(iv_size=4), hbs.mp4_senc_params(flags=2)):
        refused(params=prm)
    prm = hbs.mp4_senc_params()
    prm["reserved"][0][4] = 1
    refused(params=prm)
    refused(n_frags=1 << 32)
    refused(n_samples=1 << 32)
    refused(n_frags=0)
    refused(iv=None)
    refused(sub_first=None)
    refused(summary=None)
    refused(in_bytes=(1 << 62) + 1)
    for name in ("data", "frag", "iv", "summary"):
        refused(**{name: torch.zeros(4096, dtype=torch.uint8, device="cuda")[8:]})
    refused(sample_size=torch.zeros(4096, dtype=torch.uint8, device="cuda")[4:])
    refused(sub_first=torch.zeros(4096, dtype=torch.uint8, device="cuda")[4:])
    refused(sub=torch.zeros(4096, dtype=torch.uint8, device="cuda")[4:])
    torch.cuda.synchronize()
    for t in (first, iv):
        assert (t.cpu().numpy() == CAN).all()
    assert (summary.cpu().numpy() == 0x5A).all()


# ---- 6. a scan that takes more than one pass ----------------------------------------------------------------------------------------------

def test_more_samples_than_one_pass_of_the_scan(ctx):
    """524 289 samples: one more than 2 048 workgroups of 256.  One template fragment of 3 samples, tiled by numpy; the loop's result
    for the tiling is the template's, repeated, with the entry offsets moved on"""
    V = 8
    iv = lambda k: bytes([k] * 8) + bytes(8)          # noqa: E731
    smp = [(iv(1), [(5, 20)]), (iv(2), []), (iv(3), [(3, 0), (0, 7)])]
    one = S.fragment([S.traf(1, [25, 0, 10], S.saiz_box(V, smp), S.senc_box(V, smp))])
    n = 174763
    assert 3 * n == PASS * W + 1
    t_first, t_sub, t_iv, t_s = S.senc_samples(one, S.frag_table([one], [3])[1], None, V)
    assert t_first.tolist() == [0, 1, 1, 3]
    data = np.tile(np.frombuffer(one, dtype=np.uint8), n)
    fr = np.zeros(n, dtype=R.FRAG)
    fr["out_off"], fr["out_bytes"], fr["samples"] = np.arange(n, dtype=np.uint64) * np.uint64(len(one)), len(one), 3
    fr["first_au"] = 3 * np.arange(n, dtype=np.uint64) + 11
    first = np.concatenate([(t_first[:3][None, :] + (3 * np.arange(n, dtype=np.uint64))[:, None]).reshape(-1), [3 * n]]).astype(np.uint64)
    want = (first, np.tile(t_sub, n), np.tile(t_iv, n), S.summary(0, 3 * n, 3 * n, 27 * n, len(data), senc_read=n))
    d = put(dev(data), len(data), fr, None, V)
    run(ctx, d, want)
    # the same through the serial walk: a saiz that counts another number of samples
    at = one.index(b"saiz") + 12
    data2 = data.reshape(n, len(one)).copy()
    data2[:, at] ^= 1
    run(ctx, put(dev(data2.reshape(-1)), len(data), fr, None, V), want)


# ---- 7. HIP graphs ------------------------------------------------------------------------------------------------------------------------

def test_one_replay_from_a_graph(ctx):
    """captured on a side stream after one warm-up call on contents 0, replayed on contents 1 and 0 of the same buffers: other
    fragments of the same counts"""
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(780)
    V = 8
    cases = []
    for i in range(2):
        b = build(ctx, rng, case=random_case(rng, 210, max_nal=800, keep_some=False, irap_every=1000), flags=0, max_samples=7)
        iv = ivs(rng, 210, V)
        _, host, fr, ss = protected(ctx, b, V, iv)
        if i:                                                            # the second contents take the serial path in one fragment
            host = host.copy()
            host[int(fr["out_off"][3]) + 88 + 16 * 7 + 16] ^= 1
        cases.append((host, fr, S.senc_samples(host, fr, None, V)))
    assert all(len(c[1]) == 30 for c in cases) and len(cases[0][0]) != len(cases[1][0])
    nbytes = max(len(c[0]) for c in cases)
    cap = max(c[2][3]["nal_count"] for c in cases)
    d_in, d_frag = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros(30 * R.FRAG.itemsize, dtype=torch.uint8, device="cuda")
    first, sub, iv = canary(211 * 8), canary(cap * 8), canary(210 * 16)
    summary = torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device="cuda")
    prm = hbs.mp4_senc_params(iv_size=V)

    def launch():
        return ctx.mp4_senc_samples_async(d_in, nbytes, d_frag, 30, None, 210, prm, first, sub, iv, summary, sub_cap=cap)

    def load(i):
        host, fr, _ = cases[i]
        d_in.zero_()
        d_in[:len(host)].copy_(torch.from_numpy(host.copy()))
        d_frag.copy_(torch.from_numpy(np.ascontiguousarray(fr).view(np.uint8).reshape(-1).copy()))
        for t in (first, sub, iv):
            t.fill_(CAN)
        summary.fill_(0x5A)

    def check(i):
        want = cases[i][2]
        assert summary_dict(ctx.read_summary(summary)) == dict(want[3], stream_bytes=nbytes)
        check_tables(first, sub, iv, want, 210, V)

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


# ---- 8. empty calls -----------------------------------------------------------------------------------------------------------------------

def test_empty_calls(ctx):
    d = put(dev(np.zeros(0, np.uint8)), 0, np.zeros(0, dtype=R.FRAG), None, 8)
    run(ctx, d, S.senc_samples(b"", np.zeros(0, R.FRAG), None, 8))
    fr = np.zeros(2, dtype=R.FRAG)
    fr["out_off"], fr["out_bytes"] = [0, 8], [8, 3]
    data = np.frombuffer(b"x" * 11, dtype=np.uint8)
    run(ctx, put(dev(data), 11, fr, None, 8), S.senc_samples(data, fr, None, 8))
    fr["out_bytes"][1] = 4
    fails(ctx, put(dev(data), 11, fr, None, 8), S.senc_samples(data, fr, None, 8)[3])
