"""hbs_au_times on the GPU against tests/_au_times_ref.py (one sort per segment, every pair of a segment for the spans), entry for
entry: a plan, then a run into tables of exactly n_aus entries with canaries behind each, every summary field checked.  AU tables
are fabricated as ACCESS_UNIT records; the fields the call does not read hold random bytes.  No tolerances: every comparison is
exact.  B = 256 AUs a workgroup, H = 64 AUs of halo on either side in the rank kernel (kAutLanes, kAutHalo: hbs_autimes.h)."""
import ctypes as C

import numpy as np
import pytest

from tests import _au_times_ref as T

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 1024
B, H = 256, 64
PASS = 256 * 8                  # workgroups the scans over workgroups take in one step (kPlanLanes * kPlanPer: hbs_plan.h)
TABLES = (("dts", 8, np.uint64), ("pts", 8, np.uint64), ("order", 4, np.uint32), ("display", 4, np.uint32))
LO, HI = -(1 << 31), (1 << 31) - 1


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


def canary(n):
    import torch
    return torch.full((n + PAD,), CAN, dtype=torch.uint8, device="cuda")


def call(ctx, d_au, n, kw, outs=None, rc=0):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    got = ctx.au_times_async(d_au, n, T.params_record(**kw), summary, **(outs or {}))
    assert got == rc, got
    if rc:
        assert (summary.cpu().numpy() == 0x5A).all(), "a refused call wrote the summary"
        return None
    return ctx.read_summary(summary)


def summary_matches(s, want):
    got = dict(error=int(s["error"]), nal_count=int(s["nal_count"]), nal_found=int(s["nal_found"]), rbsp_bytes=int(s["rbsp_bytes"]),
               stream_bytes=int(s["stream_bytes"]), stop_reason=int(s["stop_reason"]), reserved=[int(x) for x in s["reserved"]])
    assert got == want


def make_outs(n, which=None):
    return {name: canary(n * size) for name, size, _ in TABLES if which is None or name in which}


def check_outs(outs, want, n):
    for name, size, dt in TABLES:
        if name not in outs:
            continue
        p = outs[name].cpu().numpy()
        got = p[: n * size].view(dt)
        bad = np.flatnonzero(got != want[name])
        assert not len(bad), "%s differs at AU %d of %d: %d, want %d (%d differ)" % (name, bad[0], n, got[bad[0]], want[name][bad[0]], len(bad))
        assert (p[n * size:] == CAN).all(), "stored behind d_" + name


def run(ctx, au, want=None, **kw):
    """the plan, then all four tables at exactly n_aus entries; everything against the reference -> the reference's answer"""
    want = want if want is not None else T.au_times(au, **kw)
    assert want["summary"]["error"] == 0
    n = len(au)
    d_au = dev(au)
    summary_matches(call(ctx, d_au, n, kw), want["summary"])
    outs = make_outs(n)
    summary_matches(call(ctx, d_au, n, kw, outs), want["summary"])
    check_outs(outs, want, n)
    return want


def refused_in_the_summary(ctx, au, lowest, **kw):
    """HBS_E_DEPTH with the lowest offending AU, from the plan and from a run; the tables keep their canaries"""
    want = T.au_times(au, **kw)["summary"]
    assert want == dict(nal_count=0, nal_found=0, rbsp_bytes=0, stream_bytes=0, stop_reason=0, error=T.E_DEPTH, reserved=[1 + lowest, 0, 0])
    d_au = dev(au)
    summary_matches(call(ctx, d_au, len(au), kw), want)
    outs = make_outs(len(au))
    summary_matches(call(ctx, d_au, len(au), kw, outs), want)
    for name, t in outs.items():
        assert (t.cpu().numpy() == CAN).all(), "d_%s written in spite of the error" % name


# ---- sizes, heads at the edges of wavefronts and workgroups -------------------------------------------------------------------

@pytest.mark.parametrize("n", (0, 1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1))
def test_sizes(ctx, n):
    rng = np.random.default_rng(100 + n)
    want = run(ctx, T.table(T.pyramid(8, n // 8 + 1)[:n], junk=rng), tick=3003, base_time=90000)
    assert want["summary"]["reserved"][1] == (3 if n > 8 else 0)
    run(ctx, T.table(rng.integers(-3, 3, n).tolist(), heads=[a for a in (1, 64, B) if a < n], junk=rng), delay=5)


@pytest.mark.parametrize("heads", ([B - 1], [B], [B - 1, B], [63], [64], [63, 64, 2 * B - 1, 2 * B], [], list(range(3 * B))),
                         ids=("last-of-a-workgroup", "first-of-the-next", "both", "lane-63", "lane-64", "several", "one-segment", "every-AU"))
def test_heads_at_edges(ctx, heads):
    """`one-segment` is one segment over three workgroups with no head but AU 0"""
    rng = np.random.default_rng(200 + len(heads))
    pocs = T.pyramid(16, 3 * B // 16 + 1)[:3 * B]
    want = run(ctx, T.table(pocs, heads=heads, junk=rng))
    assert want["summary"]["nal_found"] == len(set(heads) | {0})
    # falling keys across every head: nothing moves across it
    keys = (10000 - np.arange(3 * B) // 7).tolist()
    run(ctx, T.table(keys, heads=heads, junk=rng), tick=7)


# ---- inversions across a workgroup edge, from LDS into memory -----------------------------------------------------------------

def test_pyramid_straddles_a_workgroup_edge(ctx):
    for gop in (8, 32, 64):
        pocs = T.pyramid(gop, 3 * B // gop + 1)[:3 * B]       # AU 0 is the IDR: every GOP ends one AU behind a multiple of gop
        want = run(ctx, T.table(pocs), tick=1001)
        assert want["order"].tolist() == np.argsort(np.argsort(pocs)).tolist() and want["summary"]["reserved"][1] == gop.bit_length() - 1


@pytest.mark.parametrize("lower", (H, H + 1, H + 40))
def test_walks_leave_the_halo_in_both_directions(ctx, lower):
    """a high key on the last AU of workgroup 0 with `lower` lower keys behind it: from H + 1 on its forward walk leaves what the
    workgroup staged; a high key `lower` AUs in front of the first AU of workgroup 2: from H + 1 on that AU's backward walk does"""
    rng = np.random.default_rng(300 + lower)
    au = T.table([0] * (B - 1) + [500] + list(range(1, lower + 1)) + [600] * 40, junk=rng)
    back, fwd = T.spans(au)
    assert int(fwd[B - 1]) == lower == int(back[B - 1 + lower])
    want = run(ctx, au)
    assert int(want["order"][B - 1]) == B - 1 + lower
    au = T.table([0] * (2 * B - lower) + [900] + list(range(1, lower + 1)) + [1000] * 30, junk=rng)
    back, fwd = T.spans(au)
    assert int(back[2 * B]) == lower == int(fwd[2 * B - lower])
    want = run(ctx, au)
    assert int(want["order"][2 * B]) == 2 * B - 1 and want["summary"]["reserved"][1] == 1


def test_a_head_cuts_the_walk(ctx):
    """a high key just in front of a CVS_START is not counted behind it, at a workgroup edge and inside one"""
    for at in (B, B + 1, 100):
        keys = [5] * (at - 1) + [900] + [1, 2, 3] + [5] * 50
        want = run(ctx, T.table(keys, heads=[at]))
        assert want["order"].tolist()[at - 1:at + 3] == [at - 1, at, at + 1, at + 2] and want["summary"]["reserved"][1] == 0
        moved = run(ctx, T.table(keys))
        assert int(moved["order"][at - 1]) == len(keys) - 1 and moved["summary"]["reserved"][1] == at


# ---- the span limit -----------------------------------------------------------------------------------------------------------

def span_tables(span):
    """[(table, the lowest AU that offends when span is above the limit)]: forwards, backwards behind a cut, inside the second
    segment of a table whose first segment is long"""
    return [(T.table([0] * 10 + [9] + [1] * span + [50] * 40), 10),
            (T.table([0] * 10 + [3] * span + [1] + [5] * 40), 10),
            (T.table([3] * 300 + [7] + [5] * span + [9] * 5, heads=[200]), 300),
            (T.table([4] * (B - 1) + [8] + [6] * (span - 1) + [5] + [9] * 3, heads=[B - 1]), B - 1)]


def test_span_of_exactly_the_limit(ctx):
    for au, _ in span_tables(T.MAX_SPAN):
        back, fwd = T.spans(au)
        assert max(int(back.max()), int(fwd.max())) == T.MAX_SPAN
        run(ctx, au, tick=2)


def test_span_above_the_limit(ctx):
    for au, lowest in span_tables(T.MAX_SPAN + 1):
        back, fwd = T.spans(au)
        assert max(int(back.max()), int(fwd.max())) == T.MAX_SPAN + 1
        refused_in_the_summary(ctx, au, lowest)
    # the same with a head in the way is no error
    au, _ = span_tables(T.MAX_SPAN + 1)[0]
    au["flags"][500] |= T.CVS_START
    run(ctx, au)


# ---- more workgroups than one step of the scan over workgroups ----------------------------------------------------------------

def test_more_workgroups_than_one_step_of_the_parts_scan(ctx):
    rng = np.random.default_rng(400)
    n = PASS * B + 3 * B + 17
    keys = np.asarray(T.near_sorted(rng, n, reach=16))
    heads = np.unique(rng.integers(0, n, n // 60))
    edge = PASS * B
    heads = heads[(heads < edge - 40) | (heads > edge + 40)].tolist()         # one segment runs across the step's edge ...
    nopic = list(range(edge - 3, edge + 5)) + rng.integers(0, n, 2000).tolist()       # ... and so does a run of AUs without a picture
    keys[edge - 4] += 14                                                      # ... whose key is inverted against what follows
    au = T.table(keys.tolist(), heads=heads, nopic=nopic, junk=rng)
    back, fwd = T.spans(au)
    assert max(int(back.max()), int(fwd.max())) <= 64
    want = run(ctx, au, tick=3003, base_time=1 << 40)
    assert int(want["order"][edge - 4]) > edge and want["summary"]["nal_found"] == len(set(heads) | {0})


# ---- keys ---------------------------------------------------------------------------------------------------------------------

def test_keys(ctx):
    rng = np.random.default_rng(500)
    run(ctx, T.table([HI, LO, HI, LO, 0, -1, 1, HI, LO, LO, HI] * 40, junk=rng))
    run(ctx, T.table(rng.integers(-4, 4, 3 * B).tolist(), heads=[B + 3], junk=rng))                      # ties
    run(ctx, T.table(rng.integers(LO, LO + 3, 2 * B).tolist(), junk=rng))
    keys = T.near_sorted(rng, 3 * B, reach=20)
    for nopic in (range(0, 5), range(0, B + 9), range(B - 3, B + 9), range(3 * B - 9, 3 * B), range(0, 3 * B), sorted(rng.integers(0, 3 * B, 90).tolist())):
        run(ctx, T.table(keys, nopic=nopic, junk=rng))
        run(ctx, T.table(keys, heads=[B, B + 4, 2 * B - 1], nopic=nopic, junk=rng))     # heads without a picture: ranked by the same formula


# ---- delay and wrap -----------------------------------------------------------------------------------------------------------

def test_delay_given_below_at_and_above(ctx):
    au = T.table(T.pyramid(16, 40), heads=[161, 322])
    R = T.au_times(au)["summary"]["reserved"][1]
    assert R == 4
    for d in (0, R - 1, R, R + 1, 1000):
        want = run(ctx, au, tick=3003, delay=d)
        assert (want["summary"]["reserved"][2] > 0) == (d < R) and want["summary"]["reserved"][0] == d
        assert (d < R) == any(p < t for p, t in zip(want["exact_pts"], want["exact_dts"]))


def test_wrap33(ctx):
    au = T.table(T.pyramid(8, 70))
    for base in ((1 << 33) - 3003 * 5 - 1, (1 << 33) - 1, (1 << 34) + 5, 0):
        want = run(ctx, au, tick=3003, base_time=base, flags=T.WRAP33)
        assert int(want["dts"].max()) < 1 << 33 and int(want["pts"].max()) < 1 << 33
        assert (base > 0) == (max(want["exact_pts"]) >= 1 << 33)
    run(ctx, au, tick=3003, base_time=(1 << 33) - 1, flags=T.WRAP33, delay=2)


# ---- outputs and buffers ------------------------------------------------------------------------------------------------------

def test_each_output_alone(ctx):
    rng = np.random.default_rng(600)
    au = T.table(T.pyramid(32, 20), heads=[300], junk=rng)
    n = len(au)
    kw = dict(tick=1500, base_time=77)
    want = T.au_times(au, **kw)
    d_au = dev(au)
    for which in (("dts",), ("pts",), ("order",), ("display",), ("dts", "pts"), ("order", "display"), ("pts", "display")):
        outs = make_outs(n, which)
        summary_matches(call(ctx, d_au, n, kw, outs), want["summary"])
        check_outs(outs, want, n)


def test_every_alignment_the_abi_accepts(ctx):
    """the AU table and the summary at a multiple of 16 that is no multiple of 32, the times at 8, the slots at 4"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(700)
    au = T.table(T.pyramid(8, 80)[:2 * B + 5], heads=[B + 1], junk=rng)
    n = len(au)
    want = T.au_times(au, tick=9)
    raw = np.concatenate([np.full(16, CAN, dtype=np.uint8), au.view(np.uint8)])
    d_raw = dev(raw)
    summary = torch.full((16 + SUMMARY.itemsize + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    outs, views = {}, {}
    for name, size, _ in TABLES:
        outs[name] = canary(size + n * size)
        views[name] = outs[name][size:]
        assert views[name].data_ptr() % (2 * size) == size
    assert d_raw[16:].data_ptr() % 32 == 16
    assert ctx.au_times_async(d_raw[16:], n, T.params_record(tick=9), summary[16:], **views) == 0
    s = summary.cpu().numpy()
    assert (s[:16] == 0x5A).all() and (s[16 + SUMMARY.itemsize:] == 0x5A).all()
    summary_matches(s[16:16 + SUMMARY.itemsize].view(SUMMARY)[0], want["summary"])
    for name, size, dt in TABLES:
        p = outs[name].cpu().numpy()
        assert (p[:size] == CAN).all() and (p[size + n * size:] == CAN).all(), "stored outside d_" + name
        assert np.array_equal(p[size:size + n * size].view(dt), want[name]), name


def test_a_gop_cut_is_a_pointer_offset(ctx):
    rng = np.random.default_rng(800)
    au = T.table(T.pyramid(8, 100), heads=[401], junk=rng)
    d_au = dev(au)
    first, n = 401, len(au) - 401
    want = T.au_times(au[first:], tick=5)
    outs = make_outs(n)
    summary_matches(call(ctx, d_au[first * 64:], n, dict(tick=5), outs), want["summary"])
    check_outs(outs, want, n)


# ---- at-once refusals ---------------------------------------------------------------------------------------------------------

def test_refused_at_once(ctx):
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import SUMMARY
    au = T.table(T.pyramid(8, 10))
    n = len(au)
    d_au = dev(au)
    outs = make_outs(n)
    bad = [dict(flags=4), dict(flags=1 << 31), dict(reserved=(1, 0, 0)), dict(reserved=(0, 1, 0)), dict(reserved=(0, 0, 1)), dict(tick=0),
           dict(base_time=T.LIMIT), dict(base_time=T.LIMIT - (n + T.MAX_SPAN)), dict(base_time=T.LIMIT - (n + 3) * 7, tick=7, delay=3),
           dict(tick=(1 << 32) - 1, base_time=T.LIMIT - 1, delay=(1 << 32) - 1)]
    for kw in bad:
        assert T.refused(n, **kw), kw
        call(ctx, d_au, n, kw, outs, rc=T.E_ARG)
    # ... and the values next to them are taken
    for kw in (dict(base_time=T.LIMIT - 1 - (n + T.MAX_SPAN)), dict(base_time=T.LIMIT - 1 - (n + 3) * 7, tick=7, delay=3)):
        assert not T.refused(n, **kw)
        summary_matches(call(ctx, d_au, n, kw), T.au_times(au, **kw)["summary"])
    # n_aus above 2^32 - 1 (nothing is read), a missing table
    call(ctx, d_au, 1 << 32, {}, outs, rc=T.E_ARG)
    summary = torch.full((SUMMARY.itemsize + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    prm = T.params_record()
    ptr = lambda t: C.c_void_p(t.data_ptr())         # noqa: E731
    pp = prm.ctypes.data_as(C.c_void_p)
    lib, h = ctx.lib, ctx.h
    o = [ptr(outs[name]) for name, _, _ in TABLES]
    assert lib.hbs_au_times(h, ptr(d_au), n, pp, *o, ptr(summary)) == 0
    summary.fill_(0x5A)
    assert lib.hbs_au_times(None, ptr(d_au), n, pp, *o, ptr(summary)) == T.E_ARG
    assert lib.hbs_au_times(h, None, n, pp, *o, ptr(summary)) == T.E_ARG
    assert lib.hbs_au_times(h, ptr(d_au), n, None, *o, ptr(summary)) == T.E_ARG
    assert lib.hbs_au_times(h, ptr(d_au), n, pp, *o, None) == T.E_ARG
    # misaligned pointers, one at a time
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)      # noqa: E731
    assert lib.hbs_au_times(h, off(d_au, 8), n - 1, pp, *o, ptr(summary)) == T.E_ARG
    assert lib.hbs_au_times(h, ptr(d_au), n, pp, *o, off(summary, 8)) == T.E_ARG
    for i, k in ((0, 4), (1, 4), (2, 2), (3, 1)):
        shifted = list(o)
        shifted[i] = off(outs[TABLES[i][0]], k)
        assert lib.hbs_au_times(h, ptr(d_au), n, pp, *shifted, ptr(summary)) == T.E_ARG
    torch.cuda.synchronize()
    assert (summary.cpu().numpy() == 0x5A).all()
    for name, t in outs.items():
        t.fill_(CAN)
    # n_aus == 0 needs no table; the delay passes through
    summary_matches(call(ctx, None, 0, dict(delay=9), make_outs(0)), T.au_times(T.table([]), delay=9)["summary"])
    assert hbs.AUT_MAX_SPAN == T.MAX_SPAN


# ---- random -------------------------------------------------------------------------------------------------------------------

def test_random_near_sorted(ctx):
    rng = np.random.default_rng(900)
    n = 100000 + 77
    keys = T.near_sorted(rng, n, reach=60)
    heads = np.unique(rng.integers(0, n, 700)).tolist()
    nopic = np.unique(rng.integers(0, n, 3000)).tolist()
    au = T.table(keys, heads=heads, nopic=nopic, junk=rng)
    back, fwd = T.spans(au)
    assert 32 < max(int(back.max()), int(fwd.max())) <= 64          # the reference alone says the table is inside the limit
    want = run(ctx, au, tick=1001, base_time=12345)
    assert want["summary"]["reserved"][1] > 8 and not np.array_equal(want["order"], np.arange(n))


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def test_end_to_end_from_a_stream_to_mp4_and_ts(ctx):
    import hevcbitstream_amd as hbs
    from tests.hevc_synth import stream_4k30
    from tests.test_gpu_au import parse_stream
    stream, n = stream_4k30(9, n_pictures=96, slices_per_picture=2, idr_every=32, payload_bytes=(60, 200))
    d, got, index, parsed, cc, structs = parse_stream(ctx, stream, n)
    assert got == n
    au, nal_au, s, _ = ctx.access_units(index, parsed, cc, structs, got)
    assert len(au) == 96 and int(s["reserved"][1]) == 3
    # the generator draws every slice_pic_order_cnt_lsb at random: the table as it came, whatever order that is ...
    assert run(ctx, au, tick=2)["summary"]["nal_found"] == 3
    # ... and, as it codes no reordered pictures of its own, with a GOP-8 pyramid in every coded video sequence
    for s0 in (0, 32, 64):
        au["pic_order_cnt"][s0:s0 + 32] = T.pyramid(8, 4)[:32]
    want = T.au_times(au, tick=3003, base_time=900000)
    assert want["summary"]["reserved"][1] == 3 and want["summary"]["nal_found"] == 3
    dts, pts, order, display, s = ctx.au_times(au, tick=3003, base_time=900000)
    summary_matches(s, want["summary"])
    for name, t in (("dts", dts), ("pts", pts), ("order", order), ("display", display)):
        assert np.array_equal(t.cpu().numpy().view(want[name].dtype), want[name]), name
    # fragments with these times, and the sample table read back from them
    idx = index[: got * 32]
    out, so, ss, frags, _ = ctx.mp4_fragment(d, idx, nal_au, au, dts=dts, pts=pts, flags=hbs.MP4_CUT_AT_IRAP, sample_duration=3003, track_id=1)
    assert len(frags) == 3
    got_tables = ctx.mp4_samples(out, seg=frags, track_id=1)
    assert np.array_equal(got_tables[2], want["dts"]) and np.array_equal(got_tables[3], want["pts"])
    # the transport multiplexer takes the same tables modulo 2^33
    dts33, pts33, _, _, s33 = ctx.au_times(au, tick=3003, base_time=(1 << 33) - 3003 * 40, flags=hbs.AUT_WRAP33)
    w33 = T.au_times(au, tick=3003, base_time=(1 << 33) - 3003 * 40, flags=T.WRAP33)
    assert np.array_equal(pts33.cpu().numpy().view(np.uint64), w33["pts"]) and int(w33["pts"].min()) < 3003 * 60
    ts, au_packet, s_ts = ctx.ts_mux(d, au, pts=pts33, dts=dts33)
    assert int(s_ts["error"]) == 0 and len(au_packet) == 97 and ts.numel() % 188 == 0 and ts.numel() > 0


# ---- HIP graph ----------------------------------------------------------------------------------------------------------------

def test_one_replay_from_a_graph_on_another_table(ctx):
    """captured on a side stream after one warm-up call, replayed on other contents of the same buffers: another table of the same
    n_aus, with other heads and another R; every host argument is the same"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(1000)
    n = 3 * B + 11
    tables = [T.table(T.pyramid(8, n)[:n], heads=[B - 1], junk=rng), T.table(T.pyramid(32, n)[:n], heads=[70, B, B + 1], nopic=[0, 1, B], junk=rng)]
    kw = dict(tick=3003, base_time=5)
    wants = [T.au_times(t, **kw) for t in tables]
    assert wants[0]["summary"] != wants[1]["summary"]
    d_au = dev(tables[0])
    outs = make_outs(n)
    summary = torch.full((SUMMARY.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
    prm = T.params_record(**kw)

    def launch():
        return ctx.au_times_async(d_au, n, prm, summary, **outs)

    def check(want):
        summary_matches(ctx.read_summary(summary), want["summary"])
        check_outs(outs, want, n)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert launch() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    check(wants[0])
    held = ctx.device_bytes()
    for which in (1, 0):
        d_au.copy_(torch.from_numpy(tables[which].view(np.uint8).reshape(-1).copy()))
        for t in outs.values():
            t.fill_(CAN)
        summary.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        check(wants[which])
    assert ctx.device_bytes() == held
