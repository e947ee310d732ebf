"""hbs_ts_demux on the GPU against the plain loop of tests/_ts_ref.py: plan first, then a run into outputs of exactly the planned
capacity with canaries behind them, every summary field checked."""
import numpy as np
import pytest

from tests import _ts_ref as R
from tests._carve import carve

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
BLOCK = 2048
PID = 0x100


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).cuda() if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda")


def canary(n):
    import torch
    return torch.full((n + PAD,), CAN, dtype=torch.uint8, device="cuda")


def summary_matches(s, want):
    assert int(s["error"]) == want["error"], (s, want)
    assert int(s["rbsp_bytes"]) == 0 and int(s["stop_reason"]) == 0
    assert int(s["reserved"][0]) == want["reserved"][0]
    if want["error"] != R.E_ARG:
        for k in ("nal_count", "nal_found", "stream_bytes"):
            assert int(s[k]) == want[k], (k, s, want)
        assert [int(x) for x in s["reserved"]] == want["reserved"], (s, want)


def call(ctx, d_ts, nbytes, B, pid, out, pes, out_cap=None, pes_cap=None):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = ctx.ts_demux_async(d_ts, nbytes, B, pid, out, pes, summary, out_cap=out_cap, pes_cap=pes_cap)
    assert rc == 0, rc
    return ctx.read_summary(summary)


def run(ctx, ts, B, pid=PID, d_ts=None, with_pes=True):
    """plan, then a run into outputs of exactly the planned capacity; everything against the plain loop.  -> (out, pes, summary)"""
    ts = np.ascontiguousarray(ts).reshape(-1)
    want_out, want_pes, want = R.demux(ts, B, pid)
    if d_ts is None:
        d_ts = dev(ts)
    s = call(ctx, d_ts, len(ts), B, pid, None, None)
    summary_matches(s, want)
    if want["error"]:
        return None, None, s
    need, n_pes = int(s["stream_bytes"]), int(s["nal_count"])
    out = canary(need)
    pes = canary(n_pes * 32) if with_pes else None
    s = call(ctx, d_ts, len(ts), B, pid, out, pes, out_cap=need, pes_cap=n_pes)
    summary_matches(s, want)
    o = out.cpu().numpy()
    bad = np.flatnonzero(o[:need] != want_out)
    assert len(bad) == 0, "output differs at %d (of %d), %d bytes in all" % (bad[0], need, len(bad))
    assert (o[need:] == CAN).all(), "stored behind the output"
    if with_pes:
        p = pes.cpu().numpy()
        got_pes = p[: n_pes * 32].view(R.TS_PES)
        assert np.array_equal(got_pes, want_pes), [(k, a, b) for k, (a, b) in enumerate(zip(got_pes, want_pes)) if a != b][:3]
        assert (p[n_pes * 32:] == CAN).all(), "stored behind the PES table"
    return o[:need], want_pes, s


COUNTS = (0, 1, 255, 256, 257, 2047, 2048, 2049, 3 * BLOCK + 7)


@pytest.mark.parametrize("B", R.SIZES)
def test_packet_counts(ctx, B):
    rng = np.random.default_rng(B)
    for k, n in enumerate(COUNTS):
        share = (1.0, 0.9)[k % 2]
        run(ctx, R.random_ts(rng, n, B, PID, share=share, first_pes=0 if n else None, p_break=0.02), B)
        run(ctx, R.random_ts(rng, n, B, PID, share=share, first_pes=min(3, n - 1) if n else None, lens="full"), B)


def test_more_blocks_than_one_scan_pass(ctx):
    """70 blocks and a packet, and 300 blocks (the scan takes 256 a pass): sums, the first PES start and the continuity
    join carried from pass to pass"""
    rng = np.random.default_rng(70)
    run(ctx, R.random_ts(rng, 70 * BLOCK + 1, 188, PID, share=0.9, first_pes=40 * BLOCK + 5, p_break=0.01), 188)
    run(ctx, R.random_ts(rng, 300 * BLOCK + 1, 192, PID, share=0.02, first_pes=258 * BLOCK + 77, p_break=0.05, p_pes=0.2), 192)


@pytest.mark.parametrize("B", R.SIZES)
@pytest.mark.parametrize("share", (1.0, 0.9, 0.02, 0.0))
def test_share_of_the_pid(ctx, B, share):
    rng = np.random.default_rng(int(share * 100) + B)
    n = 3 * BLOCK + 7
    _, pes, s = run(ctx, R.random_ts(rng, n, B, PID, share=share, first_pes=9 if share else None, p_break=0.05), B)
    assert (int(s["nal_found"]) == 0) == (share == 0.0)
    if share >= 0.9:
        assert len(pes) > 0 and int(s["reserved"][1]) > 0 and int(s["reserved"][2]) > 0


@pytest.mark.parametrize("first", (0, BLOCK - 1, 2 * BLOCK + 100, None))
def test_first_pes_start(ctx, first):
    rng = np.random.default_rng(11)
    for B, share in ((188, 1.0), (192, 0.5), (204, 0.9)):
        out, pes, s = run(ctx, R.random_ts(rng, 3 * BLOCK + 7, B, PID, share=share, first_pes=first, p_break=0.03), B)
        if first is None:
            assert len(out) == 0 and len(pes) == 0 and int(s["reserved"][2]) == int(s["nal_found"]) > 0
        else:
            assert int(pes["packet"][0]) == first and int(pes["out_off"][0]) == 0


def test_empty_es_parts_and_short_runs(ctx):
    """PES starts without ES bytes, payloads of a byte or two: output chunks that span many packets"""
    rng = np.random.default_rng(12)
    a = R.random_ts(rng, 2 * BLOCK + 300, 188, PID, share=1.0, p_pes=0.3, p_empty=0.9)
    run(ctx, a, 188)
    # payloads of 1..3 bytes: adaptation_field_length 180..182
    n = BLOCK + 700
    t = np.frombuffer(b"".join(R.fit(PID, rng.integers(0, 256, size=int(k), dtype=np.uint8).tobytes(), cc=i & 15)
                               for i, k in enumerate(rng.integers(1, 4, size=n))), dtype=np.uint8).copy().reshape(n, 188)
    t[0] = np.frombuffer(R.fit(PID, R.pes_header(pts=5) + b"\x01\x02", pusi=1, cc=15), dtype=np.uint8)
    out, _, _ = run(ctx, t, 188)
    assert 2 + n - 1 <= len(out) <= 2 + 3 * (n - 1)


def test_a_round_whose_output_is_under_16_bytes(ctx):
    """rounds of 256 packets that put out 3, 0, 5 and 15 bytes, between rounds that put out thousands"""
    rng = np.random.default_rng(13)
    for B in R.SIZES:
        other = R.packet(0x101, rng.integers(0, 256, size=184, dtype=np.uint8).tobytes(), B=B)
        pk, cc = [], 0

        def es(data, **kw):
            nonlocal cc
            pk.append(R.fit(PID, data, cc=cc, B=B, **kw))
            cc = (cc + 1) & 15
        es(R.pes_header(pts=1) + b"\xA1\xA2\xA3", pusi=1)
        pk += [other] * 255                                         # round 0: 3 bytes
        pk += [other] * 256                                         # round 1: nothing
        pk += [other] * 100
        es(b"\xB1\xB2\xB3\xB4\xB5")
        pk += [other] * 155                                         # round 2: 5 bytes
        for _ in range(256):                                        # round 3: full
            es(rng.integers(0, 256, size=184, dtype=np.uint8).tobytes())
        es(b"\xC1" * 7)
        pk += [other] * 200
        es(R.pes_header() + b"\xC2" * 8, pusi=1)
        pk += [other] * 54                                          # round 4: 15 bytes
        for _ in range(300):
            es(rng.integers(0, 256, size=int(rng.integers(1, 185)), dtype=np.uint8).tobytes())
        out, pes, s = run(ctx, np.frombuffer(b"".join(pk), dtype=np.uint8), B)
        assert out[:8].tobytes() == b"\xA1\xA2\xA3\xB1\xB2\xB3\xB4\xB5" and len(pes) == 2 and int(s["reserved"][1]) == 0


@pytest.mark.parametrize("at", (BLOCK, BLOCK - 1, 2 * BLOCK))
def test_continuity_across_a_block_boundary(ctx, at):
    """a break, a duplicate and a break under the discontinuity flag in the first / last packet of a block"""
    counts = {}
    for what in ("break", "dup", "break_di", None):
        rng = np.random.default_rng(14)                             # the same draws but for the event
        a = R.random_ts(rng, 2 * BLOCK + 10, 188, PID, share=1.0, first_pes=0, p_pes=0.02, cc_events=[(at, what)] if what else [])
        _, _, s = run(ctx, a, 188)
        counts[what] = int(s["reserved"][1])
    assert counts == {None: 0, "break_di": 0, "dup": 1, "break": 1}, counts
    # the join across blocks that hold no packet of the PID: events two blocks apart
    rng = np.random.default_rng(15)
    a = R.random_ts(rng, 4 * BLOCK, 204, PID, share=0.0, first_pes=None)
    for p, cc in ((5, 3), (BLOCK - 1, 4), (3 * BLOCK, 5), (3 * BLOCK + 1, 5), (4 * BLOCK - 1, 9)):
        a[p] = np.frombuffer(R.fit(PID, (R.pes_header() if p == 5 else b"") + b"\x55" * 20, pusi=1 if p == 5 else 0, cc=cc, B=204), dtype=np.uint8)
    _, _, s = run(ctx, a, 204)
    assert int(s["reserved"][1]) == 2 and int(s["nal_found"]) == 5


def test_skipped_packets(ctx):
    rng = np.random.default_rng(16)
    _, _, s = run(ctx, R.random_ts(rng, BLOCK + 50, 192, PID, share=0.8, first_pes=100, p_skip=0.3, p_nopay=0.2), 192)
    assert int(s["reserved"][2]) > 300


FAULTS = {
    "sync loss in another PID's packet": lambda t: t.__setitem__(slice(0, 3), [0x46, 0x01, 0x01]),
    "afl 184": lambda t: t.__setitem__(slice(1, 5), [0x01, 0x00, 0x30, 184]),
    "payload under 9 bytes": lambda t: t.__setitem__(slice(1, 5), [0x41, 0x00, 0x30, 175]),
    "no start code prefix": lambda t: t.__setitem__(slice(1, 7), [0x41, 0x00, 0x10, 0, 0, 2]),
    "not an MPEG-2 PES header": lambda t: t.__setitem__(slice(1, 13), [0x41, 0x00, 0x10, 0, 0, 1, 0xE0, 0, 0, 0x40, 0x00, 0]),
    "PTS_DTS_flags 01": lambda t: t.__setitem__(slice(1, 13), [0x41, 0x00, 0x10, 0, 0, 1, 0xE0, 0, 0, 0x80, 0x40, 5]),
    "header past the packet": lambda t: t.__setitem__(slice(1, 13), [0x41, 0x00, 0x10, 0, 0, 1, 0xE0, 0, 0, 0x80, 0x00, 176]),
    "PTS without room": lambda t: t.__setitem__(slice(1, 13), [0x41, 0x00, 0x10, 0, 0, 1, 0xE0, 0, 0, 0x80, 0x80, 4]),
    "PTS and DTS without room": lambda t: t.__setitem__(slice(1, 13), [0x41, 0x00, 0x10, 0, 0, 1, 0xE0, 0, 0, 0x80, 0xC0, 9]),
}


@pytest.mark.parametrize("kind", sorted(FAULTS))
def test_faults(ctx, kind):
    """one fault in the first, a middle and the last block (and two: the lowest is reported); nothing is written"""
    rng = np.random.default_rng(17)
    n = 3 * BLOCK + 7
    for B, places in ((188, [7]), (192, [BLOCK + 1000]), (204, [n - 1]), (188, [2 * BLOCK + 3, BLOCK - 1, n - 2])):
        a = R.random_ts(rng, n, B, PID, share=0.9, first_pes=2)
        _, _, clean = R.demux(a.reshape(-1), B, PID)
        for p in places:
            FAULTS[kind](a[p, R.lead(B):])
        ts = a.reshape(-1)
        _, _, want = R.demux(ts, B, PID)
        assert want["error"] == R.E_ARG and want["reserved"][0] == 1 + min(places)
        d_ts = dev(ts)
        summary_matches(call(ctx, d_ts, len(ts), B, PID, None, None), want)
        out, pes = canary(clean["stream_bytes"]), canary(clean["nal_count"] * 32)
        s = call(ctx, d_ts, len(ts), B, PID, out, pes, out_cap=clean["stream_bytes"], pes_cap=clean["nal_count"])
        summary_matches(s, want)
        assert (out.cpu().numpy() == CAN).all() and (pes.cpu().numpy() == CAN).all(), "written in spite of the fault"


def test_capacity_and_no_pes_table(ctx):
    rng = np.random.default_rng(18)
    B = 188
    ts = R.random_ts(rng, BLOCK + 500, B, PID, share=0.9, first_pes=1).reshape(-1)
    want_out, want_pes, want = R.demux(ts, B, PID)
    need, n_pes = len(want_out), len(want_pes)
    d_ts = dev(ts)
    for out_cap, pes_cap in ((need - 1, n_pes), (need, n_pes - 1), (0, 0)):
        out, pes = canary(need), canary(n_pes * 32)
        s = call(ctx, d_ts, len(ts), B, PID, out, pes, out_cap=out_cap, pes_cap=pes_cap)
        summary_matches(s, dict(want, error=R.E_CAPACITY))
        assert (out.cpu().numpy() == CAN).all() and (pes.cpu().numpy() == CAN).all(), "written in spite of the capacity"
    # without a PES table its capacity means nothing
    out = canary(need)
    s = call(ctx, d_ts, len(ts), B, PID, out, None, out_cap=need, pes_cap=0)
    summary_matches(s, want)
    assert np.array_equal(out.cpu().numpy()[:need], want_out) and (out.cpu().numpy()[need:] == CAN).all()
    run(ctx, ts, B, with_pes=False)
    # the convenience call
    o, p, s = ctx.ts_demux(d_ts, PID, B)
    assert np.array_equal(o.cpu().numpy(), want_out) and np.array_equal(p, want_pes)


def test_argument_refusals(ctx):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    ts = R.random_ts(np.random.default_rng(19), 300, 188, PID).reshape(-1)
    big = torch.zeros(len(ts) + 64, dtype=torch.uint8, device="cuda")
    big[16:16 + len(ts)] = dev(ts)
    d_ts = big[16:16 + len(ts)]
    out, pes = canary(300 * 184), canary(300 * 32)
    summary = torch.full((SUMMARY.itemsize + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(ts=d_ts, n=len(ts), B=188, pid=PID, out=out, pes=pes, s=summary[:SUMMARY.itemsize])
    for change in (dict(B=187), dict(B=0), dict(B=208), dict(pid=-1), dict(pid=8192), dict(n=len(ts) - 1), dict(n=len(ts) + 4, B=192),
                   dict(ts=big[17:17 + len(ts)]), dict(ts=big[24:24 + len(ts)]), dict(out=out[8:]), dict(pes=pes[4:]), dict(s=summary[8:8 + SUMMARY.itemsize])):
        a = dict(good, **change)
        rc = ctx.ts_demux_async(a["ts"], a["n"], a["B"], a["pid"], a["out"], a["pes"], a["s"], out_cap=300 * 184, pes_cap=300)
        assert rc == -3, (change, rc)
    rc = ctx.lib.hbs_ts_demux(ctx.h, d_ts.data_ptr(), len(ts), 188, PID, None, 0, None, 0, None)
    assert rc == -3
    torch.cuda.synchronize()
    assert (summary.cpu().numpy() == 0x5A).all() and (out.cpu().numpy() == CAN).all() and (pes.cpu().numpy() == CAN).all()
    assert ctx.ts_demux_async(good["ts"], good["n"], 188, PID, out, pes, good["s"], out_cap=300 * 184, pes_cap=300) == 0


@pytest.mark.parametrize("offset", (16, 48, 1008, 4080))
def test_carved_input_between_hostile_bytes(ctx, offset):
    """d_ts 16 bytes and more off a page boundary, inside an allocation full of sync bytes and PES starts of the PID; a stream
    whose size is no multiple of 16, so that its last granule holds bytes that are not its own"""
    rng = np.random.default_rng(offset)
    hostile = R.fit(PID, R.pes_header(pts=77) + b"\x47" * 60, pusi=1, cc=1)
    for B, n in ((188, 257), (204, BLOCK + 3), (192, 255)):
        ts = R.random_ts(rng, n, B, PID, share=0.9, first_pes=1).reshape(-1)
        view, chk = carve(len(ts), offset, fill=hostile)
        chk.put(ts)
        chk.hostile(front=hostile * 4, back=hostile * 4)
        run(ctx, ts, B, d_ts=view)
        assert chk.intact(), chk.damage()


def parse_stream(ctx, d, n):
    """index + header parse of the Annex-B stream in the device tensor d, which holds n NAL units"""
    import torch
    from hevcbitstream_amd.api import COMPACT, PARSED, SUMMARY
    cap = n + 8
    index = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    parsed = torch.zeros(cap * PARSED.itemsize, dtype=torch.uint8, device="cuda")
    cc = torch.zeros(cap * COMPACT.itemsize, dtype=torch.uint8, device="cuda")
    structs = torch.zeros(8 << 20, dtype=torch.uint8, device="cuda")
    ss, ps = (torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2))
    got = ctx.index_parse_compact_async(d, index, cap, parsed, cc, structs, ss, ps)
    assert int(ctx.read_summary(ps)["error"]) == 0
    return got, index, parsed, cc, structs


def test_pipeline_ts_to_access_units(ctx):
    """hevc_synth pictures muxed one access unit per PES packet: demux gives the stream byte for byte, index + parse + access
    units of it give AUs whose unit_begin are the out_off of the PES table, the times are what the muxer stamped"""
    from tests.hevc_synth import Synth, annexb
    g = Synth(3, rich=False)
    rng = np.random.RandomState(4)
    units, n_nals, times = [], 0, []
    for pic in range(60):
        nals = []
        if pic % 20 == 0:
            nals += [g.vps(), g.sps_nal(1920, 1080, ctb_log2=6), g.pps_nal(force={"tiles": 0})]
        for sl in range(4):
            pay = rng.randint(0, 256, size=int(rng.randint(30, 900))).astype(np.uint8).tobytes()
            nals.append(g.slice_nal(19 if pic % 20 == 0 else 1, first=(sl == 0), payload=pay, address=sl * 120, tid=1))
        units.append(annexb(nals))
        n_nals += len(nals)
        times.append((90000 + 3003 * (pic + 2), 90000 + 3003 * pic if pic % 2 else None))
    stream = b"".join(units)
    for B in R.SIZES:
        ts, begins = R.mux_units(units, PID, B, times, np.random.default_rng(B))
        import hevcbitstream_amd as hbs
        assert hbs.ts_find_pid(ts[: 16 * B], B) == (PID, 1)
        out, pes, s = ctx.ts_demux(dev(np.frombuffer(ts, dtype=np.uint8)), PID, B)
        assert out.cpu().numpy().tobytes() == stream
        assert int(s["nal_count"]) == 60 and int(s["reserved"][1]) == 0 and pes["packet"].tolist() == begins
        n, index, parsed, cc, structs = parse_stream(ctx, out, n_nals)
        assert n == n_nals
        au, _, _, _ = ctx.access_units(index, parsed, cc, structs, n)
        assert len(au) == 60 and au["unit_begin"].tolist() == pes["out_off"].tolist()
        assert pes["pts"].tolist() == [t[0] for t in times] and pes["dts"].tolist() == [t[1] if t[1] is not None else t[0] for t in times]
        assert all(int(f) & R.F_PTS and int(f) & R.F_ALIGN for f in pes["flags"])
        assert [bool(int(f) & R.F_DTS) for f in pes["flags"]] == [t[1] is not None for t in times]
