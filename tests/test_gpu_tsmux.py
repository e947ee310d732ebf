"""hbs_ts_mux on the GPU against the plain loop of tests/_tsmux_ref.py, byte for byte: plan first, then a run into outputs of
exactly the planned capacity with canaries behind d_out and d_au_packet, every summary field checked; then the way back
through hbs_ts_demux on the device."""
import numpy as np
import pytest

from tests import _ts_ref as D
from tests import _tsmux_ref as R
from tests import _carve as K
from tests._tsmux_ref import random_case

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
BLOCK = 2048                    # output packets of a copy workgroup
PLAN = 256                      # AUs of a plan workgroup; the scan takes 2048 workgroups a pass


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


def summary_matches(s, want):
    assert int(s["error"]) == want["error"], (s, want)
    assert int(s["stop_reason"]) == 0 and int(s["nal_found"]) == want["nal_found"]
    assert int(s["reserved"][0]) == want["reserved"][0], (s, want)
    if want["error"] != R.E_ARG:
        for k in ("nal_count", "rbsp_bytes", "stream_bytes"):
            assert int(s[k]) == want[k], (k, s, want)
        assert [int(x) for x in s["reserved"]] == want["reserved"], (s, want)


def call(ctx, d, out, au_packet, out_cap=None):
    """d: the device inputs of a case (put)"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = ctx.ts_mux_async(d["stream"], d["nbytes"], d["au"], d["n"], d["pts"], d["dts"], d["prm"], out, au_packet, summary, out_cap=out_cap)
    assert rc == 0, rc
    return ctx.read_summary(summary)


def put(stream, au, pts, dts, prm, d_stream=None):
    return dict(stream=dev(stream) if d_stream is None else d_stream, nbytes=len(stream), au=dev(au), n=len(au),
                pts=dev(pts) if pts is not None else None, dts=dev(dts) if dts is not None else None, prm=R.params_record(prm))


def run(ctx, stream, au, pts, dts, prm, d_stream=None, want=None):
    """plan, then a run into outputs of exactly the planned capacity; everything against the plain loop.
    -> (out, au_packet, summary, device inputs)"""
    want_out, want_ap, want_s = want if want is not None else R.mux(stream, au, pts, dts, prm)
    d = put(stream, au, pts, dts, prm, d_stream)
    s = call(ctx, d, None, None)
    summary_matches(s, want_s)
    assert want_s["error"] == 0
    need, n = int(s["stream_bytes"]), len(au)
    out, ap = canary(need), canary((n + 1) * 4)
    s = call(ctx, d, out, ap, out_cap=need)
    summary_matches(s, want_s)
    o = out.cpu().numpy()
    bad = np.flatnonzero(o[:need] != want_out)
    assert len(bad) == 0, "output differs at byte %d (packet %d, byte %d of it; %d bytes of %d differ)" % (
        bad[0], bad[0] // prm["packet_bytes"], bad[0] % prm["packet_bytes"], len(bad), need)
    assert (o[need:] == CAN).all(), "stored behind the output"
    p = ap.cpu().numpy()
    assert np.array_equal(p[: (n + 1) * 4].view(np.uint32), want_ap), "d_au_packet"
    assert (p[(n + 1) * 4:] == CAN).all(), "stored behind d_au_packet"
    return out[:need], want_ap, s, d


def untouched_on_error(ctx, d, want_s, cap_bytes, n, out_cap):
    """the plan and a run both report want_s; the canary-filled outputs are untouched"""
    summary_matches(call(ctx, d, None, None), dict(want_s, error=want_s["error"] if want_s["error"] == R.E_ARG else 0))
    out, ap = canary(cap_bytes), canary((n + 1) * 4)
    summary_matches(call(ctx, d, out, ap, out_cap=out_cap), want_s)
    assert (out.cpu().numpy() == CAN).all() and (ap.cpu().numpy() == CAN).all(), "written in spite of the error"


COUNTS = (0, 1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 7)


@pytest.mark.parametrize("B", R.SIZES)
def test_au_counts(ctx, B):
    rng = np.random.default_rng(B)
    for k, n in enumerate(COUNTS):
        prm = R.params(packet_bytes=B, flags=(0, R.PCR, R.PCR | R.PSI_AT_IRAP, R.NO_PSI)[k % 4], cc_es=k % 16, cc_pat=(k * 5) % 16, cc_pmt=(k * 3) % 16,
                       pcr_lead=1000 * k)
        stream, au, pts, dts = random_case(rng, n, prm, max_es=420)
        run(ctx, stream, au, pts, dts, prm)


def edge_sizes(f, pcr):
    H, R1 = {0: 9, 2: 14, 3: 19}[f], 184 - (8 if pcr else 2)
    return [0] + [T - H for T in (R1 - 1, R1, R1 + 1, R1 + 183, R1 + 184, R1 + 185, R1 + 2 * 184)]


@pytest.mark.parametrize("B", R.SIZES)
def test_packet_count_edges(ctx, B):
    """the single packet, and a last packet with 1, 183 (a lone length byte) and 184 (no adaptation field) bytes, for each
    time form with and without a PCR; and an AU without ES bytes"""
    rng = np.random.default_rng(40 + B)
    for flags in (0, R.PCR):
        sizes, pts, dts = [], [], []
        for f in (0, 2, 3):
            for E in edge_sizes(f, bool(flags) and f != 0):
                sizes.append(E)
                pts.append(R.NO_TIME if f == 0 else int(rng.integers(0, 1 << 33)))
                dts.append(R.NO_TIME if f != 3 else (pts[-1] + 1) & R.MASK33)
        sizes = np.array(sizes)
        begins = np.concatenate([[0], np.cumsum(sizes[:-1])])
        stream = rng.integers(0, 256, size=int(sizes.sum()), dtype=np.uint8)
        prm = R.params(packet_bytes=B, flags=flags, pcr_lead=77)
        au = R.aus(begins, begins + sizes, np.arange(len(sizes)) % 2 == 0)
        _, ap, _, _ = run(ctx, stream, au, np.array(pts, dtype=np.uint64), np.array(dts, dtype=np.uint64), prm)
        assert int(ap[0]) == 2 and np.diff(ap).tolist() == [1, 1, 1, 2, 2, 2, 3, 3] * 3        # E = 0, then T = R1 - 1 .. R1 + 2 * 184


def test_every_source_alignment(ctx):
    """unit_begin takes all 16 residues modulo 16, for AUs of several packets"""
    rng = np.random.default_rng(50)
    sizes = rng.integers(400, 1200, size=64)
    begins, at = [], 0
    for k, size in enumerate(sizes):
        at += (k % 16 - at) % 16 + 16 * int(rng.integers(0, 3))
        begins.append(at)
        at += int(size)
    begins = np.array(begins)
    assert sorted(set(begins % 16)) == list(range(16))
    stream = rng.integers(0, 256, size=at, dtype=np.uint8)
    for B in R.SIZES:
        run(ctx, stream, R.aus(begins, begins + sizes), None, None, R.params(packet_bytes=B))


def test_gaps_between_aus_and_the_end_of_the_allocation(ctx):
    """gaps of 0, 1, 15, 16, 17 and 100 000 bytes; the last AU ends at stream_bytes, and the stream is a 12 MiB allocation of
    its own, so that its last byte is the allocation's last"""
    import torch
    rng = np.random.default_rng(51)
    total = 12 << 20
    gaps = [0, 1, 15, 16, 17, 100000] * 20
    sizes = rng.integers(0, 3000, size=len(gaps))
    begins = np.cumsum(np.array(gaps) + np.concatenate([[0], sizes[:-1]]))
    ends = begins + sizes
    shift = total - int(ends[-1])
    assert shift >= 0
    begins, ends = begins + shift, ends + shift
    stream = rng.integers(0, 256, size=total, dtype=np.uint8)
    torch.cuda.empty_cache()                                    # (no cached block to cut the 12 MiB from)
    d_stream = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_stream.copy_(torch.from_numpy(stream))
    for B, last in ((188, 0), (192, 1), (204, 17)):
        ends[-1] = total
        begins[-1] = total - 3000 - last
        prm = R.params(packet_bytes=B, flags=R.PCR)
        pts = (np.arange(len(gaps), dtype=np.uint64) * 3003) & np.uint64(R.MASK33)
        run(ctx, stream, R.aus(begins, ends), pts, None, prm, d_stream=d_stream)


def test_one_au_larger_than_a_workgroups_range(ctx):
    rng = np.random.default_rng(52)
    E = 176 - 14 + 184 * (3 * BLOCK + 6)
    stream = rng.integers(0, 256, size=E + 300, dtype=np.uint8)
    au = R.aus([5, 5 + E, 5 + E + 40], [5 + E, 5 + E + 33, 5 + E + 200], [1, 0, 1])
    for B in R.SIZES:
        prm = R.params(packet_bytes=B, flags=R.PSI_AT_IRAP, cc_es=11)
        _, ap, _, _ = run(ctx, stream, au, np.array([90000, 93003, 96006], dtype=np.uint64), None, prm)
        assert ap.tolist() == [2, 2 + 3 * BLOCK + 7, 2 + 3 * BLOCK + 7 + 1 + 2, 2 + 3 * BLOCK + 7 + 1 + 2 + 1]


def test_many_one_packet_aus(ctx):
    """5 000 AUs of one packet each: every packet has stuffing"""
    rng = np.random.default_rng(53)
    for B, flags in ((188, R.PCR), (204, 0)):
        prm = R.params(packet_bytes=B, flags=flags)
        stream, au, pts, dts = random_case(rng, 5000, prm, max_es=150)
        _, ap, s, _ = run(ctx, stream, au, pts, dts, prm)
        assert int(s["reserved"][1]) == 5000 and np.diff(ap).tolist()[1:] == [1] * 4999


def test_more_plan_blocks_than_one_scan_pass(ctx):
    """2049 plan workgroups and five AUs (the scan takes 2048 a pass), AUs of 0..8 ES bytes: 98.6 MB of output, against the
    vectorised restatement (which tests/test_tsmux_abi.py holds against the loop)"""
    rng = np.random.default_rng(54)
    n = 2049 * PLAN + 5
    prm = R.params(packet_bytes=188, cc_es=5)
    stream, au, _, _ = random_case(rng, n, prm, max_es=9)
    au["flags"] |= (rng.random(n) < 0.3).astype(np.uint32)
    want = R.mux_one_packet_aus(stream, au, prm)
    assert len(want[0]) < 150_000_000
    run(ctx, stream, au, None, None, prm, want=want)


def test_psi_placement(ctx):
    """HBS_TSMUX_PSI_AT_IRAP with IRAP on AUs 0, 1 and 2047..2049; the same AUs with HBS_TSMUX_NO_PSI, and with both flags"""
    rng = np.random.default_rng(55)
    n = 2100
    for B in R.SIZES:
        prm = R.params(packet_bytes=B, flags=R.PSI_AT_IRAP, cc_pat=14, cc_pmt=15)
        stream, au, pts, dts = random_case(rng, n, prm, max_es=500)
        au["flags"] &= ~np.uint32(R.AU_IRAP)
        au["flags"][[0, 1, 2047, 2048, 2049]] |= R.AU_IRAP
        _, ap, s, _ = run(ctx, stream, au, pts, dts, prm)
        assert int(s["reserved"][2]) == 5
        N = np.array([R.au_packets(int(e - b), R.time_fields(int(p), int(d)), False) for b, e, p, d in zip(au["unit_begin"], au["unit_end"], pts, dts)])
        pairs = (ap[:-1].astype(np.int64) - np.concatenate([[0], np.cumsum(N)[:-1]])) // 2           # in front of AU a, its own included
        assert np.flatnonzero(np.diff(np.concatenate([[0], pairs]))).tolist() == [0, 1, 2047, 2048, 2049]
        for flags in (R.NO_PSI, R.NO_PSI | R.PSI_AT_IRAP):
            _, ap, s, _ = run(ctx, stream, au, pts, dts, dict(prm, flags=flags))
            assert int(s["reserved"][2]) == 0 and int(ap[0]) == 0 and int(s["nal_count"]) == int(s["reserved"][1])


def test_continuity_across_two_calls(ctx):
    """non-zero starting counters; a second call seeded from reserved[1] continues the first"""
    rng = np.random.default_rng(56)
    for B in R.SIZES:
        prm = R.params(packet_bytes=B, cc_es=13, cc_pat=9, cc_pmt=6, flags=R.PCR)
        stream, au, pts, dts = random_case(rng, 300, prm, max_es=800)
        first, _, s1, _ = run(ctx, stream, au[:170], pts[:170], dts[:170], prm)
        assert int(s1["reserved"][1]) % 16 != 0
        prm2 = dict(prm, cc_es=(13 + int(s1["reserved"][1])) & 15, flags=R.PCR | R.NO_PSI)
        second, _, _, _ = run(ctx, stream, au[170:], pts[170:], dts[170:], prm2)
        both = np.concatenate([first.cpu().numpy(), second.cpu().numpy()])
        es, pes, ds = D.demux(both, B, prm["pid"])
        assert ds["error"] == 0 and ds["reserved"][1] == 0 and len(pes) == 300
        assert es.tobytes() == b"".join(stream[int(b):int(e)].tobytes() for b, e in zip(au["unit_begin"], au["unit_end"]))


@pytest.mark.parametrize("at", (0, 2047, 2048))
def test_malformed_entries_and_times(ctx, at):
    rng = np.random.default_rng(57 + at)
    n = 2300
    prm = R.params(packet_bytes=(188, 192, 204)[at % 3], flags=R.PCR)
    stream, au0, pts0, dts0 = random_case(rng, n, prm, max_es=300)
    pts0 = np.where(pts0 == R.NO_TIME, np.uint64(5), pts0).astype(np.uint64)
    _, _, clean = R.mux(stream, au0, pts0, dts0, prm)
    cases = {}
    for what in ("begin > end", "end > stream_bytes", "begin < the end in front", "pts 2^33", "dts 2^33", "dts without pts", "two, the lowest is named"):
        au, pts, dts = au0.copy(), pts0.copy(), dts0.copy()
        if what == "begin > end":
            au["unit_begin"][at] = au["unit_end"][at] + 1
        elif what == "end > stream_bytes":
            au["unit_end"][at] = len(stream) + 1
        elif what == "begin < the end in front":
            if at == 0:
                continue                                       # (AU 0 has nothing in front of it: 0 <= unit_begin always holds)
            au["unit_begin"][at] = au["unit_end"][at - 1] - 1
        elif what == "pts 2^33":
            pts[at] = 1 << 33
        elif what == "dts 2^33":
            dts[at] = 1 << 33
        elif what == "dts without pts":
            pts[at], dts[at] = R.NO_TIME, 7
        else:
            pts[at] = 1 << 40
            au["unit_end"][n - 1] = len(stream) + 9
        _, _, want = R.mux(stream, au, pts, dts, prm)
        assert want["error"] == R.E_ARG and want["reserved"][0] == at + 1, (what, want)
        untouched_on_error(ctx, put(stream, au, pts, dts, prm), want, clean["stream_bytes"], n, clean["stream_bytes"])
        cases[what] = True
    assert len(cases) >= 6


def test_capacity_one_byte_short(ctx):
    rng = np.random.default_rng(58)
    for B in R.SIZES:
        prm = R.params(packet_bytes=B)
        stream, au, pts, dts = random_case(rng, 2100, prm, max_es=300)
        _, _, want = R.mux(stream, au, pts, dts, prm)
        need = want["stream_bytes"]
        d = put(stream, au, pts, dts, prm)
        for cap in (need - 1, need - B, 0):
            untouched_on_error(ctx, d, dict(want, error=R.E_CAPACITY), need, 2100, cap)
    # the convenience call
    out, ap, s = ctx.ts_mux(d["stream"], au, pts, dts, packet_bytes=204)
    want_out, want_ap, _ = R.mux(stream, au, pts, dts, prm)
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(ap, want_ap) and int(s["error"]) == 0


def test_argument_refusals(ctx):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(59)
    prm = R.params()
    stream, au, pts, dts = random_case(rng, 40, prm)
    big = torch.zeros(len(stream) + 64, dtype=torch.uint8, device="cuda")
    d_au, d_pts, d_dts = (torch.cat([dev(x), torch.zeros(64, dtype=torch.uint8, device="cuda")]) for x in (au, pts, dts))
    out, ap = canary(400 * 188), canary(41 * 4 + 16)
    summary = torch.full((SUMMARY.itemsize + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(stream=big[16:16 + len(stream)], au=d_au, pts=d_pts, dts=d_dts, prm=R.params_record(prm), out=out, ap=ap, s=summary[:SUMMARY.itemsize])
    changes = [dict(stream=big[24:24 + len(stream)]), dict(stream=big[17:17 + len(stream)]), dict(au=d_au[8:]), dict(pts=d_pts[4:]), dict(dts=d_dts[4:]),
               dict(out=out[8:]), dict(ap=ap[2:]), dict(ap=ap[1:]), dict(s=summary[8:8 + SUMMARY.itemsize]), dict(prm=None)]
    changes += [dict(prm=R.params_record(R.params(**bad))) for bad in (dict(pid=15), dict(pid=8191), dict(pid=0x300, pmt_pid=0x300), dict(packet_bytes=190),
                                                                        dict(reserved=1), dict(flags=8), dict(cc_es=16), dict(program_number=0))]
    for change in changes:
        a = dict(good, **change)
        rc = ctx.ts_mux_async(a["stream"], len(stream), a["au"], 40, a["pts"], a["dts"], a["prm"], a["out"], a["ap"], a["s"], out_cap=400 * 188)
        assert rc == R.E_ARG, (change, rc)
    assert ctx.lib.hbs_ts_mux(ctx.h, good["stream"].data_ptr(), len(stream), d_au.data_ptr(), 40, None, None, good["prm"].ctypes.data, None, 0, None, None) == R.E_ARG
    assert ctx.ts_mux_async(good["stream"], len(stream), d_au, 1 << 32, d_pts, d_dts, good["prm"], None, None, good["s"]) == R.E_ARG
    torch.cuda.synchronize()
    assert (summary.cpu().numpy() == 0x5A).all() and (out.cpu().numpy() == CAN).all() and (ap.cpu().numpy() == CAN).all()
    assert ctx.ts_mux_async(good["stream"], len(stream), d_au, 40, d_pts, d_dts, good["prm"], out, ap, good["s"], out_cap=400 * 188) == 0
    assert int(ctx.read_summary(good["s"])["error"]) == 0


@pytest.mark.parametrize("B", R.SIZES)
def test_round_trip_on_the_device(ctx, B):
    """hbs_ts_demux of the mux's output: the AU bytes back to back, the PES table from the AU table"""
    rng = np.random.default_rng(60 + B)
    n = 2500
    prm = R.params(packet_bytes=B, flags=R.PCR | R.PSI_AT_IRAP, cc_es=3)
    stream, au, _, _ = random_case(rng, n, prm, max_es=700)
    E = (au["unit_end"] - au["unit_begin"]).astype(np.int64)
    want_es = b"".join(stream[int(b):int(e)].tobytes() for b, e in zip(au["unit_begin"], au["unit_end"]))
    irap = (au["flags"] & R.AU_IRAP) != 0
    dts = (np.arange(n, dtype=np.uint64) * np.uint64(3003) + np.uint64((1 << 33) - 2000 * 3003)) & np.uint64(R.MASK33)      # wraps on the way
    for pts, sent_dts, flags in (((dts + np.uint64(6006)) & np.uint64(R.MASK33), dts, D.F_PTS | D.F_DTS | D.F_ALIGN), (dts, None, D.F_PTS | D.F_ALIGN)):
        d = put(stream, au, pts, sent_dts, prm)
        out, ap, s = ctx.ts_mux(d["stream"], au, pts, sent_dts, **prm)
        es, pes, ds = ctx.ts_demux(out, prm["pid"], B)
        assert es.cpu().numpy().tobytes() == want_es
        assert int(ds["error"]) == 0 and int(ds["nal_count"]) == n and int(ds["reserved"][1]) == 0 and int(ds["reserved"][2]) == 0
        assert int(ds["nal_found"]) == int(s["reserved"][1])
        assert pes["out_off"].tolist() == np.concatenate([[0], np.cumsum(E)[:-1]]).tolist()
        assert np.array_equal(pes["packet"], ap[:-1])
        assert np.array_equal(pes["pts"], pts) and np.array_equal(pes["dts"], pts if sent_dts is None else sent_dts)
        assert np.array_equal(pes["flags"], np.where(irap, flags | D.F_RAI, flags))


def test_end_to_end_one_gop(ctx):
    """hevc_synth pictures -> index + parse -> access units -> hbs_ts_mux of one GOP, cut by pointer offset -> the PMT names the
    PID -> hbs_ts_demux -> hbs_index_extract: the index of the original NALs of that range"""
    import hevcbitstream_amd as hbs
    from tests.hevc_synth import Synth, annexb
    from tests.test_gpu_ts import parse_stream
    g = Synth(3, rich=False)
    rng = np.random.RandomState(4)
    units, n_nals = [], 0
    for pic in range(60):
        nals = []
        if pic % 20 == 0:
            nals += [g.vps(), g.sps_nal(1920, 1080, ctb_log2=6), g.pps_nal(force={"tiles": 0})]
        for sl in range(4):
            pay = rng.randint(0, 256, size=int(rng.randint(30, 900))).astype(np.uint8).tobytes()
            nals.append(g.slice_nal(19 if pic % 20 == 0 else 1, first=(sl == 0), payload=pay, address=sl * 120, tid=1))
        units.append(annexb(nals))
        n_nals += len(nals)
    stream = np.frombuffer(b"".join(units), dtype=np.uint8)
    d_stream = dev(stream)
    n, index, parsed, cc, structs = parse_stream(ctx, d_stream, n_nals)
    assert n == n_nals
    au, _, _, _ = ctx.access_units(index, parsed, cc, structs, n)
    assert len(au) == 60 and [k for k in range(60) if au["flags"][k] & hbs.AU_IRAP] == [0, 20, 40]
    ents = index[: n * 32].cpu().numpy().view(hbs.NAL_ENTRY)
    d_au = dev(au)
    first, count = 20, 20                                                     # the second GOP
    pts = ((np.arange(60, dtype=np.uint64) + 2) * 3003 + 90000).astype(np.uint64)
    dts = (np.arange(60, dtype=np.uint64) * 3003 + 90000).astype(np.uint64)
    d_pts, d_dts = dev(pts), dev(dts)
    for B in R.SIZES:
        prm = R.params(packet_bytes=B, flags=R.PCR, pid=0x1E1, pmt_pid=0x20, program_number=7, pcr_lead=9000)
        cut = slice(first * 64, (first + count) * 64)
        out, ap, s = ctx.ts_mux(d_stream, d_au[cut], d_pts[first * 8:(first + count) * 8], d_dts[first * 8:(first + count) * 8], **prm)
        want_out, want_ap, _ = R.mux(stream, au[first:first + count], pts[first:first + count], dts[first:first + count], prm)
        assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(ap, want_ap)
        assert hbs.ts_find_pid(out[: 2 * B].cpu().numpy(), B) == (0x1E1, 7)
        es, pes, ds = ctx.ts_demux(out, 0x1E1, B)
        lo, hi = int(au["unit_begin"][first]), int(au["unit_end"][first + count - 1])
        assert es.cpu().numpy().tobytes() == stream[lo:hi].tobytes()
        assert pes["pts"].tolist() == pts[first:first + count].tolist() and pes["dts"].tolist() == dts[first:first + count].tolist()
        assert bool(int(pes["flags"][0]) & D.F_RAI) and not any(int(f) & D.F_RAI for f in pes["flags"][1:])
        got, _, gs = ctx.index_extract(es, want_rbsp=False)
        k0, k1 = int(au["first_nal"][first]), int(au["first_nal"][first + count - 1] + au["nal_count"][first + count - 1])
        assert len(got) == k1 - k0
        assert np.array_equal(got["start"], ents["start"][k0:k1] - lo) and np.array_equal(got["end"], ents["end"][k0:k1] - lo)
        assert np.array_equal(got["rbsp_len"], ents["rbsp_len"][k0:k1])


def test_carved_buffers_at_each_accepted_alignment(ctx):
    """every pointer of the call inside a larger allocation, at each offset from a page boundary its alignment accepts; the bytes
    around every buffer are looked at afterwards, hostile sync bytes around the stream"""
    rng = np.random.default_rng(61)
    n = 300
    hostile = b"\x47\x41\x00\x10\x00\x00\x01\xE0" * 8
    for k in range(len(K.OFFS4)):
        B = R.SIZES[k % 3]
        prm = R.params(packet_bytes=B, flags=(R.PCR, R.PSI_AT_IRAP, 0)[k % 3], cc_es=k % 16)
        stream, au, pts, dts = random_case(rng, n, prm, max_es=600)
        want_out, want_ap, want_s = R.mux(stream, au, pts, dts, prm)
        need = want_s["stream_bytes"]
        o16 = lambda j: K.OFFS16[(k + j) % len(K.OFFS16)]          # noqa: E731
        o8 = lambda j: K.OFFS8[(k + j) % len(K.OFFS8)]             # noqa: E731
        cs = K.Carved(len(stream), o16(0), hostile, K.PAD, True).put(stream).hostile(front=hostile, back=hostile)
        ca = K.Carved(n * 64, o16(5), 0xFF, K.PAD, True).put(au)
        cp = K.Carved(n * 8, o8(0), 0xFF, K.PAD, True).put(pts)
        cd = K.Carved(n * 8, o8(4), 0xFF, K.PAD, True).put(dts)
        co = K.Carved(need, o16(3), CAN, K.PAD, True)
        ck = K.Carved((n + 1) * 4, K.OFFS4[k], CAN, K.PAD, True)
        cm = K.Carved(64, o16(6), 0xEE, K.PAD, True)
        tag = dict(stream=o16(0), au=o16(5), pts=o8(0), dts=o8(4), out=o16(3), au_packet=K.OFFS4[k], summary=o16(6), B=B)
        rc = ctx.ts_mux_async(cs.view, len(stream), ca.view, n, cp.view, cd.view, R.params_record(prm), co.view, ck.view, cm.view, out_cap=need)
        assert rc == 0, tag
        summary_matches(ctx.read_summary(cm.view), want_s)
        assert np.array_equal(co.get(), want_out), tag
        assert np.array_equal(ck.get().view(np.uint32), want_ap), tag
        for name, c in (("stream", cs), ("au", ca), ("pts", cp), ("dts", cd), ("out", co), ("au_packet", ck), ("summary", cm)):
            assert c.intact(), (tag, name, c.damage())
