"""hbs_mp4_fragment on the GPU against the plain loop of tests/_mp4_ref.py, byte for byte: plan first, then a run into outputs of
exactly the planned capacity with canaries behind d_out, both sample tables and d_frag, every summary field checked; then the
way back through the reader and hbs_lenpref_to_annexb."""
import numpy as np
import pytest

from tests import _mp4_ref as R
from tests import _carve as K
from tests._mp4_ref import random_case

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
W = 256                         # NALs, and AUs, of a plan workgroup (kMp4NalsPerBlock, kMp4AusPerBlock: hbs_mp4.h)
PASS = 256 * 8                  # plan workgroups scan_parts takes in one pass (kPlanLanes * kPlanPer: hbs_plan.h)
TILE = 64 * 1024                # output bytes of a copy workgroup
LDS_RECS = 1024                 # records of a tile the copy stages in LDS; a tile with more reads them from memory
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


def summary_matches(s, want):
    assert int(s["error"]) == want["error"], (s, want)
    assert int(s["stop_reason"]) == 0 and int(s["nal_found"]) == want["nal_found"]
    assert [int(x) for x in s["reserved"][:2]] == want["reserved"][:2], (s, want)
    if want["error"] != R.E_ARG:
        for k in ("nal_count", "rbsp_bytes", "stream_bytes"):
            assert int(s[k]) == want[k], (k, s, want)
        assert int(s["reserved"][2]) == want["reserved"][2], (s, want)


def put(case, prm, d_stream=None, nbytes=None):
    stream, index, keep, nal_au, au, dts, pts = case
    return dict(stream=dev(stream) if d_stream is None else d_stream, nbytes=len(stream) if nbytes is None else nbytes, index=dev(index),
                n=len(index), keep=dev(keep), nal_au=dev(nal_au), au=dev(au), n_aus=len(au), dts=dev(dts), pts=dev(pts), prm=R.params_record(prm))


def call(ctx, d, out, so, ss, fr, out_cap=None, frag_cap=None, fill=0x5A):
    """d: the device inputs of a case (put)"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), fill, dtype=torch.uint8, device="cuda")
    rc = ctx.mp4_fragment_async(d["stream"], d["nbytes"], d["index"], d["n"], d["nal_au"], d["au"], d["n_aus"], d["prm"], out, summary,
                                keep=d["keep"], dts=d["dts"], pts=d["pts"], sample_off=so, sample_size=ss, frag=fr, frag_cap=frag_cap, out_cap=out_cap)
    assert rc == 0, rc
    return ctx.read_summary(summary)


def check_outputs(out, so, ss, fr, want):
    want_out, want_off, want_size, want_frags, want_s = want
    need, n_aus, R_ = want_s["stream_bytes"], len(want_off), want_s["nal_count"]
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
        assert np.array_equal(p[: n_aus * 8].view(np.uint64), w), name
        assert (p[n_aus * 8:] == CAN).all(), "stored behind " + name
    p = fr.cpu().numpy()
    assert np.array_equal(p[: R_ * FRAG].view(R.FRAG), want_frags), "d_frag"
    assert (p[R_ * FRAG:] == CAN).all(), "stored behind d_frag"


def run(ctx, case, prm, d_stream=None, nbytes=None, want=None):
    """plan, then a run into outputs of exactly the planned capacity; everything against the plain loop.
    -> (out, the reference's results, summary, device inputs)"""
    want = want if want is not None else R.fragment(*case, prm)
    want_s = want[4]
    assert want_s["error"] == 0, want_s
    d = put(case, prm, d_stream, nbytes)
    s = call(ctx, d, None, None, None, None)
    summary_matches(s, want_s)
    need, n_aus, frags = int(s["stream_bytes"]), d["n_aus"], int(s["nal_count"])
    out, so, ss, fr = canary(need), canary(n_aus * 8), canary(n_aus * 8), canary(frags * FRAG)
    s2 = call(ctx, d, out, so, ss, fr, out_cap=need, frag_cap=frags)
    summary_matches(s2, want_s)
    assert s2.tobytes() == s.tobytes(), "the plan's summary is the run's"
    check_outputs(out, so, ss, fr, want)
    return out[:need], want, s2, d


MODES = (dict(), dict(flags=R.CUT_AT_IRAP), dict(max_samples=1), dict(max_samples=3, flags=R.CUT_AT_IRAP))


@pytest.mark.parametrize("L", (1, 2, 4))
@pytest.mark.parametrize("mode", range(4))
def test_random_mixes(ctx, L, mode):
    """with and without d_keep, AUs with nothing kept, kept NALs of length 0, times present and absent, negative cts"""
    rng = np.random.default_rng(10 * L + mode)
    for k, n_aus in enumerate((1, 2, 37, W - 1, W, W + 1, 3 * W + 7)):
        every = (1, 2, 3, 4, 7)[k % 5] if mode == 3 else None
        case = random_case(rng, n_aus, max_nal=255 if L == 1 else (700, 5000)[k % 2], keep_some=k % 2 == 0, times=k % 3 != 1, irap_every=every)
        assert mode != 1 or not case[4]["flags"][0] & 1
        prm = R.params(length_size=L, track_id=int(rng.integers(1, 1 << 32)), sequence=(1 << 32) - 2 if k == 2 else int(rng.integers(0, 1 << 32)),
                       sample_duration=int(rng.integers(0, 1 << 32)), base_time=int(rng.integers(0, 1 << 60)), **MODES[mode])
        _, want, s, _ = run(ctx, case, prm)
        if mode == 0:
            assert int(s["nal_count"]) == 1
        if mode == 2:
            assert int(s["nal_count"]) == n_aus


def test_every_source_alignment(ctx):
    rng = np.random.default_rng(50)
    for lead in range(16):
        case = random_case(rng, 20, max_nal=3000, keep_some=False, lead=lead, irap_every=5)
        assert int(case[1]["start"][0]) % 16 == lead
        run(ctx, case, R.params(length_size=(4, 2, 4)[lead % 3], flags=R.CUT_AT_IRAP))


def test_gaps_junk_and_the_end_of_the_allocation(ctx):
    """gaps of 0, 1, 15, 16, 17 and 100 000 bytes of junk between the NALs; the last NAL ends at stream_bytes, and the stream is a
    12 MiB allocation of its own, so that its last byte is the allocation's last (tests/_carve.py keeps every buffer away from
    its allocation's ends, so it cannot make this one)"""
    import torch
    rng = np.random.default_rng(51)
    total = 12 << 20
    gaps = [0, 1, 15, 16, 17, 100000] * 20
    sizes = rng.integers(0, 3000, size=len(gaps))
    starts = np.cumsum(np.array(gaps) + np.concatenate([[0], sizes[:-1]]))
    ends = starts + sizes
    shift = total - int(ends[-1])
    assert shift >= 0
    starts, ends = starts + shift, ends + shift
    stream = rng.integers(0, 256, size=total, dtype=np.uint8)
    torch.cuda.empty_cache()                                    # (no cached block to cut the 12 MiB from)
    d_stream = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_stream.copy_(torch.from_numpy(stream))
    n = len(gaps)
    for L, last in ((4, 0), (2, 1), (4, 17), (2, 5)):
        ends[-1] = total
        starts[-1] = total - 3000 - last
        nal_au = (np.arange(n) // 4).astype(np.uint32)
        n_aus = int(nal_au[-1]) + 1
        au = R.au_records((np.arange(n_aus) % 6 == 0).astype(np.uint32))
        run(ctx, (stream, R.entries(starts, ends), None, nal_au, au, None, None), R.params(length_size=L, flags=R.CUT_AT_IRAP, max_samples=4), d_stream=d_stream)


def test_tiles_inside_a_payload_and_inside_a_trun_array(ctx):
    """one NAL of 200 KiB: tiles that lie wholly inside a payload; one fragment of 4 200 samples of 3-byte NALs: 67 200 bytes of
    trun entries, a tile wholly inside them, and more records a tile (64 KiB / 7) than the copy stages in LDS"""
    rng = np.random.default_rng(52)
    big = 200 * 1024
    sizes = np.array([40, big, 7, 300])
    starts = np.cumsum(np.array([3, 5, 4, 3]) + np.concatenate([[0], sizes[:-1]]))
    stream = rng.integers(0, 256, size=int(starts[-1] + sizes[-1]), dtype=np.uint8)
    run(ctx, (stream, R.entries(starts, starts + sizes), None, np.array([0, 0, 1, 2], np.uint32), R.au_records([1, 0, 0]), None, None), R.params())
    n = 4200
    starts = 5 * np.arange(n) + 3
    stream = rng.integers(0, 256, size=5 * n + 8, dtype=np.uint8)
    case = (stream, R.entries(starts, starts + 3), None, np.arange(n, dtype=np.uint32) + 9, R.au_records(np.zeros(n, np.uint32)), None, None)
    assert 16 * n > TILE + 96 and TILE // 7 > LDS_RECS
    _, want, s, _ = run(ctx, case, R.params(length_size=4, sample_duration=1))
    assert int(s["nal_count"]) == 1


def test_tiles_of_slow_chunks_only_and_a_partial_last_chunk(ctx):
    """18 801 AUs of one 3-byte NAL, L = 4, one fragment: a 7-byte record never holds 16 payload bytes, so every chunk of every
    tile is on the copy's slow list -- the tiles of the trun array, the tile the payload begins in, a whole tile of payload
    alone -- and the last tile ends in a chunk of 7 bytes"""
    rng = np.random.default_rng(55)
    n = 18801
    starts = 3 * np.arange(n)
    stream = rng.integers(0, 256, size=3 * n, dtype=np.uint8)
    case = (stream, R.entries(starts, starts + 3), None, np.arange(n, dtype=np.uint32), R.au_records(np.zeros(n, np.uint32)), None, None)
    out, want, s, _ = run(ctx, case, R.params(length_size=4, sample_duration=3003))
    payload = int(want[1][0])                                   # where the first sample begins
    assert int(s["nal_count"]) == 1 and len(out) == payload + 7 * n and len(out) % 16 == 7
    assert (payload + TILE - 1) // TILE < len(out) // TILE, "a whole tile of payload alone"


def test_more_plan_blocks_than_one_scan_pass(ctx):
    """PASS plan workgroups and five entries more on both sides: PASS * W + 5 = 524 293 NALs, one an AU, so as many AUs; NALs of
    0..3 bytes, L = 1, an IRAP every 64th AU with HBS_MP4_CUT_AT_IRAP: 8 193 fragments, 11 MB of output"""
    rng = np.random.default_rng(54)
    n = PASS * W + 5
    lens = rng.integers(0, 4, size=n)
    starts = np.cumsum(3 + np.concatenate([[0], lens[:-1]]))
    stream = rng.integers(0, 256, size=int(starts[-1] + lens[-1]), dtype=np.uint8)
    keep = (rng.integers(0, 8, size=n) != 0).astype(np.uint8)
    au = R.au_records((np.arange(n) % 64 == 0).astype(np.uint32))
    case = (stream, R.entries(starts, starts + lens), keep, np.arange(n, dtype=np.uint32), au, None, None)
    want = R.fragment(*case, R.params(length_size=1, flags=R.CUT_AT_IRAP, sample_duration=1001, base_time=5))
    assert want[4]["nal_count"] == (n + 63) // 64 and want[4]["stream_bytes"] < 12_000_000
    run(ctx, case, R.params(length_size=1, flags=R.CUT_AT_IRAP, sample_duration=1001, base_time=5), want=want)


def test_round_trip_through_the_reader(ctx):
    """the READER's sample table of the call's output -> hbs_lenpref_to_annexb -> hbs_index_extract: the kept NALs' payloads in
    order; the call's own tables equal the reader's"""
    rng = np.random.default_rng(55)
    n_aus = 90
    counts = rng.integers(1, 5, size=n_aus)
    n = int(counts.sum())
    lens = rng.integers(2, 900, size=n)
    starts = np.cumsum(4 + np.concatenate([[0], lens[:-1]]))
    stream = rng.integers(4, 256, size=int(starts[-1] + lens[-1]), dtype=np.uint8)          # no zero byte: a walk finds the payloads alone
    keep = (rng.integers(0, 4, size=n) != 0).astype(np.uint8)
    nal_au = np.repeat(np.arange(n_aus, dtype=np.uint32), counts)
    for a in (3, 50):
        keep[nal_au == a] = 0
    case = (stream, R.entries(starts, starts + lens), keep, nal_au, R.au_records((np.arange(n_aus) % 9 == 0).astype(np.uint32)), None, None)
    prm = R.params(length_size=2, flags=R.CUT_AT_IRAP, max_samples=4)
    out, want, s, _ = run(ctx, case, prm)
    got = R.read_fragments(out.cpu().numpy())
    table = [x for f in got for x in f["samples"]]
    off, size = np.array([x[0] for x in table], np.uint64), np.array([x[1] for x in table], np.uint64)
    assert np.array_equal(off, want[1]) and np.array_equal(size, want[2])
    back, _, bs = ctx.lenpref_to_annexb(out, off, size, length_size=2, startcode_bytes=4)
    idx, _, _ = ctx.index_extract(back, index_cap=n + 16, want_rbsp=False)
    b = back.cpu().numpy()
    kept = np.flatnonzero(keep)
    assert len(idx) == len(kept) == int(s["reserved"][2])
    for e, k in zip(idx, kept):
        assert b[int(e["start"]):int(e["end"])].tobytes() == stream[starts[k]:starts[k] + lens[k]].tobytes()


def untouched_on_error(ctx, d, want_s, cap_bytes, out_cap, frag_cap):
    """the plan and a run both report want_s; the canary-filled outputs are untouched"""
    summary_matches(call(ctx, d, None, None, None, None), dict(want_s, error=want_s["error"] if want_s["error"] == R.E_ARG else 0))
    out, so, ss, fr = canary(cap_bytes), canary(d["n_aus"] * 8), canary(d["n_aus"] * 8), canary(max(frag_cap, 1) * FRAG)
    summary_matches(call(ctx, d, out, so, ss, fr, out_cap=out_cap, frag_cap=frag_cap), want_s)
    for t in (out, so, ss, fr):
        assert (t.cpu().numpy() == CAN).all(), "written in spite of the error"


def error_case(rng):
    case = random_case(rng, 260, max_nal=250, max_nals_per_au=5, keep_some=False)
    assert len(case[1]) > 2 * W + 10
    return case


@pytest.mark.parametrize("at", ("0", "255", "256", "last"))
def test_nal_errors(ctx, at):
    rng = np.random.default_rng(60)
    stream, index, keep, nal_au, au, dts, pts = error_case(rng)
    n = len(index)
    k = n - 1 if at == "last" else int(at)
    prm = R.params(length_size=1)
    spoils = ["start_gt_end", "end_gt_stream", "overlap", "too_long"] + (["au_step_2", "au_step_back"] if k else []) + (["last_au"] if k == n - 1 else [])
    for what in spoils:
        i2, a2, s2 = index.copy(), nal_au.copy(), stream
        if what == "start_gt_end":
            i2["start"][k] = i2["end"][k] + 1
        elif what == "end_gt_stream":
            i2["end"][k] = len(stream) + 1
            i2["start"][k + 1:] = len(stream) + 1
            i2["end"][k + 1:] = len(stream) + 1
        elif what == "overlap":
            if k == 0:
                continue
            i2["end"][k - 1] += 1
            i2["start"][k] = i2["end"][k - 1] - 1
        elif what == "too_long":
            grow = 256 - int(i2["end"][k] - i2["start"][k])
            i2["end"][k] += grow
            i2["start"][k + 1:] += grow
            i2["end"][k + 1:] += grow
            s2 = np.concatenate([stream, rng.integers(0, 256, size=grow, dtype=np.uint8)])
        elif what == "au_step_2":
            a2[k:] += 2 if a2[k] == a2[k - 1] else 1
        elif what == "au_step_back":
            a2[k:] -= 2 if a2[k] != a2[k - 1] else 1
        elif what == "last_au":
            au = au[:-1] if len(au) > 1 else au
        case = (s2, i2, keep, a2, au, dts, pts)
        want = R.fragment(*case, prm)[4]
        assert want["error"] == R.E_ARG and want["reserved"][0] >= 1, (what, want)
        if what in ("start_gt_end", "too_long", "au_step_2", "au_step_back", "last_au"):
            assert want["reserved"][0] == k + 1, (what, want)
        untouched_on_error(ctx, put(case, prm), want, 1 << 20, 1 << 20, len(au))


@pytest.mark.parametrize("at", ("0", "last"))
def test_time_errors_and_both_kinds(ctx, at):
    rng = np.random.default_rng(61)
    stream, index, keep, nal_au, au, dts, pts = error_case(rng)
    n_aus = len(au)
    a = n_aus - 1 if at == "last" else 0
    prm = R.params(length_size=2, sample_duration=40)
    for what in ("dts_limit", "dts_absent", "dts_back", "dur_big", "pts_limit", "cts_big", "cts_low", "ruled", "both"):
        d2, p2, i2, prm2 = dts.copy(), pts.copy(), index, prm
        if what == "dts_limit":
            d2[a:] += np.uint64(1 << 62) - d2[a]
            p2[a:] = d2[a:]
        elif what == "dts_absent":
            d2[a] = (1 << 64) - 1
        elif what == "dts_back":
            b = max(a, 1)
            d2[b] = d2[b - 1] - np.uint64(1)
            p2[b] = d2[b]
        elif what == "dur_big":
            b = max(a, 1)
            d2[b:] += np.uint64(1 << 32)
            p2[b:] += np.uint64(1 << 32)
        elif what == "pts_limit":
            p2[a] = 1 << 62
        elif what == "cts_big":
            p2[a] = d2[a] + np.uint64(1 << 31)
        elif what == "cts_low":
            d2 += np.uint64(1 << 33)
            p2 += np.uint64(1 << 33)
            p2[a] = d2[a] - np.uint64((1 << 31) + 1)
        elif what == "ruled":
            d2 = p2 = None
            prm2 = dict(prm, base_time=(1 << 62) - 40 * max(a, 1))              # dts(max(a, 1)) is 2^62
        elif what == "both":
            p2[a] = 1 << 62
            i2 = index.copy()
            i2["start"][7] = i2["end"][7] + 1
        case = (stream, i2, keep, nal_au, au, d2, p2)
        want = R.fragment(*case, prm2)[4]
        assert want["error"] == R.E_ARG and want["reserved"][1] >= 1, (what, want)
        if what in ("pts_limit", "cts_big", "cts_low", "both"):
            assert want["reserved"][1] == a + 1, (what, want)
        assert (want["reserved"][0] == 8) == (what == "both")
        untouched_on_error(ctx, put(case, prm2), want, 1 << 20, 1 << 20, n_aus)
    # the exact edges are accepted: the last dts 2^62 - 1 behind a duration of 2^32 - 1, a duration of 0, both ends of cts
    top = (1 << 62) - 1
    d2 = np.array([top - ((1 << 32) - 1) - (n_aus - 2 - i) * 40 for i in range(n_aus - 1)] + [top], dtype=np.uint64)
    d2[n_aus - 3] = d2[n_aus - 2]
    p2 = d2.copy()
    p2[0], p2[1] = d2[0] - np.uint64(1 << 31), d2[1] + np.uint64((1 << 31) - 1)
    run(ctx, (stream, index, keep, nal_au, au, d2, p2), prm)
    run(ctx, (stream, index, keep, nal_au, au, None, None), dict(prm, base_time=(1 << 62) - 1 - 40 * (n_aus - 1)))


def test_capacity_plan_only_and_empty(ctx):
    rng = np.random.default_rng(62)
    case = random_case(rng, 70, irap_every=9)
    prm = R.params(length_size=4, flags=R.CUT_AT_IRAP)
    want = R.fragment(*case, prm)
    need, frags = want[4]["stream_bytes"], want[4]["nal_count"]
    assert frags == 8
    d = put(case, prm)
    short = R.fragment(*case, prm, out_cap=need - 1)[4]
    assert short["error"] == R.E_CAPACITY and short["stream_bytes"] == need
    untouched_on_error(ctx, d, short, need, need - 1, frags)
    untouched_on_error(ctx, d, R.fragment(*case, prm, frag_cap=frags - 1)[4], need, need, frags - 1)
    # without a d_frag, frag_cap means nothing; without the sample tables they are not written
    out = canary(need)
    summary_matches(call(ctx, d, out, None, None, None, out_cap=need, frag_cap=0), want[4])
    assert np.array_equal(out.cpu().numpy()[:need], want[0]) and (out.cpu().numpy()[need:] == CAN).all()
    # no NAL, no AU: an empty output with no fragment
    empty = (np.zeros(0, np.uint8), R.entries([], []), None, np.zeros(0, np.uint32), R.au_records([]), None, None)
    d0 = put(empty, prm)
    for o in (None, canary(64)):
        s = call(ctx, d0, o, None, None, None, out_cap=64 if o is not None else 0)
        summary_matches(s, R.summary())
        assert o is None or (o.cpu().numpy() == CAN).all()


def test_argument_refusals(ctx):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(63)
    case = random_case(rng, 20)
    d = put(case, R.params())
    need = R.fragment(*case, R.params())[4]["stream_bytes"]
    out, so, ss, fr = canary(need), canary(20 * 8), canary(20 * 8), canary(4 * FRAG)
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")

    def rc(prm=None, **kw):
        a = dict(d, out=out, so=so, ss=ss, fr=fr, summary=summary, out_cap=need, frag_cap=4, prm=R.params_record(R.params(**(prm or {}))))
        a.update(kw)
        return ctx.mp4_fragment_async(a["stream"], a["nbytes"], a["index"], a["n"], a["nal_au"], a["au"], a["n_aus"], a["prm"], a["out"], a["summary"],
                                      keep=a["keep"], dts=a["dts"], pts=a["pts"], sample_off=a["so"], sample_size=a["ss"], frag=a["fr"],
                                      frag_cap=a["frag_cap"], out_cap=a["out_cap"])
    for prm in (dict(length_size=0), dict(length_size=3), dict(length_size=8), dict(flags=2), dict(flags=1 << 31), dict(track_id=0),
                dict(base_time=1 << 62), dict(base_time=(1 << 64) - 1)):
        assert rc(prm) == R.E_ARG, prm
    for kw in (dict(prm=None), dict(n=1 << 32), dict(n_aus=1 << 32), dict(n=0), dict(out_cap=(1 << 46) + 1), dict(so=None), dict(ss=None),
               dict(summary=None), dict(index=None), dict(nal_au=None), dict(au=None), dict(stream=None),
               dict(stream=d["stream"][8:]), dict(out=out[8:]), dict(au=d["au"][8:]), dict(fr=fr[8:]), dict(summary=canary(64)[8:]),
               dict(index=d["index"][4:]), dict(dts=d["dts"][4:]), dict(pts=d["pts"][4:]), dict(so=so[4:]), dict(ss=ss[4:]), dict(nal_au=d["nal_au"][2:])):
        if "prm" in kw:
            a = dict(d, prm=None)
            got = ctx.mp4_fragment_async(a["stream"], a["nbytes"], a["index"], a["n"], a["nal_au"], a["au"], a["n_aus"], None, out, summary)
        else:
            got = rc(**kw)
        assert got == R.E_ARG, list(kw)
    torch.cuda.synchronize()
    for t in (out, so, ss, fr):
        assert (t.cpu().numpy() == CAN).all()
    assert (summary.cpu().numpy() == 0x5A).all()
    assert rc() == 0 and rc(dict(base_time=(1 << 62) - 1, track_id=(1 << 32) - 1), dts=None, pts=None) == 0 and rc(out_cap=1 << 46) == 0


def test_sources_above_4gib_and_the_mdat_limit(ctx):
    """one allocation of 2^32 + 64 MiB, filled once on the device.  (a) AUs in the first MiB and around offset 2^32: the gaps are
    not copied, so the output is small and is compared byte for byte (the reference works on the two regions put next to each
    other).  (b) plan only, a fabricated index of one NAL: 2^32 - 13 bytes make a record of 2^32 - 9, the largest an mdat of 32
    bits holds, and are accepted; one byte more is HBS_E_ARG at AU 0.  Output offsets above 2^32 stay untested."""
    import torch
    rng = np.random.default_rng(64)
    total = (1 << 32) + (64 << 20)
    torch.cuda.empty_cache()
    d_stream = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_stream.random_(0, 256)
    half = 512 << 10
    lo, hi = (1 << 32) - half, (1 << 32) + half
    compact = np.concatenate([d_stream[: 2 * half].cpu().numpy(), d_stream[lo:hi].cpu().numpy()])
    n_aus = 60
    counts = rng.integers(1, 5, size=n_aus)
    n = int(counts.sum())
    lens = rng.integers(0, 8000, size=n)
    lens[n // 2] = 40000                                       # this one straddles 2^32
    starts = np.cumsum(rng.integers(3, 40, size=n) + np.concatenate([[0], lens[:-1]]))
    first_b = n // 2
    assert starts[first_b - 1] + lens[first_b - 1] <= 2 * half
    to_b = 2 * half + half - 20000 - int(starts[first_b])
    cstarts = starts.copy()
    cstarts[first_b:] += to_b
    assert cstarts[-1] + lens[-1] <= len(compact) and cstarts[first_b] < 3 * half < cstarts[first_b] + lens[first_b]
    real = cstarts.copy()
    real[first_b:] += lo - 2 * half
    assert real[first_b] < (1 << 32) < real[first_b] + lens[first_b] and real[-1] > (1 << 32)
    nal_au = np.repeat(np.arange(n_aus, dtype=np.uint32), counts)
    au = R.au_records((np.arange(n_aus) % 7 == 0).astype(np.uint32))
    prm = R.params(length_size=4, flags=R.CUT_AT_IRAP, max_samples=5)
    seed = 99
    want = R.fragment(compact, R.entries(cstarts, cstarts + lens, seed), None, nal_au, au, None, None, prm, stream_bytes=total)
    run(ctx, (compact, R.entries(real, real + lens, seed), None, nal_au, au, None, None), prm, d_stream=d_stream, nbytes=total, want=want)
    # (b)
    one_au = R.au_records([1])
    for size, ok in (((1 << 32) - 13, True), ((1 << 32) - 12, False)):
        d = put((compact, R.entries([16], [16 + size]), None, np.zeros(1, np.uint32), one_au, None, None), prm, d_stream=d_stream, nbytes=total)
        s = call(ctx, d, None, None, None, None)
        if ok:
            summary_matches(s, R.summary(0, 1, 1, size + 4, size + 4 + 112, kept=1))
        else:
            summary_matches(s, R.summary(R.E_ARG, n_nals=1, bad_au=1))
    del d_stream
    torch.cuda.empty_cache()


def test_two_calls_chained_equal_one(ctx):
    """sequence and base_time continued, the second call's tables passed by pointer offset: the same bytes as one call that cuts
    at the same AU"""
    import torch
    rng = np.random.default_rng(65)
    n_aus, split = 100, 40
    stream, index, keep, nal_au, au, _, _ = random_case(rng, n_aus, irap_every=20, max_nal=2000)
    prm = R.params(length_size=4, flags=R.CUT_AT_IRAP, max_samples=7, sequence=(1 << 32) - 2, sample_duration=3003, base_time=1 << 40)
    out, want, s, d = run(ctx, (stream, index, keep, nal_au, au, None, None), prm)
    k = int(np.searchsorted((nal_au - nal_au[0]).astype(np.int64), split))
    r1 = int(np.searchsorted(want[3]["first_au"], split))
    assert want[3]["first_au"][r1] == split
    cut = int(want[3]["out_off"][r1])
    parts = []
    for sl_n, sl_a, seq, base in ((slice(0, k), slice(0, split), prm["sequence"], prm["base_time"]),
                                  (slice(k, None), slice(split, None), (prm["sequence"] + r1) & R.M32, prm["base_time"] + split * 3003)):
        d2 = dict(d, index=d["index"][sl_n.start * 32:], n=len(index[sl_n]), keep=d["keep"][sl_n.start:], nal_au=d["nal_au"][sl_n.start * 4:],
                  au=d["au"][sl_a.start * 64:], n_aus=len(au[sl_a]), prm=R.params_record(dict(prm, sequence=seq, base_time=base)))
        sp = call(ctx, d2, None, None, None, None)
        need = int(sp["stream_bytes"])
        o, so = canary(need), canary(d2["n_aus"] * 8)
        ss = canary(d2["n_aus"] * 8)
        s3 = call(ctx, d2, o, so, ss, None, out_cap=need)
        assert int(s3["error"]) == 0
        parts.append((o[:need].cpu().numpy(), so.cpu().numpy()[: d2["n_aus"] * 8].view(np.uint64), int(s3["nal_count"])))
    assert len(parts[0][0]) == cut and parts[0][2] == r1 and parts[0][2] + parts[1][2] == int(s["nal_count"])
    assert np.array_equal(np.concatenate([parts[0][0], parts[1][0]]), want[0])
    assert np.array_equal(np.concatenate([parts[0][1], parts[1][1] + np.uint64(cut)]), want[1])
    torch.cuda.synchronize()


def test_carved_buffers_at_each_accepted_alignment(ctx):
    """every pointer of the call inside a larger allocation, at each offset from a page boundary its alignment accepts; the bytes
    around every buffer are looked at afterwards"""
    rng = np.random.default_rng(66)
    for k in range(len(K.OFFS4)):
        prm = R.params(length_size=(1, 2, 4)[k % 3], flags=k % 2, max_samples=(0, 2, 5)[k % 3])
        case = random_case(rng, 80, max_nal=255 if k % 3 == 0 else 2500)
        stream, index, keep, nal_au, au, dts, pts = case
        want = R.fragment(*case, prm)
        need, frags, n, n_aus = want[4]["stream_bytes"], want[4]["nal_count"], len(index), len(au)
        o16 = lambda j: K.OFFS16[(k + j) % len(K.OFFS16)]          # noqa: E731
        o8 = lambda j: K.OFFS8[(k + j) % len(K.OFFS8)]             # noqa: E731
        cs = K.Carved(len(stream), o16(0), 0x3C, K.PAD, True).put(stream)
        ci = K.Carved(n * 32, o8(5), 0xFF, K.PAD, True).put(index)
        ck = K.Carved(n, K.OFFS1[k % len(K.OFFS1)], 0xFF, K.PAD, True).put(keep)
        ca = K.Carved(n * 4, K.OFFS4[k], 0xFF, K.PAD, True).put(nal_au)
        cu = K.Carved(n_aus * 64, o16(2), 0xFF, K.PAD, True).put(au)
        cd = K.Carved(n_aus * 8, o8(0), 0xFF, K.PAD, True).put(dts)
        cp = K.Carved(n_aus * 8, o8(3), 0xFF, K.PAD, True).put(pts)
        co = K.Carved(need, o16(3), CAN, K.PAD, True)
        cso = K.Carved(n_aus * 8, o8(2), CAN, K.PAD, True)
        css = K.Carved(n_aus * 8, o8(7), CAN, K.PAD, True)
        cf = K.Carved(frags * FRAG, o16(5), CAN, K.PAD, True)
        cm = K.Carved(64, o16(6), 0xEE, K.PAD, True)
        rc = ctx.mp4_fragment_async(cs.view, len(stream), ci.view, n, ca.view, cu.view, n_aus, R.params_record(prm), co.view, cm.view, keep=ck.view,
                                    dts=cd.view, pts=cp.view, sample_off=cso.view, sample_size=css.view, frag=cf.view, frag_cap=frags, out_cap=need)
        assert rc == 0, k
        summary_matches(ctx.read_summary(cm.view), want[4])
        assert np.array_equal(co.get(), want[0]), k
        assert np.array_equal(cso.get().view(np.uint64), want[1]) and np.array_equal(css.get().view(np.uint64), want[2]), k
        assert np.array_equal(cf.get().view(R.FRAG), want[3]), k
        for name, c in (("stream", cs), ("index", ci), ("keep", ck), ("nal_au", ca), ("au", cu), ("dts", cd), ("pts", cp), ("out", co),
                        ("sample_off", cso), ("sample_size", css), ("frag", cf), ("summary", cm)):
            assert c.intact(), (k, name, c.damage())


def test_one_replay_from_a_graph_on_other_contents(ctx):
    """captured on a side stream after one warm-up call, replayed on other contents of the same buffers: other bytes, the NAL
    sizes in another order, other AU numbers, flags and times; every host argument is the same"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(67)
    n = 3 * W + 11
    n_aus = W + 30
    sizes = rng.integers(0, 2600, size=n)
    prm = R.params(length_size=4, flags=R.CUT_AT_IRAP, max_samples=6, sequence=77)
    members = []
    for order in (sizes, sizes[::-1].copy()):
        starts = np.concatenate([[0], np.cumsum(order[:-1])])
        stream = rng.integers(0, 256, size=int(order.sum()), dtype=np.uint8)
        steps = np.zeros(n, np.int64)
        steps[rng.choice(np.arange(1, n), size=n_aus - 1, replace=False)] = 1
        nal_au = (np.cumsum(steps) + int(rng.integers(0, 99))).astype(np.uint32)
        au = R.au_records((rng.integers(0, 10, size=n_aus) == 0).astype(np.uint32), seed=len(members))
        dts = (np.cumsum(rng.integers(0, 5000, size=n_aus)) + (1 << 35)).astype(np.uint64)
        pts = dts + rng.integers(0, 9000, size=n_aus).astype(np.uint64)
        case = (stream, R.entries(starts, starts + order, seed=len(members)), None, nal_au, au, dts, pts)
        members.append((case, R.fragment(*case, prm)))
    need = max(m[1][4]["stream_bytes"] for m in members)
    frags = max(m[1][4]["nal_count"] for m in members)
    assert not np.array_equal(members[0][1][0][:1000], members[1][1][0][:1000])
    d = put(members[0][0], prm)
    out, so, ss, fr = canary(need), canary(n_aus * 8), canary(n_aus * 8), canary(frags * FRAG)
    summary = torch.full((SUMMARY.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")

    def launch():
        return ctx.mp4_fragment_async(d["stream"], d["nbytes"], d["index"], n, d["nal_au"], d["au"], n_aus, d["prm"], out, summary, dts=d["dts"],
                                      pts=d["pts"], sample_off=so, sample_size=ss, frag=fr, frag_cap=frags, out_cap=need)

    def check(want):
        s = ctx.read_summary(summary)
        summary_matches(s, want[4])
        w, f = want[4]["stream_bytes"], want[4]["nal_count"]
        o = out.cpu().numpy()
        assert np.array_equal(o[:w], want[0]) and (o[w:] == CAN).all()
        assert np.array_equal(so.cpu().numpy()[: n_aus * 8].view(np.uint64), want[1]) and np.array_equal(ss.cpu().numpy()[: n_aus * 8].view(np.uint64), want[2])
        p = fr.cpu().numpy()
        assert np.array_equal(p[: f * FRAG].view(R.FRAG), want[3]) and (p[f * FRAG:] == CAN).all()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert launch() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    check(members[0][1])
    held = ctx.device_bytes()
    for which in (1, 0):
        case, want = members[which]
        for name, a in (("stream", case[0]), ("index", case[1]), ("nal_au", case[3]), ("au", case[4]), ("dts", case[5]), ("pts", case[6])):
            d[name].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        for t in (out, so, ss, fr):
            t.fill_(CAN)
        summary.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        check(want)
    assert ctx.device_bytes() == held
