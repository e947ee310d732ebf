"""hbs_mp4_stbl_samples on the GPU against the reader of tests/_mp4_stbl_ref.py, entry for entry: plan first, then a run into
tables of exactly N entries with canaries behind every one of them, every summary field checked; the round trip from an
Annex-B stream through a progressive file and back."""
import numpy as np
import pytest

from tests import _mp4_stbl_ref as S
from tests.test_mp4_read_ref import NALS

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 1024
W = 256                         # table entries and samples of a workgroup (kStLanes: hbs_mp4stbl.h)
PASS = 256 * 8                  # workgroups scan_parts / seg_scan_parts take in one pass (kPlanLanes * kPlanPer: hbs_plan.h)
M = S.M32
TABLES = (("sample_off", 8), ("sample_size", 8), ("dts", 8), ("pts", 8), ("sample_flags", 4))


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


def call(ctx, d_buf, nbytes, rec, sample_cap=0, outs=None, fill=0x5A):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), fill, dtype=torch.uint8, device="cuda")
    rc = ctx.mp4_stbl_samples_async(d_buf, nbytes, rec, summary, sample_cap=sample_cap, **(outs or {}))
    assert rc == 0, rc
    return ctx.read_summary(summary)


def summary_matches(s, want):
    got = dict(error=int(s["error"]), nal_count=int(s["nal_count"]), nal_found=int(s["nal_found"]), rbsp_bytes=int(s["rbsp_bytes"]),
               stream_bytes=int(s["stream_bytes"]), stop_reason=int(s["stop_reason"]), reserved=[int(x) for x in s["reserved"]])
    if want["reserved"][0]:
        got.update(nal_count=0, nal_found=0, rbsp_bytes=0)          # a table error: no count means anything
    assert got == want


def make_outs(n, which=None):
    return {name: canary(n * size) for name, size in TABLES if which is None or name in which}


def check_outs(outs, want, n):
    for (name, size), w in zip(TABLES, want[:5]):
        if name not in outs:
            continue
        p = outs[name].cpu().numpy()
        got = p[: n * size].view(w.dtype)
        bad = np.flatnonzero(got != w)
        assert not len(bad), "%s differs at sample %d of %d: %d, want %d (%d differ)" % (name, bad[0], n, got[bad[0]], w[bad[0]], len(bad))
        assert (p[n * size:] == CAN).all(), "stored behind " + name


def untouched(outs):
    for name, t in outs.items():
        assert (t.cpu().numpy() == CAN).all(), "stored into " + name


def run(ctx, buf, rec, which=None, want=None):
    """plan, then a run into tables of exactly N entries; everything against the reference"""
    want = want if want is not None else S.read(buf, rec)
    assert want[5]["error"] == 0, want[5]
    d_buf = dev(np.frombuffer(buf, dtype=np.uint8))
    n = want[5]["nal_count"]
    s = call(ctx, d_buf, len(buf), rec)
    summary_matches(s, want[5])
    outs = make_outs(n, which)
    s2 = call(ctx, d_buf, len(buf), rec, sample_cap=n, outs=outs)
    summary_matches(s2, want[5])
    assert s2.tobytes() == s.tobytes(), "the plan's summary is the run's"
    check_outs(outs, want, n)
    return outs


def fails(ctx, buf, rec, n_outs=8):
    """a call that ends in an error, plan only and with outputs: the summary is the reference's, nothing else is written"""
    d_buf = dev(np.frombuffer(buf, dtype=np.uint8))
    want_plan, want = S.read(buf, rec, outputs=False)[5], S.read(buf, rec, sample_cap=n_outs)[5]
    assert want["error"] != 0
    summary_matches(call(ctx, d_buf, len(buf), rec), want_plan)
    outs = make_outs(n_outs)
    summary_matches(call(ctx, d_buf, len(buf), rec, sample_cap=n_outs, outs=outs), want)
    untouched(outs)
    return want


def offsets_of(sizes, chunk_lens, first=0, gap=3):
    """chunk offsets of chunks that lie one behind the other, `gap` bytes apart"""
    offs, at, k = [], first, 0
    for c in chunk_lens:
        offs.append(at)
        at += sum(sizes[k:k + c]) + gap
        k += c
    return offs, at


def track(rng, n, chunk_lens=None, constant=None, **kw):
    t = S.random_track(rng, n, constant=constant, **kw)
    if chunk_lens is not None:
        assert sum(chunk_lens) == n
        t["chunk_lens"] = list(chunk_lens)
    t["sizes"] = [len(x) for x in t["samples"]]
    return t


def case(t, co64=False, constant=None, first=0, file_bytes=None, **lay):
    offs, end = offsets_of(t["sizes"], t["chunk_lens"], first)
    pay = S.payloads(t["sizes"], t["chunk_lens"], offs, t["deltas"], t["cts"], t["sync"], co64, constant)
    pay.update(t.get("change", {}))
    buf, rec = S.layout(pay, **lay)
    rec["flags"] = S.CO64 if co64 else 0
    rec["file_bytes"] = end if file_bytes is None else file_bytes
    return buf, rec


# ---- round trip ---------------------------------------------------------------------------------------------------------------

def test_round_trip_annexb_progressive_file_annexb(ctx):
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(20)
    n_aus = 2 * W + 37
    counts = rng.integers(1, 4, size=n_aus)
    n = int(counts.sum())
    lens = rng.integers(2, 300, size=n)
    stream = bytearray()
    for k in range(n):
        stream += b"\x00\x00\x00\x01" + bytes(rng.integers(4, 256, size=int(lens[k]), dtype=np.uint8))
    stream = np.frombuffer(bytes(stream), dtype=np.uint8)
    d_stream = dev(stream)
    idx, _, s = ctx.index_extract(d_stream, index_cap=n + 16, want_rbsp=False)
    assert len(idx) == n
    nal_au = np.repeat(np.arange(n_aus, dtype=np.uint32), counts)
    lp, _, so, s = ctx.annexb_to_lenpref(d_stream, idx, nal_au=nal_au, n_aus=n_aus, length_size=4)
    host = lp.cpu().numpy().tobytes()
    samples = [host[int(so[a]):int(so[a + 1])] for a in range(n_aus)]
    t = S.random_track(rng, n_aus, max_chunk=9)
    data, offs = S.progressive_file(samples, t["chunk_lens"], t["deltas"], t["cts"], t["sync"], nals=NALS, track_id=4, gaps=5)
    assert len(set(t["chunk_lens"])) > 3
    rec = hbs.mp4_stbl_find(data, track_id=4)
    assert rec.tobytes() == S.find(data).tobytes()
    d_file = dev(np.frombuffer(data, dtype=np.uint8))
    off, size, dts, pts, flags, s = ctx.mp4_stbl_samples(d_file, rec)
    want = S.read(data, rec)
    for got, w in zip((off, size, dts, pts, flags), want[:5]):
        assert got.dtype == w.dtype and np.array_equal(got, w)
    summary_matches(s, want[5])
    # what went in
    assert off.tolist() == offs and size.tolist() == [len(x) for x in samples]
    want_dts = np.concatenate([[0], np.cumsum(t["deltas"][:-1])]).astype(np.int64)
    assert np.array_equal(dts.astype(np.int64), want_dts) and np.array_equal(pts.astype(np.int64), want_dts + np.array(t["cts"], dtype=np.int64))
    assert np.flatnonzero(flags == 0).tolist() == t["sync"]
    # the moov alone: on the host with its position as the base; on the device with the file's size to check offsets against
    track, sets = hbs.mp4_track_read(data)
    assert int(track["length_size"]) == 4 and int(track["track_id"]) == 4 and sets == [bytes(x) for x in NALS]
    at = data.index(b"moov") - 4
    moov = data[at:at + int.from_bytes(data[at:at + 4], "big")]
    assert hbs.mp4_stbl_find(moov, base=at).tobytes() == rec.tobytes()
    alone = hbs.mp4_stbl_find(moov)
    alone["file_bytes"] = len(data)
    got = ctx.mp4_stbl_samples(dev(np.frombuffer(moov, dtype=np.uint8)), alone)
    for g, w in zip(got[:5], want[:5]):
        assert np.array_equal(g, w)
    # and back: byte for byte the Annex-B stream
    back, _, _ = ctx.lenpref_to_annexb(d_file, off, size, length_size=4, startcode_bytes=4)
    assert np.array_equal(back.cpu().numpy(), stream)
    run(ctx, data, rec)


# ---- sizes and edges ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (0, 1, W - 1, W, W + 1, 2 * W + 1))
def test_sample_counts_around_a_workgroup(ctx, n):
    t = track(np.random.default_rng(n), n)
    run(ctx, *case(t, lead=5))
    run(ctx, *case(t, constant=None, co64=True), which=("sample_off", "sample_size", "pts"))


def test_chunk_edges_on_lane_0_and_lane_255_and_a_chunk_longer_than_two_workgroups(ctx):
    lens = [W - 1, 1, W, 1, W - 2, 1, 2 * W + 77, W - 77, 3]           # chunks begin at samples 255, 256, 512, 513, 767 (lane 255), 768 ...
    starts = np.cumsum([0] + lens[:-1])
    assert {int(x) % W for x in starts} >= {0, W - 1, 1} and max(lens) > 2 * W
    t = track(np.random.default_rng(31), sum(lens), chunk_lens=lens)
    run(ctx, *case(t))


def test_more_sample_workgroups_than_one_scan_pass(ctx):
    n = PASS * W + 3 * W + 1
    rng = np.random.default_rng(32)
    lens = [1000] * (n // 1000) + [n % 1000]
    t = dict(samples=None, sizes=[3] * n, chunk_lens=lens, deltas=[40] * n, cts=None, sync=list(range(0, n, 32)))
    buf, rec = case(t, constant=3)
    assert len(buf) < 1 << 20
    run(ctx, buf, rec)
    # sizes from a table, chunks that straddle the passes' seam, composition offsets
    sizes = rng.integers(0, 9, size=n).tolist()
    t = dict(samples=None, sizes=sizes, chunk_lens=[n - 5 * W - 9, 5 * W + 9], deltas=[1] * n, cts=[7] * (n - 1) + [0], sync=None)
    run(ctx, *case(t), which=("sample_off", "sample_size", "dts", "pts"))


# ---- stsc ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entries", (1, W + 1))
def test_stsc_entry_counts(ctx, entries):
    lens = [4] * 90 if entries == 1 else [(1, 2, 3, 0, 5)[i % 5] for i in range(W + 1)]
    t = track(np.random.default_rng(40 + entries), sum(lens), chunk_lens=lens)
    assert len(S.stsc_of(lens)) == entries
    run(ctx, *case(t))


def test_stsc_runs_that_change_with_empty_chunks_and_surplus_chunks(ctx):
    lens = [0, 0, 3, 3, 3, 0, 7, 7, 1, 0, 0, 0, 300, 300, 2, 2, 2, 2, 0, 5]
    rng = np.random.default_rng(41)
    t = track(rng, sum(lens), chunk_lens=lens)
    run(ctx, *case(t))
    # N below what the chunks hold: surplus chunks, surplus room in the last chunk used, surplus stts and ctts counts, stss numbers above N
    for n in (sum(lens) - 8, sum(lens) - 5, 620, 9, 8, 0):
        t2 = dict(t, change={"stsz": S.p_stsz(t["sizes"][:n])})
        buf, rec = case(t2)
        want = S.read(buf, rec)
        assert want[5]["nal_count"] == n and want[5]["nal_found"] == len(lens)
        run(ctx, buf, rec, want=want)


# ---- stts, ctts, stss ---------------------------------------------------------------------------------------------------------

def test_stts_and_ctts_of_one_entry_and_of_an_entry_a_sample(ctx):
    n = 3 * W + 5
    rng = np.random.default_rng(50)
    t = track(rng, n)
    for deltas, cts in (([3000] * n, [6000] * n), (list(range(1, n + 1)), list(range(n, 2 * n))), ([3000] * n, list(range(n, 2 * n))),
                        (list(range(1, n + 1)), None)):
        t2 = dict(t, deltas=deltas, cts=cts)
        buf, rec = case(t2)
        assert int(rec["stts"][0][1]) == 8 + 8 * (1 if deltas[0] == deltas[1] else n)
        run(ctx, buf, rec)


def test_entries_of_count_0_ctts_versions_and_a_short_ctts(ctx):
    n = 2 * W + 9
    t = track(np.random.default_rng(51), n, reorder=False)
    stts = [(0, 99), (0, 5), (W, 10), (0, 1 << 31), (0, 7), (1, 20), (n - W - 1, 30), (0, 1), (5, 9), (0, 2)]
    for ctts in (S.p_pairs([(0, 5), (W - 1, 40), (0, M), (2, 0), (n, 17)], version=0),
                 S.p_pairs([(3, 50), (0, -9), (W, -1), (W + 20, 1 << 30)], version=1, signed=True),        # 14 samples short
                 S.p_pairs([(n - 1, M)], version=0),                                                       # unsigned: 2^32 - 1
                 S.p_pairs([(0, -1)], version=1, signed=True), S.p_pairs([], version=1)):
        t2 = dict(t, change={"stts": S.p_pairs(stts), "ctts": ctts})
        run(ctx, *case(t2))


@pytest.mark.parametrize("kind", ("absent", "empty", "all", "every 32nd", "above N"))
def test_stss(ctx, kind):
    n = 2 * W + 40
    t = track(np.random.default_rng(52), n)
    numbers = dict(absent=None, empty=[], all=list(range(1, n + 1)))
    numbers["every 32nd"] = list(range(1, n + 1, 32))
    numbers["above N"] = [1, W, W + 1, n, n + 1, n + 2, M]
    x = numbers[kind]
    t2 = dict(t, change={"stss": None if x is None else S.p_stss(x)})
    outs = run(ctx, *case(t2))
    want_sync = {None: n, 0: 0}.get(None if x is None else len(x), len([v for v in x or [] if v <= n]))
    assert int((outs["sample_flags"][: 4 * n].cpu().numpy().view(np.uint32) == 0).sum()) == want_sync


def test_co64_offsets_above_4_gib(ctx):
    t = track(np.random.default_rng(53), W + 30)
    buf, rec = case(t, co64=True, first=(1 << 40) + 12345)
    assert int(rec["file_bytes"][0]) > 1 << 40 and len(buf) < 1 << 16
    outs = run(ctx, buf, rec)
    assert int(outs["sample_off"][: 8 * (W + 30)].cpu().numpy().view(np.uint64).min()) >= (1 << 40) + 12345


@pytest.mark.parametrize("align", range(16))
def test_tables_at_every_alignment_the_last_box_ending_the_buffer(ctx, align):
    t = track(np.random.default_rng(60 + align), W + 3 + align)
    order = S.BOXES[align % 6:] + S.BOXES[:align % 6]
    buf, rec = case(t, co64=bool(align & 1), lead=align % 5, align=align, order=order)
    last = order[-1]
    assert int(rec[last][0][0]) + int(rec[last][0][1]) == len(buf)
    assert all(int(rec[b][0][0]) % 16 == align for b in S.BOXES)
    run(ctx, buf, rec)


# ---- counts that nothing in the box bounds ---------------------------------------------------------------------------------------

def test_counts_of_2_to_the_32_minus_1(ctx):
    huge = dict(stsz=S.p_stsz([], constant=7, count=M), stco=S.p_stco([0] * 3), stsc=S.p_stsc([(1, M)]), stts=S.p_pairs([(M, M)]), ctts=None, stss=None)
    rights = 0
    for ch in ({}, {"stsc": S.p_stsc([(1, 1), (2, M)])}, {"stsc": S.p_stsc([(1, 1)])}, {"stts": S.p_pairs([(M - 1, 1)])}, {"stts": S.p_pairs([(M, M)] * 5)},
               {"stsz": S.p_stsz([], constant=0, count=M)}, {"stsc": S.p_stsc([(1, M), (2, M), (3, M)])},
               {"stts": S.p_pairs([(0, M), (M, 0)]), "ctts": S.p_pairs([(M, M)] * 3), "stss": S.p_stss([M])}):
        p = dict(huge)
        p.update(ch)
        buf, rec = S.layout(p)
        rec["file_bytes"] = 1 << 62
        d_buf = dev(np.frombuffer(buf, dtype=np.uint8))
        want = S.read(buf, rec, outputs=False)[5]
        summary_matches(call(ctx, d_buf, len(buf), rec), want)
        if want["error"] == 0:
            rights += 1
            assert want["nal_count"] == M and want["rbsp_bytes"] == 7 * M
            outs = make_outs(100)
            summary_matches(call(ctx, d_buf, len(buf), rec, sample_cap=100, outs=outs), S.summary(S.E_CAPACITY, M, 3, 0, len(buf)))
            untouched(outs)
    assert rights == 5


# ---- errors -------------------------------------------------------------------------------------------------------------------

SIZES, LENS, OFFS, DELTAS = [4, 5, 6, 7], [3, 1], [100, 200], [10, 10, 10, 10]


def small(change, file_bytes=1000, co64=False, **lay):
    pay = S.payloads(SIZES, LENS, OFFS, DELTAS, cts=[0, 5, 0, 0], sync=[0, 2], co64=co64)
    pay.update(change)
    buf, rec = S.layout(pay, lead=3, **lay)
    rec["file_bytes"] = file_bytes
    rec["flags"] = S.CO64 if co64 else 0
    return buf, rec


TABLE_ERRORS = [
    (1, {"stsz": S.p_stsz(SIZES, count=5)}), (1, {"stsz": S.p_stsz(SIZES, version=1)}), (1, {"stsz": S.p_stsz(SIZES)[:11]}),
    (2, {"stco": S.p_stco(OFFS, version=1)}), (2, {"stco": S.p_stco(OFFS, count=3)}), (2, {"stco": S.p_stco(OFFS)[:7]}),
    (3, {"stsc": S.p_stsc([(1, 3), (1, 1)])}), (3, {"stsc": S.p_stsc([(1, 3), (3, 1)])}), (3, {"stsc": S.p_stsc([(2, 3)])}),
    (3, {"stsc": S.p_stsc([(1, 1)])}), (3, {"stsc": S.p_stsc([(1, 3), (2, 0)])}), (3, {"stsc": S.p_stsc([(1, 3)], version=1)}), (3, {"stsc": S.p_stsc([])}),
    (3, {"stsc": S.p_stsc([(1, 4)], count=2)}), (3, {"stsc": S.p_stsc([(0, 4)])}),
    (4, {"stts": S.p_pairs([(3, 10)])}), (4, {"stts": S.p_pairs([(4, 1)], version=1)}), (4, {"stts": S.p_pairs([(4, 1)], count=2)}), (4, {"stts": S.p_pairs([])}),
    (5, {"ctts": S.p_pairs([(1, 0)], version=2)}), (5, {"ctts": S.p_pairs([(1, 7)], count=2)}), (5, {"ctts": b"\x00\x00\x00"}),
    (6, {"stss": S.p_stss([2, 2])}), (6, {"stss": S.p_stss([0])}), (6, {"stss": S.p_stss([3, 1])}), (6, {"stss": S.p_stss([3], version=1)}),
    (6, {"stss": S.p_stss([3], count=2)}),
    (4, {"stts": S.p_pairs([(3, 10)]), "stss": S.p_stss([0])}), (3, {"stsc": S.p_stsc([(1, 1)]), "ctts": S.p_pairs([(1, 0)], version=2)}),
    (1, {"stsz": S.p_stsz(SIZES, count=5), "stco": S.p_stco(OFFS, version=1)}),
]


def test_every_table_error_at_its_box(ctx):
    assert S.read(*small({}))[5]["error"] == 0
    for box, change in TABLE_ERRORS:
        want = fails(ctx, *small(change))
        assert want == S.summary(S.E_ARG, total=want["stream_bytes"], bad=(box, 0, 0)), (box, change)
    # a broken entry far down a table: each workgroup's word reaches the scan
    n = 3 * W
    t = track(np.random.default_rng(70), n, chunk_lens=[(1, 2)[i % 2] for i in range(2 * W)])
    entries = S.stsc_of(t["chunk_lens"])
    for at in (W - 1, W, 2 * W - 1):
        broken = list(entries)
        broken[at] = (broken[at - 1][0], broken[at][1])
        buf, rec = case(dict(t, change={"stsc": S.p_stsc(broken)}))
        assert fails(ctx, buf, rec)["reserved"] == [3, 0, 0]
    numbers = list(range(1, n + 1))
    numbers[2 * W + 7] = numbers[2 * W + 6]
    buf, rec = case(dict(t, change={"stss": S.p_stss(numbers)}))
    assert fails(ctx, buf, rec)["reserved"] == [6, 0, 0]


def test_every_sample_error_at_the_lowest_sample(ctx):
    cases = [
        (2, small({}, file_bytes=114)), (0, small({}, file_bytes=103)), (3, small({}, file_bytes=206)),             # off + size above file_bytes
        (3, small({"stco": S.p_stco([100, (1 << 32) - 3])})),
        (3, small({"stco": S.p_stco([100, (1 << 64) - 2], co64=True)}, co64=True, file_bytes=1 << 62)),                 # the sum would wrap
        (0, small({"stco": S.p_stco([(1 << 64) - 1, 5], co64=True)}, co64=True, file_bytes=1 << 62)),
        (2, small({"ctts": S.p_pairs([(2, 0), (1, -21)], version=1, signed=True)})),                                   # pts below 0
        (1, small({"ctts": S.p_pairs([(1, 0), (3, -11)], version=1, signed=True)})),
    ]
    for bad, (buf, rec) in cases:
        d_buf = dev(np.frombuffer(buf, dtype=np.uint8))
        want = S.read(buf, rec, sample_cap=4)[5]
        assert want == S.summary(S.E_ARG, 4, 2, 0, len(buf), bad=(0, 0, bad + 1))
        assert S.read(buf, rec, outputs=False)[5]["error"] == 0
        summary_matches(call(ctx, d_buf, len(buf), rec), S.read(buf, rec, outputs=False)[5])          # a plan does not look for them
        outs = make_outs(4)
        summary_matches(call(ctx, d_buf, len(buf), rec, sample_cap=4, outs=outs), want)
        untouched(outs)
    # times: with 32-bit deltas a dts of 2^62 takes 2^30 samples, more than a test can hold, so that limit is checked on the rule
    # functions alone (tests/test_mp4_stbl_host_asan.py); here the largest deltas and offsets there are, which are no error,
    # and a pts below 0 far down the table
    n = W + 20
    t = track(np.random.default_rng(71), n, reorder=False)
    for stts, ctts, v, bad in (([(5, M)] + [(1, M)] * (n - 5), [(n, M)], 0, None), ([(M, M), (M, M), (1, 1)], None, 0, None),
                               ([(1, M)] * n, [(n, -(1 << 31))], 1, 0), ([(W + 3, 9), (n, 0)], [(W + 9, 0), (1, -9 * (W + 3) - 1)], 1, W + 9),
                               ([(W + 3, 9), (n, 0)], [(W + 9, 0), (1, -9 * (W + 3))], 1, None)):
        change = {"stts": S.p_pairs(stts), "ctts": None if ctts is None else S.p_pairs(ctts, version=v, signed=v == 1)}
        buf, rec = case(dict(t, change=change))
        want = S.read(buf, rec, sample_cap=n)
        if bad is None:
            assert want[5]["error"] == 0
            run(ctx, buf, rec, want=want)
        else:
            assert want[5]["reserved"] == [0, 0, bad + 1]
            assert fails(ctx, buf, rec, n_outs=n) == want[5]
    # several bad samples in several workgroups: the lowest
    t = track(np.random.default_rng(72), 3 * W, chunk_lens=[W - 10, W + 20, W - 10])
    offs, _ = offsets_of(t["sizes"], t["chunk_lens"])
    t2 = dict(t, change={"stco": S.p_stco([offs[0], 1 << 31, 1 << 30])})
    buf, rec = case(t2)
    assert fails(ctx, buf, rec, n_outs=3 * W)["reserved"] == [0, 0, W - 10 + 1]          # the second chunk's first sample


def test_capacity(ctx):
    t = track(np.random.default_rng(73), W + 1)
    buf, rec = case(t)
    d_buf = dev(np.frombuffer(buf, dtype=np.uint8))
    for cap in (0, 1, W):
        outs = make_outs(cap)
        summary_matches(call(ctx, d_buf, len(buf), rec, sample_cap=cap, outs=outs), S.summary(S.E_CAPACITY, W + 1, len(t["chunk_lens"]), 0, len(buf)))
        untouched(outs)
    want = S.read(buf, rec)
    outs = make_outs(W + 1)
    summary_matches(call(ctx, d_buf, len(buf), rec, sample_cap=4 * W, outs=outs), want[5])          # more room than samples
    check_outs(outs, want, W + 1)


def test_argument_refusals(ctx):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    buf, rec = small({})
    d = dev(np.frombuffer(buf, dtype=np.uint8))
    summary = torch.full((SUMMARY.itemsize + 16,), 0x11, dtype=torch.uint8, device="cuda")
    o = make_outs(4)
    good = dict(sample_cap=4, **o)
    E = S.E_ARG

    def rc(tables=rec, data=d, nbytes=len(buf), summ=summary[:SUMMARY.itemsize], **kw):
        return ctx.mp4_stbl_samples_async(data, nbytes, tables, summ, **kw)
    assert rc(**good) == 0 and rc() == 0
    for field, value in (("flags", 2), ("flags", 1 << 31), ("reserved0", 1), ("file_bytes", (1 << 62) + 1)):
        r = rec.copy()
        r[field] = value
        assert rc(tables=r, **good) == E, field
    for i in range(2):
        r = rec.copy()
        r["reserved"][0][i] = 1
        assert rc(tables=r, **good) == E
    for name in S.BOXES:
        r = rec.copy()
        r[name][0][1] = 0
        assert rc(tables=r, **good) == (E if name in ("stsz", "stco", "stsc", "stts") else 0), name
        r = rec.copy()
        r[name][0][0] = len(buf) - int(r[name][0][1]) + 1                # one byte past the buffer
        assert rc(tables=r, **good) == E, name
        r[name][0][0] = (1 << 64) - 4                                    # off + bytes wraps
        assert rc(tables=r, **good) == E, name
        r[name][0] = (len(buf) + 1, 1)
        assert rc(tables=r, **good) == E, name
    assert rc(nbytes=(1 << 62) + 1, **good) == E
    assert rc(sample_cap=4, sample_off=o["sample_off"]) == E and rc(sample_cap=4, sample_size=o["sample_size"]) == E
    for name in ("dts", "pts", "sample_flags"):
        assert rc(sample_cap=4, **{name: o[name]}) == E
    assert rc(**dict(good, sample_cap=1 << 32)) == E
    assert rc(sample_cap=1 << 32) == 0                                   # plan only: sample_cap sizes nothing
    for name, step in (("sample_off", 4), ("sample_size", 4), ("dts", 4), ("pts", 4), ("sample_flags", 2)):
        assert rc(**dict(good, **{name: o[name][step:]})) == E
    assert rc(data=d[8:], **good) == E and rc(summ=summary[8:8 + SUMMARY.itemsize], **good) == E
    assert rc(tables=None, **good) == E and rc(data=None, **good) == E and rc(summ=None, **good) == E
    for t in o.values():
        t.fill_(CAN)
    assert rc(sample_cap=4, sample_off=o["sample_off"], sample_size=o["sample_size"]) == 0          # the optional tables are optional
    torch.cuda.synchronize()
    assert (o["dts"].cpu().numpy() == CAN).all()


# ---- a HIP graph ---------------------------------------------------------------------------------------------------------------

def test_one_replay_from_a_graph_on_other_contents(ctx):
    """captured on a side stream after one warm-up call, replayed on other contents of the same buffers with the same box
    layout: other sizes, chunks, times and sync samples, another N; every host argument is the same"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    n = 2 * W + 50
    members, rec = [], None
    for seed, count in ((80, n), (81, n - W - 7)):
        t = track(np.random.default_rng(seed), n, chunk_lens=[2] * (n // 2))
        t["deltas"] = list(range(seed, seed + n))
        t["cts"] = list(range(n))
        t["sync"] = list(range(seed % 2, n, 2))
        # (every table keeps its length: the stsz claims fewer samples, the rest is surplus)
        t["change"] = {"stsz": S.p_stsz(t["sizes"], count=count)}
        buf, r = case(t, file_bytes=1 << 30)
        assert rec is None or (r.tobytes() == rec.tobytes() and len(buf) == len(members[0]))
        members.append(buf)
        rec = r
    wants = [S.read(b, rec) for b in members]
    assert [w[5]["nal_count"] for w in wants] == [n, n - W - 7]
    size = len(members[0])
    d = dev(np.frombuffer(members[0], dtype=np.uint8))
    outs = make_outs(n)
    summary = torch.full((SUMMARY.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")

    def launch():
        return ctx.mp4_stbl_samples_async(d, size, rec, summary, sample_cap=n, **outs)

    def check(want):
        summary_matches(ctx.read_summary(summary), want[5])
        check_outs(outs, want, want[5]["nal_count"])
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
        d.copy_(torch.from_numpy(np.frombuffer(members[which], dtype=np.uint8).copy()))
        for t in outs.values():
            t.fill_(CAN)
        summary.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        check(wants[which])
    assert ctx.device_bytes() == held
