"""hbs_mp4_samples on the GPU against the box-by-box reader of tests/_mp4_read_ref.py, entry for entry: plan first, then a run into
tables of exactly the planned capacity with canaries behind every one of them, every summary field checked; the round trip
from hbs_mp4_fragment and on through hbs_lenpref_to_annexb and hbs_index_extract."""
import struct

import numpy as np
import pytest

from tests import _mp4_ref as R
from tests import _mp4_read_ref as Q

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 1024
W = 256                         # segments, moofs and samples of a workgroup (kRdLanes: hbs_mp4rd.h)
PASS = 256 * 8                  # workgroups scan_parts / seg_scan_parts take in one pass (kPlanLanes * kPlanPer: hbs_plan.h)
FRAG = R.FRAG.itemsize
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


def seg_table(segs, stride):
    """records of `stride` bytes: offset, size, then junk"""
    t = np.full((len(segs), stride // 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    for i, (o, n) in enumerate(segs):
        t[i, 0], t[i, 1] = o, n
    return dev(t)


def call(ctx, d_buf, nbytes, prm, seg=None, stride=16, n_segs=0, moof_cap=0, sample_cap=0, outs=None, fill=0x5A):
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), fill, dtype=torch.uint8, device="cuda")
    rc = ctx.mp4_samples_async(d_buf, nbytes, hbs.mp4_read_params(**prm), summary, seg=seg, seg_stride=stride, n_segs=n_segs,
                               moof_cap=moof_cap, sample_cap=sample_cap, **(outs or {}))
    assert rc == 0, rc
    return ctx.read_summary(summary)


def summary_matches(s, want):
    got = dict(error=int(s["error"]), nal_count=int(s["nal_count"]), nal_found=int(s["nal_found"]), rbsp_bytes=int(s["rbsp_bytes"]),
               stream_bytes=int(s["stream_bytes"]), stop_reason=int(s["stop_reason"]), reserved=[int(x) for x in s["reserved"]])
    if want["reserved"][0]:
        got.update(nal_count=0, nal_found=0, rbsp_bytes=0)          # a chain error: no count means anything
    assert got == want


def make_outs(n, m, which=None):
    outs = {name: canary(n * size) for name, size in TABLES if which is None or name in which}
    if which is None or "frag" in which:
        outs["frag"] = canary(m * FRAG)
    return outs


def check_outs(outs, want, n, m):
    for (name, size), w in zip(TABLES, want[:5]):
        if name not in outs:
            continue
        p = outs[name].cpu().numpy()
        got = p[: n * size].view(w.dtype)
        bad = np.flatnonzero(got != w)
        assert not len(bad), "%s differs at sample %d of %d: %d, want %d (%d differ)" % (name, bad[0], n, got[bad[0]], w[bad[0]], len(bad))
        assert (p[n * size:] == CAN).all(), "stored behind " + name
    if "frag" in outs:
        p = outs["frag"].cpu().numpy()
        got = p[: m * FRAG].view(R.FRAG)
        for f in R.FRAG.names:
            assert np.array_equal(got[f], want[5][f]), ("d_frag." + f, np.flatnonzero(got[f] != want[5][f])[:4])
        assert (p[m * FRAG:] == CAN).all(), "stored behind d_frag"


def run(ctx, buf, segs, prm, stride=16, want=None, d_buf=None, which=None):
    """plan, then a run into tables of exactly the planned capacity; everything against the reference (or `want`)"""
    want = want if want is not None else Q.samples(buf, segs, prm)
    assert want[6]["error"] == 0, want[6]
    d_buf = dev(np.frombuffer(buf, dtype=np.uint8)) if d_buf is None else d_buf
    kw = dict(seg=None if segs is None else seg_table(segs, stride), stride=stride, n_segs=0 if segs is None else len(segs))
    n, m = want[6]["nal_count"], want[6]["nal_found"]
    s = call(ctx, d_buf, len(buf), prm, moof_cap=m, **kw)
    summary_matches(s, want[6])
    outs = make_outs(n, m, which)
    s2 = call(ctx, d_buf, len(buf), prm, moof_cap=m, sample_cap=n, outs=outs, **kw)
    summary_matches(s2, want[6])
    assert s2.tobytes() == s.tobytes(), "the plan's summary is the run's"
    check_outs(outs, want, n, m)
    return outs


# ---- round trip ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", (1, 2, 4))
@pytest.mark.parametrize("times", (False, True))
def test_round_trip_from_mp4_fragment_and_on_to_annexb(ctx, L, times):
    rng = np.random.default_rng(300 + L + 10 * times)
    n_aus = 3 * W + 40
    counts = rng.integers(1, 4, size=n_aus)
    n = int(counts.sum())
    lens = rng.integers(2, 250 if L == 1 else 700, size=n)
    starts = np.cumsum(4 + np.concatenate([[0], lens[:-1]]))
    stream = rng.integers(4, 256, size=int(starts[-1] + lens[-1]), dtype=np.uint8)          # no zero byte: a walk finds the payloads alone
    keep = (rng.integers(0, 4, size=n) != 0).astype(np.uint8)
    nal_au = np.repeat(np.arange(n_aus, dtype=np.uint32), counts)
    keep[nal_au == 7] = 0
    au = R.au_records((np.arange(n_aus) % 9 == 0).astype(np.uint32))
    dts = pts = None
    if times:
        dts = ((1 << 40) + np.cumsum(rng.integers(0, 6000, size=n_aus))).astype(np.uint64)
        pts = (dts.astype(np.int64) + rng.integers(-5000, 20000, size=n_aus)).astype(np.uint64)          # negative composition offsets
        assert (pts < dts).any()
    out, so, ss, frags, s = ctx.mp4_fragment(dev(stream), R.entries(starts, starts + lens), nal_au, au, keep=keep, dts=dts, pts=pts,
                                             length_size=L, flags=R.CUT_AT_IRAP, max_samples=5, track_id=3, sequence=40, sample_duration=3000,
                                             base_time=1 << 33)
    host = out.cpu().numpy().tobytes()
    if dts is None:
        dts = (1 << 33) + 3000 * np.arange(n_aus, dtype=np.uint64)
        pts = dts
    flags = np.where(au["flags"] & R.AU_IRAP, 0x02000000, 0x01010000).astype(np.uint32)
    want = (so, ss, dts, pts, flags, frags, Q.summary(0, n_aus, len(frags), int(ss.sum()), len(host)))
    plain = [(int(f["out_off"]), int(f["out_bytes"])) for f in frags]
    prm = Q.read_params(track_id=3)
    # the fragment table of hbs_mp4_fragment as it is, at stride 48
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import SUMMARY
    outs = make_outs(n_aus, len(frags))
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    assert ctx.mp4_samples_async(out, len(host), hbs.mp4_read_params(**prm), summary, seg=dev(frags), seg_stride=FRAG, n_segs=len(frags),
                                 moof_cap=len(frags), sample_cap=n_aus, **outs) == 0
    summary_matches(ctx.read_summary(summary), want[6])
    check_outs(outs, want, n_aus, len(frags))
    # a plain table, and one segment
    run(ctx, host, plain, prm, want=want, d_buf=out)
    outs = run(ctx, host, None, prm, want=want, d_buf=out)
    # the reference reads the same
    ref = Q.samples(host, plain, prm)
    for a, b in zip(ref[:6], want[:6]):
        assert np.array_equal(a, b)
    # and on: Annex-B, and the index of it
    back, _, _ = ctx.lenpref_to_annexb(out, outs["sample_off"][: n_aus * 8].cpu().numpy().view(np.uint64),
                                       outs["sample_size"][: n_aus * 8].cpu().numpy().view(np.uint64), length_size=L, startcode_bytes=4)
    idx, _, _ = ctx.index_extract(back, index_cap=n + 16, want_rbsp=False)
    b = back.cpu().numpy()
    kept = np.flatnonzero(keep)
    assert len(idx) == len(kept)
    for e, k in zip(idx, kept):
        assert b[int(e["start"]):int(e["end"])].tobytes() == stream[starts[k]:starts[k] + lens[k]].tobytes()


def test_convenience_call(ctx):
    rng = np.random.default_rng(7)
    prm = Q.read_params(track_id=2, trex_duration=1000, trex_size=9, trex_flags=0x01010000)
    buf, segs, expect, frags = Q.random_segments(rng, 3, prm)
    got = ctx.mp4_samples(dev(np.frombuffer(buf, dtype=np.uint8)), seg=np.array(segs, dtype=np.uint64), **prm)
    for a, b in zip(got[:5], Q.expected_tables(expect)):
        assert np.array_equal(a, b)
    assert np.array_equal(got[5], frags)


# ---- general fragments --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_general_fragments(ctx, seed):
    """every tfhd and trun flag, both versions of trun and tfdt, largesize boxes, size 0 last boxes, foreign boxes and trafs,
    several truns with and without data_offset, base_data_offset; all cases valid, none skipped"""
    for sub in range(8):
        rng = np.random.default_rng(1000 + 8 * seed + sub)
        prm = Q.read_params(track_id=int(rng.integers(0, 3)), trex_duration=int(rng.integers(1, 9000)), trex_size=int(rng.integers(0, 30)),
                            trex_flags=int(rng.integers(0, 1 << 32)))
        n_segs = int(rng.integers(1, 5))
        buf, segs, expect, frags = Q.random_segments(rng, n_segs, prm, lead=int(rng.integers(0, 4)) * 16)
        want = Q.samples(buf, segs, prm)
        assert want[6]["error"] == 0
        for a, b in zip(want[:5], Q.expected_tables(expect)):
            assert np.array_equal(a, b)
        assert np.array_equal(want[5], frags)
        run(ctx, buf, segs, prm, stride=(16, 24, 48)[sub % 3], want=want)
        if n_segs == 1 and segs[0] == (0, len(buf)):
            run(ctx, buf, None, prm, want=want, which=("sample_off", "sample_size", "pts"))


# ---- workgroup and scan edges -------------------------------------------------------------------------------------------------

def moofs_of(rng, prm, shapes, tflags=None, per_seg=None):
    """shapes: per moof the sample counts of its truns.  One segment, or a segment (a file of its own: base_data_offset counts
    from its first byte) every per_seg moofs."""
    buf, expect, frags, seg_off = bytearray(), [], [], 0
    for i, counts in enumerate(shapes):
        at = len(buf)
        if per_seg and i % per_seg == 0:
            seg_off = at
        b, e, f = Q.random_moof(rng, at, seg_off, prm, counts=list(counts), first_sample=len(expect), plain=True,
                                tflags=None if tflags is None else tflags[i])
        buf += b
        expect += e
        frags.append((f[0], len(b), f[1], f[2], f[3], f[4], f[5], 0))
    return bytes(buf), expect, np.array(frags, dtype=R.FRAG)


def run_shapes(ctx, seed, shapes, tflags=None):
    rng = np.random.default_rng(seed)
    prm = Q.read_params(track_id=1, trex_duration=7, trex_size=3, trex_flags=0x01010000)
    buf, expect, frags = moofs_of(rng, prm, shapes, tflags)
    want = Q.samples(buf, None, prm)
    assert want[6]["error"] == 0 and np.array_equal(want[5], frags)
    for a, b in zip(want[:5], Q.expected_tables(expect)):
        assert np.array_equal(a, b)
    run(ctx, buf, None, prm, want=want)


@pytest.mark.parametrize("total", (1, W - 1, W, W + 1, 2 * W + 1))
def test_sample_totals_around_a_workgroup(ctx, total):
    run_shapes(ctx, 40 + total, [[total]])
    if total > 2:
        run_shapes(ctx, 41 + total, [[total - 2, 2]])


def test_truns_across_workgroups_and_restarts_on_lane_0_and_255(ctx):
    D = 0x201                   # sizes in the entries, a data_offset: the sizes' sum restarts at the trun
    C = 0x200                   # ... no data_offset: it continues the trun in front
    # a trun that straddles a workgroup boundary; one that covers several whole workgroups
    run_shapes(ctx, 60, [[200, 100]], [[D, C]])
    run_shapes(ctx, 61, [[10, 3 * W + 11, 5]], [[D | 0x100, C | 0x800, D]])
    run_shapes(ctx, 62, [[W - 6, 3 * W, 6]])
    # the sizes restart on lane 255 and on lane 0 (a trun with a data_offset begins at samples 255, 256 and 512) ...
    run_shapes(ctx, 63, [[W - 1, 1, W, 9]], [[D, D, D | 0x100, D]])
    # ... and do not, at the same places
    run_shapes(ctx, 64, [[W - 1, 1, W, 9]], [[D, C, C | 0x100, C]])
    # the durations restart on lane 255 and on lane 0 (a moof begins there), with durations in the entries
    T = 0x301
    run_shapes(ctx, 65, [[W - 1], [1], [W], [9]], [[T], [T], [T], [T]])
    run_shapes(ctx, 66, [[W - 1], [1, W, 9]], [[T], [T, T & ~1, T]])


def test_empty_moofs_and_empty_truns(ctx):
    run_shapes(ctx, 70, [[5], [], [4]])                      # a moof of no trun between two others
    run_shapes(ctx, 71, [[5], [0], [4]])                     # ... of one empty trun
    for flags in ([0x201, 0x201, 0x200], [0x201, 0x200, 0x200], [0x200, 0x201, 0x201], [0x201, 0x201, 0x201]):
        run_shapes(ctx, 72 + flags[1] + flags[2], [[6, 0, 7]], [flags])      # a trun of count 0, with and without a data_offset
    run_shapes(ctx, 75, [[0, 0, 3], [0]])
    run_shapes(ctx, 76, [[], [], []])


@pytest.mark.parametrize("moofs", (W - 1, W, W + 1))
def test_moof_counts_around_a_workgroup(ctx, moofs):
    prm = Q.read_params(track_id=1, trex_duration=7, trex_size=3)
    for per_seg in (None, 1, 2):
        rng = np.random.default_rng(80 + moofs)
        buf, expect, frags = moofs_of(rng, prm, [[int(c)] for c in rng.integers(0, 4, size=moofs)], per_seg=per_seg)
        segs = None
        if per_seg:
            # a segment a moof, or every two; the segments in another order than the buffer's
            cut = [int(f["out_off"]) for f in frags[::per_seg]] + [len(buf)]
            segs = [(a, b - a) for a, b in zip(cut, cut[1:])]
        want = Q.samples(buf, segs, prm)
        assert want[6]["nal_found"] == moofs and np.array_equal(want[5], frags)
        for a, b in zip(want[:5], Q.expected_tables(expect)):
            assert np.array_equal(a, b)
        run(ctx, buf, segs, prm, want=want)
        if per_seg == 2:
            run(ctx, buf, segs[::-1], prm)


def test_more_sample_workgroups_than_one_scan_pass(ctx):
    """525 000 samples in five moofs of one trun with 4-byte entries (the sizes): 2051 workgroups of samples, more than the 2048
    one pass of the segmented scan takes.  The expectation is numpy's cumulative sum, not the Python reader."""
    rng = np.random.default_rng(90)
    per, moofs = 105000, 5
    assert (per * moofs + W - 1) // W > PASS
    buf, want_off, want_size, want_dts, frags = bytearray(), [], [], [], []
    for m in range(moofs):
        sizes = rng.integers(0, 4, size=per).astype(">u4")
        time, dur = int(rng.integers(0, 1 << 40)), int(rng.integers(1, 4000))

        def make(off):
            return Q.box(b"moof", Q.mfhd(m + 1) + Q.box(b"traf", Q.tfhd(1, 0x020028, dur=dur, sflags=0x01010000) + Q.tfdt(time) + Q.full(
                b"trun", 0, 0x201, struct.pack(">Ii", per, off) + sizes.tobytes())))
        moof = make(0)
        moof = make(len(moof) + 8)
        at = len(buf)
        total = int(sizes.astype(np.uint64).sum())
        buf += moof + Q.box(b"mdat", bytes(total))
        want_off.append(at + len(moof) + 8 + np.concatenate([[0], np.cumsum(sizes.astype(np.uint64))[:-1]]).astype(np.uint64))
        want_size.append(sizes.astype(np.uint64))
        want_dts.append(np.uint64(time) + np.uint64(dur) * np.arange(per, dtype=np.uint64))
        frags.append((at, len(moof) + 8 + total, m * per, time, per, m + 1, 0, 0))
    n = per * moofs
    dts = np.concatenate(want_dts)
    size = np.concatenate(want_size)
    want = (np.concatenate(want_off), size, dts, dts, np.full(n, 0x01010000, dtype=np.uint32), np.array(frags, dtype=R.FRAG),
            Q.summary(0, n, moofs, int(size.sum()), len(buf)))
    run(ctx, bytes(buf), None, Q.read_params(track_id=1), want=want)


def test_truns_whose_entries_have_no_bytes(ctx):
    """a trun without 0x100 .. 0x800 holds its count and nothing else, so 2^32 - 1 samples fit 16 bytes: the plan must not
    take a step a sample.  Three million good samples with tables; then counts of 2^32 - 1, three hundred of them in one moof,
    good, leaving the buffer and leaving the time range -- each plan is a few launches whatever the counts say"""
    prm = Q.read_params(track_id=1)

    def moof(truns, hflags, **tf):
        def make(off):
            return Q.box(b"moof", Q.mfhd(9) + Q.box(b"traf", Q.tfhd(1, hflags, **tf) + Q.tfdt(1000) + b"".join(
                Q.trun(fl, [], 0, off, 0x02000000, count=c) for fl, c in truns)))
        return make(len(make(0)) + 8)
    n = 3_000_000
    buf = moof([(5, n)], 0x020038, dur=2, size=1, sflags=0x01010000) + Q.box(b"mdat", bytes(n))
    want = Q.samples(buf, None, prm)
    assert want[6] == Q.summary(0, n, 1, n, len(buf)) and int(want[0][-1]) == len(buf) - 1 and int(want[2][-1]) == 1000 + 2 * (n - 1)
    assert int(want[4][0]) == 0x02000000 and int(want[4][1]) == 0x01010000 and int(want[5]["flags"][0]) == R.AU_IRAP
    run(ctx, buf, None, prm, want=want)
    big = (1 << 32) - 1
    for truns, tf, mdat in (([(1, big)] * 300, dict(dur=0, size=0), 16),                      # all good: 300 x (2^32 - 1) samples of no bytes
                            ([(0x201, 0)] + [(0, big)] * 3, dict(dur=1, size=1), 5000),        # leaves the buffer at the 5001st
                            ([(1, 1 << 29), (0, 7), (1, big)], dict(dur=(1 << 32) - 1, size=0), 8),  # dts reaches 2^62 in the third trun
                            ([(1, 5), (1, big)], dict(dur=0, size=3), 3 * 5 + 2)):            # the second trun leaves the buffer at its sixth
        buf = moof(truns, 0x020038, sflags=0, **tf) + Q.box(b"mdat", bytes(mdat))
        want = Q.samples(buf, None, prm, tables=False)[6]
        d = dev(np.frombuffer(buf, dtype=np.uint8))
        summary_matches(call(ctx, d, len(buf), prm, moof_cap=1), want)
        if want["error"] == 0:
            assert want["nal_count"] == 300 * big
        else:
            assert want["reserved"][2] > 0
        # with outputs the count is above any sample_cap: nothing is read, nothing written
        outs = make_outs(100, 1)
        summary_matches(call(ctx, d, len(buf), prm, moof_cap=1, sample_cap=100, outs=outs),
                        Q.summary(Q.E_CAPACITY, want["nal_count"], 1, 0, len(buf)))
        for t in outs.values():
            assert (t.cpu().numpy() == CAN).all()


# ---- errors, capacity, refusals -----------------------------------------------------------------------------------------------

def untouched(ctx, buf, segs, prm, moof_cap=None, sample_cap=None):
    """the reference's error, from the plan (unless it is sample_cap's) and from a run; the canary-filled tables untouched"""
    want = Q.samples(buf, segs, prm, moof_cap=moof_cap, sample_cap=sample_cap)[6]
    assert want["error"] != 0
    d_buf = dev(np.frombuffer(buf, dtype=np.uint8))
    kw = dict(seg=None if segs is None else seg_table(segs, 16), n_segs=0 if segs is None else len(segs))
    ok = Q.samples(buf, segs, prm)[6]
    mc = ok["nal_found"] + 3 if moof_cap is None else moof_cap
    sc = ok["nal_count"] + 3 if sample_cap is None else sample_cap
    if sample_cap is None:
        summary_matches(call(ctx, d_buf, len(buf), prm, moof_cap=mc, **kw), want)
    outs = make_outs(sc, mc)
    summary_matches(call(ctx, d_buf, len(buf), prm, moof_cap=mc, sample_cap=sc, outs=outs, **kw), want)
    for t in outs.values():
        assert (t.cpu().numpy() == CAN).all(), "written in spite of the error"
    return want


def test_errors_at_the_stated_segment_moof_and_sample(ctx):
    from tests.test_mp4_read_ref import good_moof
    prm = Q.read_params(track_id=1)
    g = good_moof()
    rng = np.random.default_rng(95)
    filler, _, _ = moofs_of(rng, prm, [[2]] * (W + 5))                 # the offender lies in the second workgroup, a lower one too
    n_fill = 2 * (W + 5)
    # chain errors: segments 300 and 280 of 400 are broken
    segs = [(0, len(g))] * 400
    buf = g + g[:-1] + struct.pack(">I4s", 7, b"free")
    segs[300] = (len(g), len(g) - 1)
    segs[280] = (2 * len(g) - 1, 8)
    assert untouched(ctx, buf, segs, prm)["reserved"] == [281, 0, 0]
    segs[280] = (8, len(buf))                                          # leaves the buffer
    assert untouched(ctx, buf, segs, prm)["reserved"] == [281, 0, 0]
    # moof errors
    no_tfdt = Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", Q.tfhd(1)))
    bad_trun = Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", Q.tfhd(1) + Q.tfdt(5) + Q.trun(0x200, [(0, 1, 0, 0)], count=2)))
    assert untouched(ctx, filler + bad_trun + g + no_tfdt, None, prm)["reserved"] == [0, W + 6, 0]
    assert untouched(ctx, g + no_tfdt, None, prm)["reserved"] == [0, 2, 0]
    # sample errors: time, presentation time, the buffer's end, a negative data begin
    for bad, at in ((good_moof(time=(1 << 62) - 10), 1), (good_moof(entries=((10, 4, 0, 0), (10, 4, 0, -1021))), 1), (good_moof(short=1), 1),
                    (good_moof(data_offset=-1 - len(filler)), 0), (good_moof(hflags=1, base=(1 << 64) - 1), 0)):
        assert untouched(ctx, filler + bad, None, prm)["reserved"] == [0, 0, n_fill + at + 1]
    bad = good_moof(entries=((10, 4, 0, 0), (10, 4, 0, -1021)))
    assert untouched(ctx, filler + bad + filler + good_moof(time=1 << 62), None, prm)["reserved"] == [0, 0, n_fill + 2]


def test_capacity_plan_only_and_nothing(ctx):
    rng = np.random.default_rng(96)
    prm = Q.read_params(track_id=1, trex_size=2)
    buf, expect, frags = moofs_of(rng, prm, [[3], [0], [4, 2]])
    assert untouched(ctx, buf, None, prm, moof_cap=2) == Q.summary(Q.E_CAPACITY, 0, 3, 0, len(buf))
    assert untouched(ctx, buf, None, prm, moof_cap=0) == Q.summary(Q.E_CAPACITY, 0, 3, 0, len(buf))
    assert untouched(ctx, buf, None, prm, sample_cap=8) == Q.summary(Q.E_CAPACITY, 9, 3, 0, len(buf))
    assert untouched(ctx, buf, None, prm, sample_cap=0) == Q.summary(Q.E_CAPACITY, 9, 3, 0, len(buf))
    # room to spare: the same tables, nothing behind them
    d_buf = dev(np.frombuffer(buf, dtype=np.uint8))
    outs = make_outs(9, 3)
    want = Q.samples(buf, None, prm)
    summary_matches(call(ctx, d_buf, len(buf), prm, moof_cap=700, sample_cap=5000, outs={k: v for k, v in outs.items()}), want[6])
    check_outs(outs, want, 9, 3)
    # n_segs == 0 with a table, and an empty buffer as one segment
    outs = make_outs(1, 1)
    summary_matches(call(ctx, d_buf, len(buf), prm, seg=seg_table([(0, 8)], 16), n_segs=0, moof_cap=1, sample_cap=1, outs=outs),
                    Q.summary(total=len(buf)))
    summary_matches(call(ctx, None, 0, prm, moof_cap=1, sample_cap=1, outs=outs), Q.summary())
    summary_matches(call(ctx, None, 0, prm), Q.summary())
    for t in outs.values():
        assert (t.cpu().numpy() == CAN).all()
    # only the sample tables
    run(ctx, buf, None, prm, which=("sample_off", "sample_size"))
    run(ctx, buf, None, prm, which=("sample_off", "sample_size", "sample_flags", "frag"))


def test_argument_refusals(ctx):
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import SUMMARY
    prm = Q.read_params(track_id=1)
    buf, _, _ = moofs_of(np.random.default_rng(97), prm, [[3]])
    d = dev(np.frombuffer(buf, dtype=np.uint8))
    summary = torch.full((SUMMARY.itemsize + 16,), 0x11, dtype=torch.uint8, device="cuda")
    o = make_outs(3, 1)
    seg = seg_table([(0, len(buf))], 16)
    good = dict(moof_cap=1, sample_cap=3, **o)

    def rc(params=None, data=d, summ=summary[:SUMMARY.itemsize], **kw):
        return ctx.mp4_samples_async(data, len(buf), hbs.mp4_read_params(**prm) if params is None else params, summ, **kw)
    assert rc(**good) == 0
    p = hbs.mp4_read_params(**prm)
    p["flags"] = 1
    assert rc(params=p, **good) == R.E_ARG
    for i in range(3):
        p = hbs.mp4_read_params(**prm)
        p["reserved"][0][i] = 1
        assert rc(params=p, **good) == R.E_ARG
    for stride in (0, 8, 12, 20, 17):
        assert rc(seg=seg, seg_stride=stride, n_segs=1, **good) == R.E_ARG
    assert rc(seg=seg, seg_stride=16, n_segs=1, **good) == 0
    assert rc(moof_cap=1, sample_cap=3, sample_off=o["sample_off"]) == R.E_ARG
    assert rc(moof_cap=1, sample_cap=3, sample_size=o["sample_size"]) == R.E_ARG
    for name in ("dts", "pts", "sample_flags", "frag"):
        assert rc(moof_cap=1, sample_cap=3, **{name: o[name]}) == R.E_ARG
    assert rc(**dict(good, moof_cap=1 << 32)) == R.E_ARG and rc(**dict(good, sample_cap=1 << 32)) == R.E_ARG
    assert rc(moof_cap=1, sample_cap=1 << 32) == 0                     # plan only: sample_cap sizes nothing
    for name, step in (("sample_off", 4), ("sample_size", 4), ("dts", 4), ("pts", 4), ("sample_flags", 2), ("frag", 8)):
        assert rc(**dict(good, **{name: o[name][step:]})) == R.E_ARG
    assert rc(data=d[8:], **good) == R.E_ARG and rc(summ=summary[8:8 + SUMMARY.itemsize], **good) == R.E_ARG
    assert rc(seg=seg[4:], seg_stride=16, n_segs=0, **good) == R.E_ARG
    for t in o.values():
        t.fill_(CAN)
    assert rc(params=hbs.mp4_read_params(**prm), **dict(good, moof_cap=0)) == 0
    assert ctx.mp4_samples_async(d, len(buf), None, summary[:SUMMARY.itemsize], **good) == R.E_ARG
    assert ctx.mp4_samples_async(None, len(buf), hbs.mp4_read_params(**prm), summary[:SUMMARY.itemsize], **good) == R.E_ARG


# ---- a HIP graph ---------------------------------------------------------------------------------------------------------------

def test_one_replay_from_a_graph_on_other_contents(ctx):
    """captured on a side stream after one warm-up call, replayed on other contents of the same buffers: other boxes, other
    counts of moofs and samples; every host argument is the same"""
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import SUMMARY
    prm = Q.read_params(track_id=2, trex_duration=50, trex_size=4, trex_flags=0x01010000)
    members = []
    for seed in (11, 12):
        buf, segs, expect, frags = Q.random_segments(np.random.default_rng(seed), 1, prm, moofs_per_seg=(40, 60), zero_last=False)
        members.append(buf[:segs[0][1]])                   # (the segment begins the buffer; what lies behind it is not boxes)
    size = max(len(b) for b in members) + 16
    members = [b + Q.box(b"free", bytes(size - len(b) - 8)) for b in members]
    wants = [Q.samples(b, None, prm) for b in members]
    assert all(w[6]["error"] == 0 for w in wants) and wants[0][6]["nal_count"] != wants[1][6]["nal_count"]
    n, m = max(w[6]["nal_count"] for w in wants), max(w[6]["nal_found"] for w in wants)
    d = dev(np.frombuffer(members[0], dtype=np.uint8))
    outs = make_outs(n, m)
    summary = torch.full((SUMMARY.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
    rec = hbs.mp4_read_params(**prm)

    def launch():
        return ctx.mp4_samples_async(d, size, rec, summary, moof_cap=m, sample_cap=n, **outs)

    def check(want):
        summary_matches(ctx.read_summary(summary), want[6])
        check_outs(outs, want, want[6]["nal_count"], want[6]["nal_found"])
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
