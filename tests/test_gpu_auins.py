"""hbs_au_insert on the GPU against the plain loop of tests/_auins_ref.py, byte for byte: plan first, then a run into outputs of
exactly the planned capacity with canaries behind every output, every summary field checked; then the ways on from its output
on the device: hbs_index_extract, hbs_ts_mux and hbs_ts_demux, hbs_annexb_to_lenpref."""
import numpy as np
import pytest

from tests import _au_ref as A
from tests import _auins_ref as R
from tests import _ts_ref as D
from tests._auins_ref import build, nal, random_case, tiny_case

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
NAL_BLOCK = 2048                # NALs of a plan workgroup of the NAL side
AU_BLOCK = 256                  # AUs of a plan workgroup of the AU side; the scan takes 2048 workgroups a pass
FIELDS = ("nal_count", "nal_found", "rbsp_bytes", "stream_bytes", "stop_reason", "error")


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
    for k in FIELDS:
        assert int(s[k]) == want[k], (k, s, want)
    assert [int(x) for x in s["reserved"]] == want["reserved"], (s, want)


def put(case):
    stream, index, parsed, compact, au, nal_au = case
    return dict(stream=dev(stream), nbytes=len(stream), index=dev(index), parsed=dev(parsed), n=len(index), au=dev(au), nal_au=dev(nal_au), m=len(au))


def call(ctx, d, first, count, flags, outs=None, out_cap=None, index_cap=0):
    """outs: None (a plan) or the five output tensors (each may be None)"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    out, io, src, nau, auo = outs if outs is not None else (None,) * 5
    rc = ctx.au_insert_async(d["stream"], d["nbytes"], d["index"], d["parsed"], d["n"], d["au"], d["nal_au"], d["m"], first, count, flags,
                             out, io, src, nau, auo, summary, out_cap=out_cap, index_cap=index_cap)
    assert rc == 0, rc
    return ctx.read_summary(summary)


def outputs(need, M, cnt):
    return canary(need), canary(M * 32), canary(M * 4), canary(M * 4), canary(cnt * 64)


def run(ctx, case, first, count, flags, d=None):
    """plan, then a run into outputs of exactly the planned capacity; everything against the plain loop.
    -> (out device tensor, the reference's results, device inputs, device outputs)"""
    stream, index, parsed, compact, au, nal_au = case
    want = R.au_insert(stream, index, parsed, au, nal_au, first, count, flags)
    w_out, w_io, w_src, w_nau, w_au, w_s = want
    assert w_s["error"] == 0
    d = d if d is not None else put(case)
    s = call(ctx, d, first, count, flags)
    summary_matches(s, w_s)
    need, M, cnt = int(s["stream_bytes"]), int(s["nal_count"]), int(s["reserved"][2])
    outs = outputs(need, M, cnt)
    s = call(ctx, d, first, count, flags, outs, out_cap=need, index_cap=M)
    summary_matches(s, w_s)
    o = outs[0].cpu().numpy()
    bad = np.flatnonzero(o[:need] != w_out)
    assert len(bad) == 0, "output differs at byte %d (%d bytes of %d differ)" % (bad[0], len(bad), need)
    assert (o[need:] == CAN).all(), "stored behind the output"
    for name, t, w in (("d_index_out", outs[1], w_io), ("d_nal_src", outs[2], w_src), ("d_nal_au_out", outs[3], w_nau), ("d_au_out", outs[4], w_au)):
        g = t.cpu().numpy()
        size = w.size * w.itemsize
        got = g[:size].view(w.dtype)
        if not np.array_equal(got, w):
            j = int(np.flatnonzero(got != w)[0])
            raise AssertionError("%s differs at entry %d: %s, wanted %s" % (name, j, got[j], w[j]))
        assert (g[size:] == CAN).all(), "stored behind " + name
    return outs[0][:need], want, d, outs


def untouched_on_error(ctx, d, first, count, flags, want_s, need, M, cnt, out_cap, index_cap):
    """the plan reports the counts (an argument error: as the run does), the run reports want_s; the canary-filled outputs stay"""
    summary_matches(call(ctx, d, first, count, flags), dict(want_s, error=want_s["error"] if want_s["error"] == R.E_ARG else 0))
    outs = outputs(need, M, cnt)
    summary_matches(call(ctx, d, first, count, flags, outs, out_cap=out_cap, index_cap=index_cap), want_s)
    for t in outs:
        assert (t.cpu().numpy() == CAN).all(), "written in spite of the error"


COUNTS = (0, 1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049)


def test_au_counts_and_every_flag_combination(ctx):
    """each count with one flag combination and with flags 0, which must be the filter's output for the range"""
    rng = np.random.default_rng(1)
    seen = set()
    for k, n in enumerate(COUNTS):
        case = random_case(rng, n, irap_every=(6, 1, 3)[k % 3], max_slices=3)
        d = put(case)
        flags = (k % 7) + 1
        seen.add(flags)
        run(ctx, case, 0, n, flags, d)
        out, want, _, _ = run(ctx, case, 0, n, 0, d)
        if n:
            fout, fio, fs = ctx.filter_annexb(d["stream"], case[1], keep=np.ones(len(case[1]), dtype=np.uint8))
            assert np.array_equal(fout.cpu().numpy(), out.cpu().numpy()) and np.array_equal(fio, want[1])
            assert int(fs["rbsp_bytes"]) == want[5]["rbsp_bytes"] and int(fs["nal_count"]) == want[5]["nal_count"]
    assert seen == set(range(1, 8))


def test_more_plan_workgroups_than_one_scan_pass(ctx):
    """2048 AU-side plan workgroups and three AUs more (the scan takes 2048 a pass), AUs of one 3-byte NAL: an AUD in front of
    each, the sets in front of every 32nd"""
    n = AU_BLOCK * 2048 + 3
    case = tiny_case(n)
    _, want, _, _ = run(ctx, case, 0, n, R.AUD | R.PARAM_SETS)
    assert want[5]["reserved"] == [n, 3 * ((n - 1) // 32), n] and want[5]["stream_bytes"] < 100_000_000


def test_ranges(ctx):
    rng = np.random.default_rng(2)
    n = 700
    case = random_case(rng, n, irap_every=7)
    d = put(case)
    au = case[4]
    non_irap = next(a for a in range(300, n) if not au["flags"][a] & (A.IRAP | A.PARAM_SETS) and case[2]["nal_unit_type"][au["first_nal"][a]] != 35)
    for first, count, flags in ((0, n, 7), (5, 0, 7), (n, 5, 7), (n + 9, 1 << 40, 3), (0, 1, 7), (n - 1, 1, 7), (n - 1, 1, 1), (n - 40, 1000, 3),
                                (650, 1 << 63, 6), (non_irap, 30, R.PARAM_SETS_FIRST), (non_irap, 30, R.PARAM_SETS), (non_irap, 30, 7),
                                (AU_BLOCK - 1, 2, 7), (AU_BLOCK, AU_BLOCK, 5)):
        _, want, _, _ = run(ctx, case, first, count, flags, d)
        if (first, count, flags) == (non_irap, 30, R.PARAM_SETS_FIRST):
            assert int(want[4]["flags"][0]) & A.PARAM_SETS and int(want[2][0]) < int(au["first_nal"][non_irap])


def far_back_case(rng, kinds=(32, 33, 34)):
    """the sets in NAL block 0; AUs of one slice for several 2048-NAL blocks, among them an SPS with rc < 0 and a PPS of an
    AU of its own kind; then IRAP AUs: a plain one, one with a PPS of its own in front of its picture, one behind an AUD"""
    nals = [nal(t, size=int(rng.integers(5, 90))) for t in kinds] + [nal(19, first=1, stype=2, size=30)]
    for a in range(3 * NAL_BLOCK + 100):
        if a == 2500:
            nals.append(nal(33, rc=-1, size=17))            # must not be taken
        nals.append(nal(1, first=1, stype=a % 3, lsb=a % 200, size=int(rng.integers(3, 20)), sc=3 + a % 2))
    nals += [nal(21, first=1, stype=2, size=40)]
    nals += [nal(34, size=11), nal(39, size=6), nal(21, first=1, stype=2, size=40), nal(21, first=0, stype=2, size=10)]       # brings its own PPS
    nals += [nal(35, size=3), nal(39, size=6), nal(21, first=1, stype=2, size=40)]
    nals += [nal(1, first=1, stype=0, size=9)]
    return build(rng, nals)


def inserted_sets(case, want, a):
    """the source NALs of the sets inserted into AU a (full range)"""
    r = want[4][a]
    src = want[2][int(r["first_nal"]): int(r["first_nal"]) + int(r["nal_count"])]
    return [int(q) for q in src if q != R.NONE and int(q) < int(case[4]["first_nal"][a])]


def test_sets_in_force_far_back(ctx):
    rng = np.random.default_rng(3)
    for kinds in ((32, 33, 34), (33, 34), (32, 34)):
        case = far_back_case(rng, kinds)
        n = len(case[4])
        d = put(case)
        _, want, _, _ = run(ctx, case, 0, n, R.PARAM_SETS | R.AUD, d)
        ins = [inserted_sets(case, want, a) for a in range(n - 4, n)]
        own_pps = [k for k in range(len(case[2])) if case[2]["nal_unit_type"][k] == 34][1]
        others = [k for k, t in enumerate(kinds) if t != 34]
        # a plain IRAP AU: all of block 0's sets; one with a PPS of its own: the others; behind it: that PPS is in force; no IRAP: none
        assert ins == [list(range(len(kinds))), others, others + [own_pps], []], (kinds, ins)
        assert inserted_sets(case, want, 0) == [] and want[5]["reserved"][0] == n - 1
        run(ctx, case, n - 4, 4, R.PARAM_SETS, d)
        run(ctx, case, n - 2, 2, R.PARAM_SETS_FIRST, d)


def test_one_au_of_5000_slices(ctx):
    rng = np.random.default_rng(4)
    nals = [nal(32, size=20), nal(33, size=50), nal(34, size=12), nal(19, first=1, stype=2, size=20)]
    nals += [nal(1, first=1, size=25), nal(39, size=5)]
    nals += [nal(21, first=(k == 0), stype=2, size=int(rng.integers(3, 30))) for k in range(5000)]
    nals += [nal(35, size=3), nal(21, first=1, stype=2, size=30)]
    case = build(rng, nals)
    assert len(case[4]) == 4 and int(case[4]["nal_count"][2]) == 5001
    d = put(case)
    for first, count, flags in ((0, 4, 7), (2, 1, 3), (2, 2, R.PARAM_SETS), (1, 3, 1)):
        run(ctx, case, first, count, flags, d)


def test_a_copied_sps_of_70_kib(ctx):
    """an inserted piece that spans copy tiles, in front of AUs at several offsets"""
    rng = np.random.default_rng(5)
    nals = [nal(32, size=20), nal(33, size=70 * 1024 + 5), nal(34, size=12), nal(19, first=1, stype=2, size=100)]
    for a in range(40):
        nals.append(nal(21 if a % 9 == 0 else 1, first=1, stype=2 if a % 9 == 0 else 1, size=int(rng.integers(50, 9000))))
    case = build(rng, nals)
    _, want, _, _ = run(ctx, case, 0, 41, R.PARAM_SETS | R.AUD)
    assert want[5]["reserved"] == [41, 15, 41] and want[5]["stream_bytes"] > 5 * 70 * 1024
    run(ctx, case, 1, 40, R.PARAM_SETS)


def test_more_pieces_in_a_tile_than_its_lds_table_holds(ctx):
    """AUs of one 3-byte NAL with an AUD in front: 13 bytes and two pieces each, five thousand AUs in a 64 KiB tile"""
    n = 30000
    case = tiny_case(n, irap_every=500)
    _, want, _, _ = run(ctx, case, 0, n, R.AUD)
    assert want[5]["stream_bytes"] == 13 * n + 18
    run(ctx, case, 7, 20000, R.AUD | R.PARAM_SETS)


def test_every_source_offset_modulo_16(ctx):
    """what stands behind an insertion is copied from a source 0..15 bytes off the output's 16-byte grid"""
    rng = np.random.default_rng(6)
    case = random_case(rng, 400, irap_every=5, p_aud=0.1)
    _, want, _, _ = run(ctx, case, 0, 400, 7)
    au, au_out = case[4], want[4]
    shift = (au_out["unit_end"].astype(np.int64) - au["unit_end"].astype(np.int64)) % 16
    assert sorted(set(shift.tolist())) == list(range(16))
    _, want, _, _ = run(ctx, case, 3, 300, 3)
    shift = (want[4]["unit_end"].astype(np.int64) - au["unit_end"][3:303].astype(np.int64)) % 16
    assert sorted(set(shift.tolist())) == list(range(16))


@pytest.mark.parametrize("at", (0, 255, 256, 2100))
def test_inconsistent_tables(ctx, at):
    rng = np.random.default_rng(70 + at)
    n = 2300
    case = random_case(rng, n, max_slices=2)
    stream, index, parsed, compact, au, nal_au = case
    clean = R.au_insert(stream, index, parsed, au, nal_au, 0, n, 7)[5]
    done = 0
    for what in ("start > end", "end > stream_bytes", "start < the end in front", "first_nal", "nal_count", "unit_begin", "unit_end",
                 "first_vcl", "the last AU ends early", "d_nal_au names another AU", "d_nal_au past the table"):
        i2, a2, n2 = index.copy(), au.copy(), nal_au.copy()
        k = int(au["first_nal"][at])
        if what == "start > end":
            i2["start"][k] = i2["end"][k] + 1
        elif what == "end > stream_bytes":
            i2["end"][-1] = len(stream) + 1
            a2["unit_end"][-1] = len(stream) + 1
        elif what == "start < the end in front":
            if k == 0:
                continue
            i2["start"][k] = i2["end"][k - 1] - 1
        elif what == "first_nal":
            a2["first_nal"][at] += 1
        elif what == "nal_count":
            a2["nal_count"][at] += 1
        elif what == "unit_begin":
            a2["unit_begin"][at] += 1
        elif what == "unit_end":
            a2["unit_end"][at] -= 1
        elif what == "first_vcl":
            a2["first_vcl"][at] = a2["nal_count"][at]
        elif what == "the last AU ends early":
            a2["nal_count"][-1] -= 1
            if a2["nal_count"][-1] == 0:
                continue
            a2["unit_end"][-1] = i2["end"][-2]
        elif what == "d_nal_au names another AU":
            n2[k] = at + 1
        else:
            n2[k] = n
        want = R.au_insert(stream, i2, parsed, a2, n2, 0, n, 7)[5]
        assert want["error"] == R.E_ARG and want["nal_count"] == 0, what
        untouched_on_error(ctx, put((stream, i2, parsed, compact, a2, n2)), 0, n, 7, want, clean["stream_bytes"], clean["nal_count"], n,
                           clean["stream_bytes"], clean["nal_count"])
        done += 1
    assert done >= 9


def test_capacity_one_short(ctx):
    rng = np.random.default_rng(8)
    n = 600
    case = random_case(rng, n)
    stream, index, parsed, compact, au, nal_au = case
    d = put(case)
    for first, count, flags in ((0, n, 7), (100, 300, 1)):
        want = R.au_insert(stream, index, parsed, au, nal_au, first, count, flags)[5]
        need, M, cnt = want["stream_bytes"], want["nal_count"], want["reserved"][2]
        short = dict(want, error=R.E_CAPACITY)
        untouched_on_error(ctx, d, first, count, flags, short, need, M, cnt, need - 1, M)
        untouched_on_error(ctx, d, first, count, flags, short, need, M, cnt, need, M - 1)
        untouched_on_error(ctx, d, first, count, flags, short, need, M, cnt, 0, 0)
        # index_cap counts only with a per-NAL table
        out, auo = canary(need), canary(cnt * 64)
        s = call(ctx, d, first, count, flags, (out, None, None, None, auo), out_cap=need, index_cap=0)
        summary_matches(s, want)
        assert np.array_equal(out.cpu().numpy()[:need], R.au_insert(stream, index, parsed, au, nal_au, first, count, flags)[0])
        # one table alone
        src = canary(M * 4)
        summary_matches(call(ctx, d, first, count, flags, (out, None, src, None, None), out_cap=need, index_cap=M - 1), short)
        assert (src.cpu().numpy() == CAN).all()


def test_argument_refusals(ctx):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(9)
    case = random_case(rng, 40)
    stream, index, parsed, compact, au, nal_au = case
    want = R.au_insert(stream, index, parsed, au, nal_au, 0, 40, 7)
    need, M = want[5]["stream_bytes"], want[5]["nal_count"]
    z = torch.zeros(64, dtype=torch.uint8, device="cuda")
    big = torch.cat([z, dev(stream), z])
    t = dict(stream=big[64:64 + len(stream)], index=torch.cat([dev(index), z]), parsed=torch.cat([dev(parsed), z]), au=torch.cat([dev(au), z]),
             nal_au=torch.cat([dev(nal_au), z]), out=canary(need + 64), io=canary(M * 32 + 64), src=canary(M * 4 + 64), nau=canary(M * 4 + 64),
             auo=canary(40 * 64 + 64), s=torch.full((SUMMARY.itemsize + 16,), 0x5A, dtype=torch.uint8, device="cuda"))

    def go(n=len(index), m=40, flags=7, out_cap=need, **change):
        a = dict(t, **change)
        return ctx.au_insert_async(a["stream"], len(stream), a["index"], a["parsed"], n, a["au"], a["nal_au"], m, 0, 40, flags,
                                   a["out"], a["io"], a["src"], a["nau"], a["auo"], a["s"][:SUMMARY.itemsize], out_cap=out_cap, index_cap=M)
    changes = [dict(stream=big[72:72 + len(stream)]), dict(index=t["index"][8:]), dict(parsed=t["parsed"][8:]), dict(au=t["au"][8:]), dict(nal_au=t["nal_au"][2:]),
               dict(out=t["out"][8:]), dict(io=t["io"][4:]), dict(src=t["src"][2:]), dict(nau=t["nau"][1:]), dict(auo=t["auo"][8:]), dict(s=t["s"][8:]),
               dict(index=None), dict(parsed=None), dict(au=None), dict(nal_au=None)]
    for change in changes:
        assert go(**change) == R.E_ARG, change
    assert go(flags=8) == R.E_ARG and go(flags=1 << 31) == R.E_ARG
    assert go(n=1 << 32) == R.E_ARG and go(m=1 << 32) == R.E_ARG and go(out_cap=(1 << 46) + 1) == R.E_ARG
    assert ctx.lib.hbs_au_insert(ctx.h, t["stream"].data_ptr(), len(stream), t["index"].data_ptr(), t["parsed"].data_ptr(), len(index), t["au"].data_ptr(),
                                 t["nal_au"].data_ptr(), 40, 0, 40, 7, None, 0, None, None, None, 0, None, None) == R.E_ARG
    torch.cuda.synchronize()
    for k in ("out", "io", "src", "nau", "auo"):
        assert (t[k].cpu().numpy() == CAN).all(), k
    assert (t["s"].cpu().numpy() == 0x5A).all()
    assert go() == 0
    summary_matches(ctx.read_summary(t["s"][:SUMMARY.itemsize]), want[5])
    assert np.array_equal(t["out"].cpu().numpy()[:need], want[0])


def test_no_nals_or_no_aus(ctx):
    rng = np.random.default_rng(10)
    case = random_case(rng, 5)
    stream, index, parsed, compact, au, nal_au = case
    for c2 in ((stream, index[:0], parsed[:0], compact[:0], au, nal_au[:0]), (stream, index, parsed, compact, au[:0], nal_au)):
        want = R.au_insert(c2[0], c2[1], c2[2], c2[4], c2[5], 0, 5, 7)[5]
        assert want["error"] == 0 and want["nal_count"] == 0 and want["nal_found"] == len(c2[1])
        d = put(c2)
        summary_matches(call(ctx, d, 0, 5, 7), want)
        outs = outputs(64, 4, 4)
        summary_matches(call(ctx, d, 0, 5, 7, outs, out_cap=64, index_cap=4), want)
        for t in outs:
            assert (t.cpu().numpy() == CAN).all()


def test_the_scan_of_the_output_is_its_index(ctx):
    """hbs_index_extract of the output equals d_index_out (cases without leading bytes and without a short last NAL)"""
    rng = np.random.default_rng(11)
    done = 0
    for it in range(6):
        n = (40, 300, 2100)[it % 3]
        case = random_case(rng, n, lead_junk=0, irap_every=4)
        out, want, _, _ = run(ctx, case, 0 if it < 3 else 7, n, 7 - it)
        exc, junk, short = R.rescan_exceptions(case[0], case[1], case[4], 0 if it < 3 else 7, n, want[0], want[1], want[2])
        if exc is not None:
            continue
        got, _, s = ctx.index_extract(out)
        assert np.array_equal(got, want[1]) and int(s["rbsp_bytes"]) == want[5]["rbsp_bytes"]
        done += 1
    assert done >= 4


def test_through_the_transport_stream_and_back(ctx):
    """hbs_ts_mux fed d_au_out, then hbs_ts_demux: the output's bytes, random access on the IRAP AUs; every PES begins with an AUD"""
    rng = np.random.default_rng(12)
    n = 500
    case = random_case(rng, n, irap_every=10, last_without_picture=True)
    out, want, _, outs = run(ctx, case, 20, 400, R.AUD | R.PARAM_SETS)
    au_out = want[4]
    pts = (np.arange(400, dtype=np.uint64) * np.uint64(3003)) + np.uint64(90000)
    ts, ap, s = ctx.ts_mux(out, outs[4][: 400 * 64], pts, None, flags=2)
    es, pes, ds = ctx.ts_demux(ts, 0x100, 188)
    assert np.array_equal(es.cpu().numpy(), want[0]) and int(ds["error"]) == 0 and len(pes) == 400
    assert np.array_equal(pes["out_off"], au_out["unit_begin"]) and np.array_equal(pes["pts"], pts)
    irap = (au_out["flags"] & A.IRAP) != 0
    assert irap.sum() >= 30 and np.array_equal((pes["flags"] & D.F_RAI) != 0, irap)
    o = want[0]
    for a in range(400):
        k = int(au_out["first_nal"][a])
        assert o[int(want[1]["start"][k])] >> 1 == 35, a


def test_one_sample_per_au_that_begins_with_the_aud(ctx):
    """hbs_annexb_to_lenpref with d_index_out and d_nal_au_out"""
    rng = np.random.default_rng(13)
    n = 300
    case = random_case(rng, n, irap_every=8)
    out, want, _, outs = run(ctx, case, 0, n, 7)
    M = want[5]["nal_count"]
    lp, lio, so, s = ctx.annexb_to_lenpref(out, outs[1][: M * 32], nal_au=outs[3][: M * 4], n_aus=n)
    assert int(s["error"]) == 0 and len(so) == n + 1 and int(so[-1]) == len(lp)
    b = lp.cpu().numpy()
    for a in range(n):
        at = int(so[a])
        size = int.from_bytes(b[at:at + 4].tobytes(), "big")
        assert size == 3 and b[at + 4] == 0x46, a                  # the first record of the sample: an AUD
    assert int(s["nal_count"]) == M


def test_the_convenience_call(ctx):
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(14)
    case = random_case(rng, 90)
    stream, index, parsed, compact, au, nal_au = case
    want = R.au_insert(stream, index, parsed, au, nal_au, 10, 50, 3)
    out, io, src, nau, auo, s = ctx.au_insert(dev(stream), index, parsed, len(index), au, nal_au, 10, 50, hbs.AUINS_AUD | hbs.AUINS_PARAM_SETS)
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(io.cpu().numpy().view(hbs.NAL_ENTRY), want[1])
    assert np.array_equal(src.cpu().numpy().view(np.uint32), want[2]) and np.array_equal(nau.cpu().numpy().view(np.uint32), want[3])
    assert np.array_equal(auo.cpu().numpy().view(hbs.ACCESS_UNIT), want[4])
    summary_matches(s, want[5])


def test_carved_buffers_at_each_accepted_alignment(ctx):
    """every pointer of the call inside a larger allocation, at each offset from a page boundary its alignment accepts; the bytes
    around every buffer are looked at afterwards, hostile start codes around the stream"""
    from tests import _carve as K
    rng = np.random.default_rng(15)
    n = 120
    hostile = b"\x00\x00\x01\x46\x01\x50\x00\x00\x01\x42\x01\x01" * 4
    for k in range(len(K.OFFS4)):
        stream, index, parsed, compact, au, nal_au = random_case(rng, n, irap_every=5)
        flags = k % 7 + 1
        want = R.au_insert(stream, index, parsed, au, nal_au, 3, 100, flags)
        need, M, cnt = want[5]["stream_bytes"], want[5]["nal_count"], want[5]["reserved"][2]
        o16 = lambda j: K.OFFS16[(k + j) % len(K.OFFS16)]          # noqa: E731
        o4 = lambda j: K.OFFS4[(k + j) % len(K.OFFS4)]             # noqa: E731
        cs = K.Carved(len(stream), o16(0), hostile, K.PAD, True).put(stream).hostile(front=hostile, back=hostile)
        ci = K.Carved(len(index) * 32, o16(1), 0xFF, K.PAD, True).put(index)
        cp = K.Carved(len(parsed) * 32, o16(2), 0xFF, K.PAD, True).put(parsed)
        ca = K.Carved(n * 64, o16(3), 0xFF, K.PAD, True).put(au)
        cn = K.Carved(len(nal_au) * 4, o4(0), 0xFF, K.PAD, True).put(nal_au)
        co = K.Carved(need, o16(4), CAN, K.PAD, True)
        cio = K.Carved(M * 32, K.OFFS8[(k + 5) % len(K.OFFS8)], CAN, K.PAD, True)
        csrc = K.Carved(M * 4, o4(3), CAN, K.PAD, True)
        cnau = K.Carved(M * 4, o4(7), CAN, K.PAD, True)
        cau = K.Carved(cnt * 64, o16(5), CAN, K.PAD, True)
        cm = K.Carved(64, o16(6), 0xEE, K.PAD, True)
        rc = ctx.au_insert_async(cs.view, len(stream), ci.view, cp.view, len(index), ca.view, cn.view, n, 3, 100, flags,
                                 co.view, cio.view, csrc.view, cnau.view, cau.view, cm.view, out_cap=need, index_cap=M)
        assert rc == 0, k
        summary_matches(ctx.read_summary(cm.view), want[5])
        assert np.array_equal(co.get(), want[0]), k
        assert np.array_equal(cio.get().view(want[1].dtype), want[1]) and np.array_equal(csrc.get().view(np.uint32), want[2]), k
        assert np.array_equal(cnau.get().view(np.uint32), want[3]) and np.array_equal(cau.get().view(want[4].dtype), want[4]), k
        for name, c in (("stream", cs), ("index", ci), ("parsed", cp), ("au", ca), ("nal_au", cn), ("out", co), ("index_out", cio),
                        ("nal_src", csrc), ("nal_au_out", cnau), ("au_out", cau), ("summary", cm)):
            assert c.intact(), (k, name, c.damage())
