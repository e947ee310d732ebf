"""The context's device scratch (hbs_capi.hip: one grow-only buffer per kind, carved by the layout functions next to each
call's arguments): what a context holds after one call of each kind, to the byte; a context whose buffers all grow under it
answers as a fresh one does; every timed call takes its slot of the timing ring.  The five framing and transport calls
(tests/test_gpu_sequences.py holds them against their reference loops) are in the last two, and their scratch is held by relations
between readings; so is that of the RTP and MP4 calls (tests/test_gpu_sequences_rtp_mp4.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import _auins_ref as INS
from tests import _seq_cases as S
from tests import _tsmux_ref as TSM
from tests.test_gpu_au import fabricate
from tests.test_gpu_carved import emit_arena, emit_index, stream_of
from tests.test_gpu_sequences import step

pytestmark = pytest.mark.gpu

# hbs_ctx_device_bytes() of a fresh context after the one call (or the few calls of the convenience wrapper) of SCRATCH_CASES,
# measured with this module's own cases on the library of commit 9853dbe, the last one whose hbs_capi.hip sized and carved every
# workspace by hand.  Exact: the sizes are arithmetic on the call's arguments (none of them depends on the device's compute
# units: the look-back words, the padded tail tile and every workspace are sized by bytes, NALs and tiles alone).
# hbs_annexb_to_lenpref, hbs_lenpref_to_annexb, hbs_ts_demux, hbs_ts_mux and hbs_au_insert came after that commit: there is no
# independent source for what they hold, and a number read off the code under test pins nothing.  They have no entry here;
# test_scratch_relations_of_the_framing_calls holds relations between readings instead.
SCRATCH_BYTES = {
    "scan of 400 KiB into an arena, dense tiles counted ahead": 197876,
    "scan of 70 KiB without an arena": 479104,
    "emit of 8 NALs": 208720,
    "emit of 5000 NALs": 332368,
    "synth_rbsp of 100 NALs": 208208,
    "parse of 300 NALs": 30627408,
    "compact parse of 300 NALs": 63657552,
    "write_headers of 300 NALs": 574800,
    "index_parse of 200 NALs": 38991504,
    "filter of 300 NALs": 203344,
    "access_units and au_keep of 300 NALs": 203600,
}


def new_ctx():
    import hevcbitstream_amd as hbs
    return hbs.Context(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def make_video():
    """a synthetic elementary stream of 2400 NALs and more (slices of 700 to 900 bytes) and the index of its NALs"""
    from tests.hevc_synth import stream_4k30
    raw, count = stream_4k30(21, n_pictures=620, slices_per_picture=4, idr_every=20, payload_bytes=(700, 900))
    assert count >= 2400
    s = np.frombuffer(raw, dtype=np.uint8).copy()
    ctx = new_ctx()
    try:
        idx, _, sm = ctx.index_extract(dev(s))
    finally:
        ctx.close()
    assert int(sm["error"]) == 0 and len(idx) == count
    return s, idx


@pytest.fixture(scope="module")
def video():
    return make_video()


def first_nals(video, n):
    """the stream cut behind its n-th NAL"""
    s, idx = video
    return s[: int(idx["end"][n - 1])]


def scanned(ctx, s, arena=True):
    """hbs_index_extract on ordinary buffers -> (index tensor, entries, rbsp tensor, rbsp bytes, NALs)"""
    import hevcbitstream_amd as hbs
    index, rbsp, summary, cap = ctx.alloc_outputs(len(s), want_rbsp=arena)
    ctx.index_extract_async(dev(s), index, cap, rbsp, summary)
    sm = ctx.read_summary(summary)
    assert int(sm["error"]) == 0, sm
    n = int(sm["nal_count"])
    return index, index[: n * 32].cpu().numpy().view(hbs.NAL_ENTRY).copy(), rbsp, int(sm["rbsp_bytes"]), n


def au_records(ctx, n, seed):
    return fabricate(np.random.default_rng(seed), n, 0.6, 0.3, off=int(ctx.lib.hbs_au_sps_poc_offset()))


# ---- scratch held is what it was ----------------------------------------------------------------------------------------------

def case_scan_arena(video):
    ctx = new_ctx()
    ctx.set_count_ahead(2)
    scanned(ctx, stream_of(np.random.default_rng(7001), 1, 400 << 10, 0))
    return ctx


def case_scan_index_only(video):
    ctx = new_ctx()
    scanned(ctx, stream_of(np.random.default_rng(7002), 1, 70 << 10, 0), arena=False)
    return ctx


def emit_case(lens, seed):
    rng = np.random.default_rng(seed)
    arena, lens = emit_arena(rng, lens)
    ctx = new_ctx()
    ctx.emit_annexb(dev(arena), emit_index(lens, rng.integers(3, 9, size=len(lens))))
    return ctx


def case_emit_small(video):
    return emit_case(np.array([40, 0, 7, 120, 33, 64, 1, 250]), 7003)


def case_emit_5000(video):
    return emit_case(np.random.default_rng(7004).integers(50, 151, size=5000), 7005)


def case_synth(video):
    import torch
    ctx = new_ctx()
    cap = int(ctx.lib.hbs_synth_rbsp_bound(100))
    rbsp = torch.empty(cap, dtype=torch.uint8, device="cuda")
    index = torch.empty(100 * 32, dtype=torch.uint8, device="cuda")
    summary = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ctx._bind_stream()
    ctx._check(ctx.lib.hbs_synth_rbsp(ctx.h, 11, 100, 0, C.c_void_p(rbsp.data_ptr()), cap, C.c_void_p(index.data_ptr()),
                                      C.c_void_p(summary.data_ptr())), "hbs_synth_rbsp")
    assert int(ctx.read_summary(summary)["error"]) == 0
    return ctx


def parse_inputs(video, n=300):
    """index and arena of the first n NALs, made by a context of their own"""
    other = new_ctx()
    try:
        index, _, rbsp, _, found = scanned(other, first_nals(video, n))
    finally:
        other.close()
    assert found == n
    return index, rbsp


def case_parse(video):
    index, rbsp = parse_inputs(video)
    ctx = new_ctx()
    ctx.parse_headers(rbsp, index, 300)
    return ctx


def case_parse_compact(video):
    index, rbsp = parse_inputs(video)
    ctx = new_ctx()
    ctx.parse_headers_compact(rbsp, index, 300)
    return ctx


def case_write_headers(video):
    index, rbsp = parse_inputs(video)
    other = new_ctx()
    try:
        parsed, structs = other.parse_headers(rbsp, index, 300)
    finally:
        other.close()
    ctx = new_ctx()
    ctx.write_headers(parsed, structs, 300, 2048)
    return ctx


def case_index_parse(video):
    import torch
    s = first_nals(video, 200)
    ctx = new_ctx()
    index = torch.empty(256 * 32, dtype=torch.uint8, device="cuda")
    parsed = torch.empty(256 * 32, dtype=torch.uint8, device="cuda")
    s1, s2 = torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert ctx.index_parse_async(dev(s), index, 256, parsed, None, s1, s2) == 200           # (the plan: no struct arena)
    assert int(ctx.read_summary(s2)["error"]) == 0
    return ctx


def case_filter(video):
    s = first_nals(video, 300)
    ctx = new_ctx()
    ctx.filter_annexb(dev(s), video[1][:300], max_temporal_id_plus1=1)
    return ctx


def case_access_units(video):
    ctx = new_ctx()
    index, parsed, compact, structs = au_records(ctx, 300, 7006)
    au, nal_au, _, _ = ctx.access_units(index, parsed, compact, dev(structs), 300)
    ctx.au_keep(dev(nal_au), dev(parsed), 300, len(au) // 3, max(len(au) // 3, 1), param_sets=True)
    return ctx


SCRATCH_CASES = {
    "scan of 400 KiB into an arena, dense tiles counted ahead": case_scan_arena,
    "scan of 70 KiB without an arena": case_scan_index_only,
    "emit of 8 NALs": case_emit_small,
    "emit of 5000 NALs": case_emit_5000,
    "synth_rbsp of 100 NALs": case_synth,
    "parse of 300 NALs": case_parse,
    "compact parse of 300 NALs": case_parse_compact,
    "write_headers of 300 NALs": case_write_headers,
    "index_parse of 200 NALs": case_index_parse,
    "filter of 300 NALs": case_filter,
    "access_units and au_keep of 300 NALs": case_access_units,
}


@pytest.mark.parametrize("name", list(SCRATCH_CASES))
def test_scratch_held_is_what_it_was(video, name):
    ctx = SCRATCH_CASES[name](video)
    try:
        got = ctx.device_bytes()
    finally:
        ctx.close()
    print("device_bytes after", name, got)
    assert got == SCRATCH_BYTES[name], (name, got, SCRATCH_BYTES[name])


# ---- growing under a live context ---------------------------------------------------------------------------------------------

def every_call(ctx, video, n):
    """scan, emit, parse, filter and access units on the first n NALs -> {what: bytes}"""
    out = {}
    s = first_nals(video, n)
    index, entries, rbsp, rbsp_bytes, found = scanned(ctx, s)
    assert found == n
    out["index"], out["arena"] = entries.view(np.uint8).copy(), rbsp[:rbsp_bytes].cpu().numpy()
    back, entries_out = ctx.emit_annexb(rbsp[:rbsp_bytes], entries)
    out["emitted"], out["emitted index"] = back.copy(), entries_out.view(np.uint8).copy()
    parsed, structs = ctx.parse_headers(rbsp, index, n, poison=0xA5)
    out["parsed"], out["structs"] = parsed.view(np.uint8).copy(), structs.cpu().numpy()
    kept, kept_entries, sm = ctx.filter_annexb(dev(s), entries, keep_types=~(1 << 34))             # (without the PPSs)
    out["filtered"], out["filtered index"], out["filter summary"] = kept.cpu().numpy(), kept_entries.view(np.uint8).copy(), sm.tobytes()
    au_index, au_parsed, compact, au_structs = au_records(ctx, n, 7100 + n)
    au, nal_au, sm, carry = ctx.access_units(au_index, au_parsed, compact, dev(au_structs), n)
    out["aus"], out["nal_au"], out["au summary"], out["carry"] = au.view(np.uint8).copy(), nal_au.copy(), sm.tobytes(), carry.tobytes()
    return out


def framing_calls(ctx, video, n):
    """the five framing and transport calls, each planned and run by its convenience wrapper: the first n NALs as records with
    a sample table and back, n random AUs as transport packets and back, AUDs and parameter sets in front of n // 2 AUs
    -> {what: bytes}"""
    out = {}
    s, entries = first_nals(video, n), video[1][:n]
    nal_au = (np.arange(n) // 3).astype(np.uint32)
    rec, rec_entries, so, sm = ctx.annexb_to_lenpref(dev(s), entries, keep=(np.arange(n) % 5 != 0).astype(np.uint8), nal_au=nal_au, n_aus=int(nal_au[-1]) + 1)
    out["records"], out["records index"], out["samples"], out["records summary"] = rec.cpu().numpy(), rec_entries.view(np.uint8).copy(), so, sm.tobytes()
    back, so2, sm = ctx.lenpref_to_annexb(rec, so[:-1].copy(), np.diff(so.astype(np.int64)).astype(np.uint64), startcode_bytes=3)
    out["records back"], out["samples back"], out["back summary"] = back.cpu().numpy(), so2, sm.tobytes()
    stream, au, pts, dts = TSM.random_case(np.random.default_rng(7300 + n), n, TSM.params(), max_es=300)
    ts, au_packet, sm = ctx.ts_mux(dev(stream), au, pts, dts, packet_bytes=192, flags=TSM.PCR | TSM.PSI_AT_IRAP)
    out["packets"], out["au_packet"], out["mux summary"] = ts.cpu().numpy(), au_packet, sm.tobytes()
    es, pes, sm = ctx.ts_demux(ts, 0x100, 192)
    out["demuxed"], out["pes"], out["demux summary"] = es.cpu().numpy(), pes.view(np.uint8).copy(), sm.tobytes()
    stream, index, parsed, _, au, nal_au = INS.random_case(np.random.default_rng(7400 + n), n // 2)
    res = ctx.au_insert(dev(stream), index, parsed, len(index), au, nal_au, flags=INS.AUD | INS.PARAM_SETS | INS.PARAM_SETS_FIRST)
    for what, t in zip(("inserted", "inserted index", "nal_src", "nal_au_out", "au_out"), res[:5]):
        out[what] = t.cpu().numpy().view(np.uint8).copy()
    out["insert summary"] = res[5].tobytes()
    return out


def all_calls(ctx, video, n):
    out = every_call(ctx, video, n)
    out.update(framing_calls(ctx, video, n))
    return out


def test_buffers_grow_under_a_live_context(video):
    small, large = 300, 2400
    want = {}
    for n in (small, large):
        fresh = new_ctx()
        fresh.set_count_ahead(2)
        try:
            want[n] = all_calls(fresh, video, n)
        finally:
            fresh.close()
    assert np.array_equal(want[small]["emitted"], first_nals(video, small)), "the way back gives the stream"
    ctx = new_ctx()
    ctx.set_count_ahead(2)
    try:
        held = []
        for run, n in enumerate((small, large, small)):
            got = all_calls(ctx, video, n)
            held.append(ctx.device_bytes())
            print("run", run, "NALs", n, "device_bytes", held[-1])
            assert got.keys() == want[n].keys()
            for what, w in want[n].items():
                g = got[what]
                assert (np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w), ("run", run, "NALs", n, what, "differs from a fresh context's")
    finally:
        ctx.close()
    assert held[1] > held[0], held
    assert held[2] >= held[1], held


@pytest.mark.parametrize("call", S.CALLS)
def test_scratch_relations_of_the_framing_calls(call):
    """device_bytes() after the five newer calls, as relations between readings (see SCRATCH_BYTES): a plan in front of a run
    adds nothing to what the run alone holds; a small call, or the same call again, leaves it as it is; a context that only
    ever sees the small case holds strictly less.  Every call is held against the reference loop on the way."""
    scratch_relations(call)


@pytest.mark.parametrize("call", S.CALLS2)
def test_scratch_relations_of_the_rtp_and_mp4_calls(call):
    """the same relations for the calls whose layout functions take capacities of the caller as well (lay_rtp, lay_rtpu, lay_rtpo,
    lay_mp4, lay_mp4rd, lay_mp4stbl, lay_mp4stblw): they follow from those functions, each of which carves at least as much
    for a run as for a plan of the same case, and strictly more for the large case's counts and capacities than for the small
    one's"""
    scratch_relations(call)


def scratch_relations(call):
    small, large = S.case(call, "small"), S.case(call, "large")
    planned, alone, little = new_ctx(), new_ctx(), new_ctx()
    try:
        step(planned, large, plan=True)
        after_plan = planned.device_bytes()
        step(planned, large)
        held = planned.device_bytes()
        step(alone, large)
        print("device_bytes of", call, ": plan", after_plan, "plan and run", held, "run alone", alone.device_bytes())
        assert after_plan <= held == alone.device_bytes()
        step(planned, small)
        assert planned.device_bytes() == held, "a small call behind a large one"
        step(planned, large)
        step(planned, large)
        assert planned.device_bytes() == held, "the same call again"
        step(little, small)
        step(little, small)
        print("device_bytes of", call, ": the small case alone", little.device_bytes())
        assert 0 < little.device_bytes() < held
    finally:
        for c in (planned, alone, little):
            c.close()


# ---- timing slots -------------------------------------------------------------------------------------------------------------

def test_every_timed_call_takes_a_slot(video):
    import torch
    s = first_nals(video, 300)
    ctx = new_ctx()
    try:
        index, entries, rbsp, _, n = scanned(ctx, s)
        records = [dev(r) for r in au_records(ctx, n, 7200)]
        summary = torch.zeros(64, dtype=torch.uint8, device="cuda")
        ctx.enable_timing(True)
        d = dev(s)
        ctx.index_extract_async(d, index, n + 1, rbsp, summary)
        ctx.filter_annexb_async(d, len(s), index, n, None, None, summary, rule=ctx.nal_filter())
        assert ctx.access_units_async(records[0], records[1], records[2], records[3], n, None, 0, None, None, summary) == 0
        ms = [ctx.kernel_ms_back(back) for back in range(3)]
        print("access units, filter, scan: ms", ms)
        assert all(m > 0 for m in ms), ms
        assert ctx.kernel_ms() == ms[0]
        with pytest.raises(Exception):
            ctx.kernel_ms_back(3)
        # a scan of no bytes launches nothing and takes no slot: the last timed call is still the one reported
        ctx.index_extract_async(torch.empty(0, dtype=torch.uint8, device="cuda"), index, n + 1, rbsp, summary)
        assert ctx.kernel_ms() == ms[0] and ctx.kernel_ms_back(0) == ms[0]
        with pytest.raises(Exception):
            ctx.kernel_ms_back(3)
        # the five framing and transport calls, the RTP and MP4 calls and hbs_au_times take a slot each time, a plan and a call
        # without input included: their launchers record both events around whatever they launch, be it the one-workgroup scan
        # kernel alone (hbs_capi.hip takes the slot in one place for all of them)
        history = list(ms)                                   # the last call first

        def timed(what, call_it):
            call_it()
            now = ctx.kernel_ms()
            assert now >= 0 and ctx.kernel_ms_back(0) == now, (what, now)
            for back, m in enumerate(history):               # the earlier calls' values, one slot further back each
                assert ctx.kernel_ms_back(back + 1) == m, (what, back)
            with pytest.raises(Exception):
                ctx.kernel_ms_back(len(history) + 1)
            history.insert(0, now)
            return now
        calls = S.CALLS + S.CALLS2
        for call in calls:
            assert timed(call, lambda: step(ctx, S.case(call, "small"))) > 0, call
        for call in calls:
            timed((call, "plan"), lambda: step(ctx, S.case(call, "small"), plan=True))
            timed((call, "empty"), lambda: step(ctx, S.empty(call)))
        # hbs_au_times: one small call on the AU table hbs_access_units makes of the fabricated records (its plan and its run
        # take a slot each), then a plan (no output) and a call of no AUs
        import hevcbitstream_amd as hbs

        def enqueued(rc):
            assert rc == 0
            sm = ctx.read_summary(summary)
            assert int(sm["error"]) == 0, sm
            return sm
        found = []
        timed(("access units", "plan"), lambda: found.append(enqueued(ctx.access_units_async(*records, n, None, 0, None, None, summary))))
        n_aus = int(found[0]["nal_count"])
        assert n_aus > 1
        au = torch.empty(n_aus * hbs.ACCESS_UNIT.itemsize, dtype=torch.uint8, device="cuda")
        assert timed("access units", lambda: enqueued(ctx.access_units_async(*records, n, au, n_aus, None, None, summary))) > 0
        prm = hbs.au_times_params()
        dts, pts = (torch.empty(n_aus, dtype=torch.int64, device="cuda") for _ in range(2))
        for what, args in (("small", (n_aus, prm, summary, dts, pts)), ("plan", (n_aus, prm, summary)), ("empty", (0, prm, summary, dts, pts))):
            ms = timed(("au_times", what), lambda: enqueued(ctx.au_times_async(au, *args)))
            assert ms > 0 or what != "small"
        print("device calls: ms", history[:-3])
    finally:
        ctx.close()
