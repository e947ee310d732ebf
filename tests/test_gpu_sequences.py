"""The five framing and transport calls back to back on one live context.  Each keeps its device scratch in a grow-only buffer
of the context that nothing clears between calls (hbs_capi.hip: carve, grow), so a scratch word a kernel reads without having
written it is the previous call's, in that call's layout.  Here calls of different sizes, layouts and outcomes follow each other
on one context, and every one of them is held, byte for byte and field for field, against the plain loops of tests/_*_ref.py:
never against a fresh context, which could be wrong in the same way.  The cases are tests/_seq_cases.py's; tests/test_seq_cases.py
holds on the CPU that they are what the sequences need.  alloc, launch, verify and step also serve the RTP and MP4 calls, whose
sequences are in tests/test_gpu_sequences_rtp_mp4.py, and hbs_au_times, hbs_cenc_subsamples, hbs_cenc_crypt and hbs_cbcs_crypt, whose
sequences are in tests/test_gpu_sequences_times_crypt.py."""
import numpy as np
import pytest

from tests import _au_times_ref as T
from tests import _mp4_ref as MF
from tests import _rtp_order_ref as RO
from tests import _rtp_ref as R
from tests import _rtp_unpack_ref as RU
from tests import _seq_cases as S
from tests import _tsmux_ref as TSM
from tests import test_gpu_au_times as TA
from tests import test_gpu_auins as AI
from tests import test_gpu_cbcs as TY
from tests import test_gpu_cenc as TC
from tests import test_gpu_lenpref as LP
from tests import test_gpu_mp4 as TF
from tests import test_gpu_mp4_read as TQ
from tests import test_gpu_mp4_stbl as TB
from tests import test_gpu_mp4_stbl_write as TW
from tests import test_gpu_rtp as TR
from tests import test_gpu_rtp_order as TO
from tests import test_gpu_rtp_unpack as TU
from tests import test_gpu_ts as TS
from tests import test_gpu_tsmux as TM

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
PACKET_SIZES = (188, 192, 204)
# what a run writes: (buffer, its place in the reference's result)
OUTPUTS = dict(a2l=(("out", 0), ("io", 1), ("so", 2)), l2a=(("out", 0), ("so", 1)), tsd=(("out", 0), ("pes", 1)), tsm=(("out", 0), ("ap", 1)),
               ins=(("out", 0), ("io", 1), ("src", 2), ("nau", 3), ("auo", 4)),
               rtp=(("out", 0), ("no", 1), ("npk", 2)), rtpa=(("out", 0), ("no", 1), ("npk", 2)), rtpu=(("out", 0), ("io", 1), ("nau", 2), ("ats", 3)),
               rtpo=(("ooff", 0), ("osize", 1), ("src", 2), ("ext", 3)), mp4f=(("out", 0), ("so", 1), ("ss", 2), ("fr", 3)),
               mp4s=(("so", 0), ("ss", 1), ("dts", 2), ("pts", 3), ("sfl", 4), ("fr", 5)), stbl=(("so", 0), ("ss", 1), ("dts", 2), ("pts", 3), ("sfl", 4)),
               stblw=(("out", 0), ("tab", 1)),
               aut=(("dts", 0), ("pts", 1), ("order", 2), ("display", 3)), csub=(("sf", 0), ("sub", 1)), cenc=(("data", 0), ("ivo", 1)),
               cbcs=(("data", 0),), cbcsd=(("data", 0),))
PER_NAL_TABLES = ("io", "src", "nau")                # of hbs_au_insert: d_index_out, d_nal_src, d_nal_au_out
# "d_out == NULL: plan only -- ... the summary and d_tables are written"; "d_sub == NULL: plan only -- the summary and d_sub_first are written"
PLAN_WRITES = {"stblw": ("tab",), "csub": ("sf",)}
IN_PLACE = ("data",)                                 # the buffer hbs_cenc_crypt and hbs_cbcs_crypt work in: uploaded, and compared after an error too
SUMMARY_MATCHES = dict(a2l=LP, l2a=LP, tsd=TS, tsm=TM, ins=AI, rtp=TR, rtpa=TR, rtpu=TU, rtpo=TO, mp4f=TF, mp4s=TQ, stbl=TB, stblw=TW,
                       aut=TA, csub=TC, cenc=TC, cbcs=TY, cbcsd=TY)


def new_ctx():
    import hevcbitstream_amd as hbs
    return hbs.Context(0)


def dev(a):
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).cuda() if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")


def canary(n):
    return filled(n + PAD, CAN)


def filled(n, byte):
    import torch
    return torch.full((n,), byte, dtype=torch.uint8, device="cuda")


def opt(a):
    return dev(a) if a is not None else None


def alloc(c, tables=True, ts=None, given=None):
    """the case's inputs on the device, outputs of exactly c.room bytes with canaries behind them, a summary full of 0xEE.
    tables False: hbs_au_insert without its per-NAL tables; ts: a device tensor that holds hbs_ts_demux's input already; given:
    inputs that lie on the device already, by their names here (for hbs_mp4_stbl_samples also "rec", the host record)"""
    from hevcbitstream_amd.api import SUMMARY
    a = c.a
    b = dict(summary=filled(SUMMARY.itemsize, 0xEE))
    held = lambda name, make: given[name] if given and name in given else make()          # noqa: E731
    if c.call == "aut":
        b.update(au=held("au", lambda: dev(a["au"])), prm=T.params_record(**a["kw"]))
    elif c.call == "csub":
        b.update(stream=held("stream", lambda: dev(a["stream"])), index=held("index", lambda: dev(a["index"])),
                 nal_au=held("nal_au", lambda: dev(a["nal_au"])), keep=opt(a["keep"]), po=held("po", lambda: opt(a["po"])))
    elif c.call in S.CRYPT_CALLS:
        b.update(off=held("off", lambda: dev(a["off"])), size=held("size", lambda: dev(a["size"])), first=held("first", lambda: dev(a["first"])),
                 sub=held("sub", lambda: dev(a["sub"])), iv=opt(a["iv"]))
    elif c.call in ("rtp", "rtpa"):
        b.update(stream=dev(a["stream"]), index=dev(a["index"]), nal_au=opt(a["nal_au"]), pts=opt(a["pts"]), prm=R.params_record(a["prm"]))
    elif c.call in ("rtpu", "rtpo"):
        b.update(data=held("data", lambda: dev(a["data"])), off=held("off", lambda: dev(a["off"])), size=held("size", lambda: dev(a["size"])),
                 prm=(RU if c.call == "rtpu" else RO).params_record(a["prm"]))
    elif c.call == "mp4f":
        b.update(stream=dev(a["stream"]), index=dev(a["index"]), keep=opt(a["keep"]), nal_au=dev(a["nal_au"]), au=dev(a["au"]), dts=opt(a["dts"]),
                 pts=opt(a["pts"]), prm=MF.params_record(a["prm"]))
    elif c.call == "mp4s":
        b.update(data=held("data", lambda: dev(a["data"])), seg=None if a["segs"] is None else TQ.seg_table(a["segs"], a["stride"]))
    elif c.call == "stbl":
        b.update(data=held("data", lambda: dev(a["data"])), rec=held("rec", lambda: a["rec"]))
    elif c.call == "stblw":
        b.update({"in_" + k: v for k, v in TW.upload(a).items()})
    elif c.call == "a2l":
        b.update(s=dev(a["s"]), idx=dev(a["idx"]), keep=dev(a["keep"]) if a["keep"] is not None else None, nal_au=dev(a["nal_au"]))
    elif c.call == "l2a":
        b.update(data=dev(a["data"]), off=dev(a["off"]), size=dev(a["size"]))
    elif c.call == "tsd":
        b.update(ts=dev(a["ts"]) if ts is None else ts)
    elif c.call == "tsm":
        b.update(stream=dev(a["stream"]), au=dev(a["au"]), pts=dev(a["pts"]), dts=dev(a["dts"]), prm=TSM.params_record(a["prm"]))
    else:
        b.update(stream=dev(a["stream"]), index=dev(a["index"]), parsed=dev(a["parsed"]), au=dev(a["au"]), nal_au=dev(a["nal_au"]))
    for name, _ in OUTPUTS[c.call]:
        if c.call in S.CALLS3 and name not in c.room:          # a table hbs_au_times is not asked for; no d_iv that receives the counter blocks
            b[name] = None
            continue
        b[name] = canary(c.room[name]) if tables or name not in PER_NAL_TABLES else None
    if c.call in S.CRYPT_CALLS:                               # the data, fresh, in front of its canary (or the device's own: `given`)
        b["data"][: len(a["data"])].copy_(held("data", lambda: dev(a["data"]))[: len(a["data"])])
    return b


def launch(ctx, c, b, plan=False):
    """one call on the current torch stream -> its return code"""
    a, caps = c.a, c.caps
    o = {name: None if plan else b[name] for name, _ in OUTPUTS[c.call]}
    cap = lambda name: 0 if plan else caps[name]          # noqa: E731
    if c.call == "aut":
        return ctx.au_times_async(b["au"], len(a["au"]), b["prm"], b["summary"], dts=o["dts"], pts=o["pts"], order=o["order"], display=o["display"])
    if c.call == "csub":                                  # (a plan writes d_sub_first)
        import hevcbitstream_amd as hbs
        return ctx.cenc_subsamples_async(b["stream"], len(a["stream"]), b["index"], len(a["index"]), b["nal_au"], a["n_aus"],
                                         hbs.cenc_plan_params(length_size=a["L"], flags=a["flags"], clear_lead=a["clear_lead"]), b["sf"], o["sub"],
                                         b["summary"], keep=b["keep"], payload_off=b["po"], sub_cap=cap("sub_cap"))
    if c.call in S.CRYPT_CALLS:
        import hevcbitstream_amd as hbs
        tables = (b["data"], len(a["data"]), b["off"], b["size"], len(a["off"]), b["first"], b["sub"])
        if c.call == "cenc":
            return ctx.cenc_crypt_async(*tables, b["ivo"] if a["ivo"] else b["iv"], hbs.cenc_params(a["key"], iv0=a["iv0"]), b["summary"])
        flags = (hbs.CBCS_DECRYPT if c.call == "cbcsd" else 0) | (hbs.CBCS_WHOLE_RUNS if a["whole"] else 0)
        prm = hbs.cbcs_params(a["key"], iv0=a["iv0"], flags=flags, crypt_byte_block=a["c"], skip_byte_block=a["k"])
        return ctx.cbcs_crypt_async(*tables, b["iv"], prm, b["summary"])
    if c.call in ("rtp", "rtpa"):
        return ctx.rtp_pack_async(b["stream"], len(a["stream"]), b["index"], len(a["index"]), b["nal_au"], a["n_aus"], b["pts"], b["prm"], o["out"],
                                  o["no"], o["npk"], b["summary"], out_cap=cap("out_cap"))
    if c.call == "rtpu":
        return ctx.rtp_unpack_async(b["data"], len(a["data"]), b["off"], b["size"], len(a["off"]), b["prm"], o["out"], o["io"], o["nau"], o["ats"],
                                    b["summary"], out_cap=cap("out_cap"), nal_cap=cap("nal_cap"), au_cap=cap("au_cap"))
    if c.call == "rtpo":
        return ctx.rtp_order_async(b["data"], len(a["data"]), b["off"], b["size"], len(a["off"]), b["prm"], o["ooff"], o["osize"], o["src"], o["ext"],
                                   b["summary"], out_cap=cap("out_cap"))
    if c.call == "mp4f":
        return ctx.mp4_fragment_async(b["stream"], len(a["stream"]), b["index"], len(a["index"]), b["nal_au"], b["au"], len(a["au"]), b["prm"], o["out"],
                                      b["summary"], keep=b["keep"], dts=b["dts"], pts=b["pts"], sample_off=o["so"], sample_size=o["ss"], frag=o["fr"],
                                      frag_cap=cap("frag_cap"), out_cap=cap("out_cap"))
    if c.call == "mp4s":                                  # (moof_cap sizes the plan's scratch as well)
        import hevcbitstream_amd as hbs
        return ctx.mp4_samples_async(b["data"], len(a["data"]), hbs.mp4_read_params(**a["prm"]), b["summary"], seg=b["seg"], seg_stride=a["stride"],
                                     n_segs=0 if a["segs"] is None else len(a["segs"]), moof_cap=caps["moof_cap"], sample_cap=cap("sample_cap"),
                                     sample_off=o["so"], sample_size=o["ss"], dts=o["dts"], pts=o["pts"], sample_flags=o["sfl"], frag=o["fr"])
    if c.call == "stbl":
        return ctx.mp4_stbl_samples_async(b["data"], len(a["data"]), b["rec"], b["summary"], sample_cap=cap("sample_cap"), sample_off=o["so"],
                                          sample_size=o["ss"], dts=o["dts"], pts=o["pts"], sample_flags=o["sfl"])
    if c.call == "stblw":                                 # (a plan writes d_tables)
        return ctx.mp4_stbl_write_async(b["in_sample_off"], b["in_sample_size"], len(a["t"]["size"]), TW.params_of(a), b["summary"], dts=b["in_dts"],
                                        pts=b["in_pts"], sample_flags=b["in_sample_flags"], out=o["out"], out_cap=cap("out_cap"), tables=b["tab"])
    out_cap = 0 if plan else caps["out_cap"]
    if c.call == "a2l":
        return ctx.annexb_to_lenpref_async(b["s"], len(a["s"]), b["idx"], len(a["idx"]), o["out"], o["io"], b["summary"], keep=b["keep"],
                                           length_size=a["L"], nal_au=b["nal_au"], n_aus=a["n_aus"], sample_off=o["so"], out_cap=out_cap)
    if c.call == "l2a":
        return ctx.lenpref_to_annexb_async(b["data"], len(a["data"]), b["off"], b["size"], len(a["off"]), o["out"], o["so"], b["summary"],
                                           length_size=a["L"], startcode_bytes=a["sc"], nal_cap=(1 << 64) - 1 if plan else caps["nal_cap"], out_cap=out_cap)
    if c.call == "tsd":
        return ctx.ts_demux_async(b["ts"], len(a["ts"]), a["B"], a["pid"], o["out"], o["pes"], b["summary"], out_cap=out_cap,
                                  pes_cap=0 if plan else caps["pes_cap"])
    if c.call == "tsm":
        return ctx.ts_mux_async(b["stream"], len(a["stream"]), b["au"], len(a["au"]), b["pts"], b["dts"], b["prm"], o["out"], o["ap"], b["summary"],
                                out_cap=out_cap)
    return ctx.au_insert_async(b["stream"], len(a["stream"]), b["index"], b["parsed"], len(a["index"]), b["au"], b["nal_au"], len(a["au"]),
                               a["first"], a["count"], a["flags"], o["out"], o["io"], o["src"], o["nau"], o["auo"], b["summary"], out_cap=out_cap,
                               index_cap=0 if plan or o["io"] is None else caps["index_cap"])


def verify(ctx, c, b, plan=False):
    """the summary, every output and the canaries behind them against the plain loop; after an error nothing is written"""
    w = S.want(c, plan)
    ws = w[-1]
    s = ctx.read_summary(b["summary"])
    if c.call == "a2l" and ws["error"] == S.E_ARG:          # the header leaves the sizes open for HBS_E_ARG
        ws = {k: v for k, v in ws.items() if k not in ("nal_count", "rbsp_bytes", "stream_bytes")}
    SUMMARY_MATCHES[c.call].summary_matches(s, ws)
    assert int(s["reserved"][0]) == S.reserved0(ws), (s, ws)
    if c.named is not None:                                 # the word the header gives this fault, where this kind of call looks for it
        word, value = c.named
        if c.in_plan or not plan:
            error = c.error if c.call in S.CALLS3 else S.E_ARG          # (hbs_au_times names the AU under HBS_E_DEPTH)
            assert int(s["error"]) == error and int(s["reserved"][word]) == value, (c, s)
        else:
            assert int(s["error"]) == 0, (c, s)
    elif c.bad is not None:                                 # this call's own entry plus one, where the call names it
        assert int(s["error"]) == S.E_ARG and int(s["reserved"][0]) == (c.bad + 1 if S.names_the_entry(c.call) else 0), (c, s)
    refused_writes_nothing = c.call in S.CALLS or S.writes_nothing_when_refused(c.call)          # (the header says so for every call here)
    for name, place in OUTPUTS[c.call]:
        if b[name] is None:
            continue
        g = b[name].cpu().numpy()
        if (ws["error"] and refused_writes_nothing and name not in IN_PLACE) or (plan and name not in PLAN_WRITES.get(c.call, ())):
            assert (g == CAN).all(), "%s written by %s" % (name, "a plan" if plan else "a call that reports error %d" % ws["error"])
            continue
        x = np.ascontiguousarray(w[place])
        item, want_bytes = x.itemsize, x.view(np.uint8).reshape(-1)
        assert len(want_bytes) == c.room[name] - c.spare.get(name, 0), (name, len(want_bytes), c.room[name], c.spare)
        bad = np.flatnonzero(g[: len(want_bytes)] != want_bytes)
        assert len(bad) == 0, "%s differs at entry %d (byte %d; %d bytes of %d differ)" % (name, bad[0] // item, bad[0], len(bad), len(want_bytes))
        assert (g[len(want_bytes):] == CAN).all(), "stored behind " + name
    return s


def step(ctx, c, plan=False, tables=True, ts=None, given=None):
    """one real call of the case into canary-backed outputs of exactly the case's capacities, held against the reference
    -> the device buffers"""
    b = alloc(c, tables, ts, given)
    rc = launch(ctx, c, b, plan)
    assert rc == 0, (c, rc)
    verify(ctx, c, b, plan)
    return b


def run_steps(ctx, steps):
    """steps: [(case, plan only?)] or [(case, plan only?, keywords of step)]"""
    for k, st in enumerate(steps):
        c, plan, kw = st if len(st) == 3 else st + ({},)
        try:
            step(ctx, c, plan, **kw)
        except AssertionError as e:
            raise AssertionError("step %d of %d, %r%s%s: %s" % (k + 1, len(steps), c, " (plan only)" if plan else "", " %s" % kw if kw else "", e)) from e


def on_one_context(steps):
    ctx = new_ctx()
    try:
        run_steps(ctx, steps)
    finally:
        ctx.close()


# ---- large, small, large bad-late, small, small bad-early, odd, empty, large short, large plan-only, large -------------------

def test_annexb_to_lenpref_sequence():
    on_one_context(S.sequence("a2l"))


def test_lenpref_to_annexb_sequence():
    on_one_context(S.sequence("l2a"))


@pytest.mark.parametrize("B", PACKET_SIZES)
def test_ts_demux_sequence(B):
    """lay_ts puts the per-block words first and the control words behind them: a small call's control words lie where the
    large call in front of it kept block words"""
    on_one_context(S.sequence("tsd", B=B))


@pytest.mark.parametrize("B", PACKET_SIZES)
def test_ts_mux_sequence(B):
    """the copy's workgroups are counted from out_cap: the plan, the run a byte short and the run carve differently"""
    on_one_context(S.sequence("tsm", B=B))


def test_au_insert_sequence():
    on_one_context(S.sequence("ins"))


# ---- three more sequences -----------------------------------------------------------------------------------------------------

def test_the_length_prefix_calls_share_one_buffer():
    """lay_a2l and lay_l2a lay the same buffer out in two ways"""
    on_one_context([(S.case(call, which), False) for call, which in (("a2l", "large"), ("l2a", "small"), ("a2l", "small"), ("l2a", "large"),
                                                                     ("a2l", "odd"), ("l2a", "odd"))])


def ranged(good, first, count):
    a = dict(good.a, first=first, count=count)
    return S.finish(S.Case("ins", "%s, AUs %d + %d" % (good.name, first, count), a))


def test_au_insert_ranges_on_one_context():
    """the AU-side workgroups run for the blocks of the range alone, and none for an empty range: the whole range, its last
    block, an empty range, the first AU, a middle block; with every table and without the per-NAL ones"""
    large = S.case("ins", "large")
    m = len(large.a["au"])
    last = (S.blocks(m, S.INS_AU_BLOCK) - 1) * S.INS_AU_BLOCK
    ranges = [ranged(large, 0, m), ranged(large, last, m - last), ranged(large, m, 5), ranged(large, 0, 1), ranged(large, 3 * S.INS_AU_BLOCK, S.INS_AU_BLOCK)]
    assert [S.summary_of(r)["reserved"][2] for r in ranges] == [m, m - last, 0, 1, S.INS_AU_BLOCK] and 0 < m - last < S.INS_AU_BLOCK
    assert last > 4 * S.INS_AU_BLOCK
    on_one_context([(r, False, dict(tables=tables)) for tables in (True, False) for r in ranges])


def all_five(which):
    """mux, demux of its output, insert, forward and back -> the cases (the demux's input is the mux's reference output)"""
    mux = S.case("tsm", which)
    return mux, S.demux_of(mux), S.case("ins", which), S.case("a2l", which), S.case("l2a", which)


def test_all_five_interleaved_on_one_context():
    """as test_gpu_scratch.py::test_buffers_grow_under_a_live_context for the older calls: every buffer grows under the
    context between the first round (small) and the second (large); the third is small calls behind large ones in all five,
    the fourth large ones behind small ones in buffers that no longer grow"""
    assert S.plan_blocks(all_five("large")[1])[0] >= 3 and S.plan_blocks(all_five("small")[1])[0] == 1
    ctx = new_ctx()
    try:
        held = []
        for which in ("small", "large", "small", "large"):
            mux, demux, ins, fw, back = all_five(which)
            out = step(ctx, mux)["out"]
            step(ctx, demux, ts=out[: mux.room["out"]])           # the device's own packets
            run_steps(ctx, [(ins, False), (fw, False), (back, False)])
            held.append(ctx.device_bytes())
    finally:
        ctx.close()
    assert held[1] > held[0] and held[1] == held[2] == held[3], held


# ---- two contexts at once -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", ("tsd", "tsm", "ins"))
def test_two_contexts_at_the_same_time(call):
    """the small and the large case on a context and a stream each, three rounds enqueued alternately, one wait at the end"""
    import torch
    jobs = [S.case(call, "small"), S.case(call, "large")]
    for c in jobs:
        S.want(c)
    streams = [torch.cuda.Stream() for _ in jobs]
    ctxs, bufs = [], []
    try:
        for c, st in zip(jobs, streams):
            with torch.cuda.stream(st):
                ctxs.append(new_ctx())
                bufs.append(alloc(c))
        for r in range(3):
            for c, st, ctx, b in zip(jobs, streams, ctxs, bufs):
                with torch.cuda.stream(st):
                    assert launch(ctx, c, b) == 0
        torch.cuda.synchronize()
        for c, ctx, b in zip(jobs, ctxs, bufs):
            verify(ctx, c, b)
    finally:
        for ctx in ctxs:
            ctx.close()
