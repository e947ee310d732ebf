"""The RTP and MP4 calls back to back on one live context, as tests/test_gpu_sequences.py holds the five older framing and transport
calls (its helpers are used here): hbs_rtp_pack without and with HBS_RTP_AGGREGATE, hbs_rtp_unpack, hbs_rtp_order, hbs_mp4_fragment,
hbs_mp4_samples, hbs_mp4_stbl_samples and hbs_mp4_stbl_write.  Their scratch is laid out by capacities the caller passes as well as
by the input (hbs_rtp.h: lay_rtp, hbs_rtpun.h: lay_rtpu, hbs_rtpord.h: lay_rtpo, hbs_mp4.h: lay_mp4, hbs_mp4rd.h: lay_mp4rd,
hbs_mp4stbl.h: lay_mp4stbl, hbs_mp4stblw.h: lay_mp4stblw), so every sequence also runs the same input with more room than it needs
between two other calls: that moves the control words and every array behind them onto what the call in front left there.  Every
step is held, byte for byte and field for field, against the plain loops of tests/_*_ref.py: never against another context.  The
cases are tests/_seq_cases.py's; tests/test_seq_cases.py holds on the CPU that they are what the sequences need.

What the kernels read of the scratch, which kernel of the same call writes it first, and the step that would put another call's
values there (a reading of the .hip files; the tests found every word written before it is read):
  hbs_rtp_pack       part[0..4] by k_rtp_count in every workgroup, scanned by k_rtp_scan, read by k_rtp_place; ctl[0..2] by
                     k_rtp_scan, read by place, tiles and copy (the small call behind the refused one: with ctl[0] written only on
                     an error that step, and no other, fails); rec_*[k] by k_rtp_place and [n_nals] by k_rtp_scan, rec_ap only
                     with HBS_RTP_AGGREGATE and read only then (the alternating test); tile_first up to the tile behind the
                     output's last by k_rtp_tiles, and k_rtp_copy leaves before it reads one for a tile at or behind the total
                     (the roomy steps: the copy's grid covers out_cap).
  hbs_rtp_unpack     rec by k_rtpu_class for every packet; ap by k_rtpu_class and read by gives() for aggregation packets alone
                     (the odd case); both chain_w words of every chain by k_rtpu_chain; state, part_n[0..5], last_n by
                     k_rtpu_count; part_c by k_rtpu_class; part_a by k_rtpu_au; ctl by k_rtpu_scan_c and k_rtpu_scan_n; the piece
                     tables by k_rtpu_place and piece_out[pieces] by k_rtpu_scan_a; tile_first by k_piece_tiles as above.  nal_cap
                     and out_cap size the piece tables, so the roomy steps move ctl and everything behind it.
  hbs_rtp_order      slot[0, span) by k_rtpo_clear in every call, before k_rtpo_mark (the table without a loss in front of the
                     tables that lose a half); rec, part_a, last_a by k_rtpo_class; ext, part_d by k_rtpo_diff; last_m, low_m by
                     k_rtpo_late; moved_m by k_rtpo_moved; part_s by k_rtpo_count; ctl[0..5] by k_rtpo_scan_a and k_rtpo_scan_m.
                     part_s and ctl lie behind the max_span slots (max_span large, small, large; the roomy steps).
  hbs_mp4_fragment   part_n[0..2] by k_mp4_nal_count; last, bad_a by k_mp4_au_count; ctl by k_mp4_scan and k_mp4_finish; au_B[a]
                     by k_mp4_nal_place at each AU's first NAL and [n_aus] by k_mp4_scan; rec_B, rec_delta by k_mp4_nal_place;
                     part_a by k_mp4_frag_count, which a bad NAL skips together with its scan; au_frag, frag_off, frag_first by
                     k_mp4_frag_place and entry R by k_mp4_finish; tile_frag, tile_rec by k_mp4_tiles.  A plan carves none of
                     the tables behind au_B (plan, then run), out_cap the tile words (roomy).
  hbs_mp4_samples    part_s, seg_cnt by k_rd_seg<0>; all of ctl by k_rd_scan_seg; moof_at, moof_size, moof_seg, moof_span by
                     k_rd_seg<1>; moof_cnt, part_m[0..2] by k_rd_moof<0>; trun, trun_first, frag_tmp by k_rd_moof<1> and
                     trun_first[truns] by k_rd_scan_moof; part_e by k_rd_moof<2> (plan); part_k[0..3] by k_rd_samp<0>; part_c
                     by k_rd_samp<1>.  Grids and scans run over moof_cap and sample_cap: the workgroups behind the counts write
                     zeros (the roomy steps, and the small roomy one behind the two short ones).
  hbs_mp4_stbl_samples  all of ctl by k_st_head; part_r[0..5] by k_st_runs<0>; the first-sample tables by k_st_runs<1>; part_k
                     by k_st_samp<0>; part_c by k_st_sizes over the stsz's entries in a plan and by k_st_samp<1> over sample_cap
                     in a run (plan, then run; roomy).
  hbs_mp4_stbl_write last by k_sw_breaks, written and read with max_chunk_samples alone (the odd case); part_r[0..4], part_s[0..4]
                     by k_sw_samp<0>; ctl by k_sw_plan and k_sw_finish, the offsets read only where kStop is 0 (the small call
                     behind the refused one); chunk_first, stts_first, ctts_first by k_sw_samp<1>; part_c by k_sw_chunk<0>."""
import numpy as np
import pytest

from tests import _rtp_order_ref as RO
from tests import _rtp_unpack_ref as RU
from tests import _seq_cases as S
from tests.test_gpu_sequences import alloc, launch, new_ctx, on_one_context, step, verify

pytestmark = pytest.mark.gpu


# ---- large, large roomy, small, large bad-late, small, small bad-early, odd, empty, each large short variant, small roomy,
# ---- large plan-only, large -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", S.CALLS2)
def test_sequence(call):
    on_one_context(S.sequence2(call))


def test_rtp_pack_with_and_without_aggregation_alternating():
    """rec_ap is carved with HBS_RTP_AGGREGATE alone, and tile_first lies behind it: the two kinds of call lay the same buffer
    out in two ways"""
    plain, agg = (lambda which: S.case("rtp", which)), (lambda which: S.case("rtpa", which))
    on_one_context([(c, plan) for c, plan in ((agg("large"), False), (plain("large"), False), (agg("small"), False), (plain("small"), False),
                                               (agg("large"), True), (plain("large"), False), (S.variant(agg("large"), "roomy"), False),
                                               (plain("odd"), False), (agg("odd"), False), (S.variant(plain("large"), "short"), False),
                                               (agg("large"), False), (S.empty("rtp"), False), (agg("small"), False))])


def spanned(good, max_span, name):
    return S.finish(S.Case("rtpo", "%s, max_span %d (%s)" % (good.name, max_span, name), dict(good.a, prm=dict(good.a["prm"], max_span=max_span))))


def test_rtp_order_spans_and_slots_left_taken():
    """the slot array has max_span entries and part_s and ctl lie behind it: the same packets with a large, a small and a large
    max_span; then a table without a loss, which takes every slot of its span, in front of tables of the same span of which
    a tenth and a half of the packets are lost"""
    rng = np.random.default_rng(11)
    small = S.case("rtpo", "small")
    span = S.summary_of(small)["stream_bytes"]
    wide = 2 * S.case("rtpo", "large").a["prm"]["max_span"] + 77
    steps = [(spanned(small, wide, "wide"), False), (spanned(small, span, "exact"), False), (spanned(small, wide, "wide again"), False)]
    n = 3 * S.RTPO_BLOCK + 50
    packets = [RU.packet(RU.random_nal(rng, 5), (65400 + k) & 0xFFFF, 90 * k) for k in range(n)]
    for lost in (0, n // 10, n // 2, 0, n // 2):
        lose = sorted(int(x) for x in rng.choice(np.arange(1, n - 1), size=lost, replace=False))
        arrived, _ = RO.arrive(packets, rng, window=8, lose=lose)
        data, off, size = RU.lay_out(arrived, rng)
        c = S.finish(S.Case("rtpo", "%d packets of %d lost" % (lost, n), dict(data=data, off=off, size=size, prm=RO.params(max_span=n))))
        s = S.summary_of(c)
        assert s["stream_bytes"] == n and s["nal_count"] == n - lost and s["reserved"][1] == lost, s
        steps.append((c, False))
    on_one_context(steps)


# ---- three pipelines, each stage fed the device's own output of the stage in front -----------------------------------------------

def rtp_pipeline(ctx, which, pack_call):
    """hbs_rtp_pack, hbs_rtp_order of the packet table shuffled on the host, hbs_rtp_unpack of the table hbs_rtp_order wrote"""
    pack = S.case(pack_call, which)
    order = S.order_of(pack)
    packed = step(ctx, pack)["out"]
    tabs = step(ctx, order, given=dict(data=packed))
    step(ctx, S.unpack_of(order), given=dict(data=packed, off=tabs["ooff"], size=tabs["osize"]))


def mp4_pipeline(ctx, which):
    frag = S.case("mp4f", which)
    step(ctx, S.samples_of(frag), given=dict(data=step(ctx, frag)["out"]))


def stbl_pipeline(ctx, which):
    """the boxes and the record hbs_mp4_stbl_write wrote; the record is host memory for hbs_mp4_stbl_samples, so it is copied
    back, and the size of the file the offsets mean is the caller's to add"""
    write = S.case("stblw", which)
    b = step(ctx, write)
    rec = b["tab"][: S.MS.STBL.itemsize].cpu().numpy().view(S.MS.STBL).copy()
    rec["file_bytes"] = S.STBL_FILE_BYTES
    step(ctx, S.stbl_of(write), given=dict(data=b["out"], rec=rec))


PIPELINES = {"rtp_pack, rtp_order, rtp_unpack": lambda ctx, which: rtp_pipeline(ctx, which, "rtp"),
             "rtp_pack with aggregation, rtp_order, rtp_unpack": lambda ctx, which: rtp_pipeline(ctx, which, "rtpa"),
             "mp4_fragment, mp4_samples": mp4_pipeline, "mp4_stbl_write, mp4_stbl_samples": stbl_pipeline}


@pytest.mark.parametrize("name", list(PIPELINES))
def test_pipeline_in_rounds_on_one_context(name):
    """as test_gpu_sequences.py::test_all_five_interleaved_on_one_context: the buffers grow between the first round (small) and
    the second (large); the third is small calls behind large ones, the fourth large ones in buffers that no longer grow"""
    ctx = new_ctx()
    try:
        held = []
        for which in ("small", "large", "small", "large"):
            PIPELINES[name](ctx, which)
            held.append(ctx.device_bytes())
    finally:
        ctx.close()
    assert held[1] > held[0] and held[1] == held[2] == held[3], held


def test_all_three_pipelines_interleaved_on_one_context():
    ctx = new_ctx()
    try:
        held = []
        for which in ("small", "large", "small", "large"):
            for name in PIPELINES:
                PIPELINES[name](ctx, which)
            held.append(ctx.device_bytes())
    finally:
        ctx.close()
    assert held[1] > held[0] and held[1] == held[2] == held[3], held


# ---- two contexts at once -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", ("rtpo", "mp4s", "stblw"))
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
