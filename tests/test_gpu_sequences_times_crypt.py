"""The timing and encryption calls back to back on one live context, as tests/test_gpu_sequences.py holds the framing and transport
calls (its helpers are used here) and tests/test_gpu_sequences_rtp_mp4.py the RTP and MP4 calls: hbs_au_times, hbs_cenc_subsamples,
hbs_cenc_crypt, hbs_cbcs_crypt encrypting and with HBS_CBCS_DECRYPT.  hbs_au_times and hbs_cenc_subsamples lay their scratch out by
their input alone (hbs_autimes.h: lay_au_times, hbs_cenc.h: lay_cenc_plan); the two crypt calls carve ONE buffer with one function
(hbs_cenc.h: lay_cenc_args), in which at_b, at_k, part_s, part_r and ctl move with n_samples.  Every step is held, byte for byte
and field for field, against the plain loops of tests/_au_times_ref.py, tests/_cenc_ref.py and tests/_cbcs_ref.py: never against
another context.  The buffer the crypt calls work in is uploaded fresh for every step and compared whole, the bytes between and
around the samples and a canary behind data_bytes included.  The cases are tests/_seq_cases.py's (CALLS3); tests/test_seq_cases.py
holds on the CPU that they are what the sequences need.  The crypt calls have no plan, so their sequences have no plan-only step.

What the kernels read of the scratch, which kernel of the same call writes it first, and the step that would put another call's
values there (a reading of hbs_autimes.hip, hbs_cenc.hip and hbs_cbcs.hip; the reading found every word written before it is read):
  hbs_au_times       key[a], bits[a] by k_aut_digest for every AU below n_aus (a key of 0 where no picture lies in front of the AU
                     in its workgroup), key[a] again by k_aut_apply for those; read by k_aut_apply and k_aut_rank.  pmax[a], smin[a]
                     by k_aut_apply for every AU (smin with the lanes in reverse); read by k_aut_rank, which stages AUs base - 64
                     to base + 320 of [0, n_aus) alone and walks beyond them in memory, never to an AU at or behind n_aus: a head,
                     the table's end (pmax, smin of the last AU are its own key) or the span limit ends a walk.  ord[a] by
                     k_aut_rank, read by k_aut_write.  part[8 w .. 8 w + 8) all by lane 0 of k_aut_digest; key, max, min rescanned
                     by k_aut_parts; lag, bad and (over the heads) the late AUs by k_aut_rank; read by k_aut_apply and k_aut_reduce
                     over the call's workgroups alone.  ctl: segments and last head by k_aut_parts, read by k_aut_reduce only when
                     there is a workgroup; bad and delay by k_aut_reduce in every call, read by k_aut_write.  The steps: the tables
                     of falling and rising size (the words right behind n_aus are the larger table's, with keys that would change
                     the ranks); the good table behind the refused one (ctl's bad word).
  hbs_cenc_subsamples  part_a[8 w .. 8 w + 3) by lane 0 of k_cenc_runs, word 0 rescanned by k_cenc_carry, read by k_cenc_count and
                     k_cenc_place; part_b[8 w .. 8 w + 5) by k_cenc_count, scanned by k_cenc_plan, word 0 read by k_cenc_place;
                     ctl[0] by k_cenc_plan in every call (no NALs: the only launch), read by k_cenc_place.  The steps: the small
                     call behind the refused one (ctl[0]); the run behind the plan; the run an entry short.
  hbs_cenc_crypt, hbs_cbcs_crypt (the checks are one function, enqueue_cenc_checks)
                     part_s[8 w] by k_cenc_samples, read by k_cenc_begin; again by k_cenc_sizes, read by k_cenc_verdict.  ctl: bad
                     and entries by k_cenc_begin, protected bytes (and a bad clear count) by k_cenc_range_scan, the error by
                     k_cenc_verdict, all in every call.  part_r[8 g .. 8 g + 3) of all 1 024 ranges by k_cenc_range_sum (zeros for
                     a range without entries, and for all of them after an error of the first group), words 0 and 1 scanned and
                     entry 1 024 written by k_cenc_range_scan; read by k_cenc_at, k_cenc_crypt, k_cbcs_crypt.  part_r[8 g + 3] by
                     k_cbcs_crypt for every range, read by k_cbcs_summary of the same call; hbs_cenc_crypt neither writes nor reads
                     it.  at_b[s], at_k[s] for s in [0, n_samples] by k_cenc_at: by the workgroup and step that sample's first entry
                     lies in, the end (and the samples without entries behind the last entry) by the step that ends with the last
                     entry, all of them by workgroup 0 when there is no entry at all (E == 0) -- and none when a check has failed,
                     after which k_cenc_sizes, k_cenc_crypt and k_cbcs_crypt read none.  The steps: the table without any entry
                     behind large tables (without the E == 0 branch k_cenc_sizes reads the large table's at_b and refuses the
                     call); either call behind the other with more and with fewer samples (every array but at_b moves); the small
                     good call behind the refused large one (at_b, at_k keep what the call before the refused one left).
"""
import numpy as np
import pytest

from tests import _au_ref as AU
from tests import _au_times_ref as T
from tests import _cbcs_ref as CB
from tests import _cenc_ref as CR
from tests import _mp4_ref as MF
from tests import _seq_cases as S
from tests.test_gpu_au_times import summary_matches as au_times_summary_matches
from tests.test_gpu_sequences import CAN, alloc, canary, dev, filled, launch, new_ctx, on_one_context, verify

pytestmark = pytest.mark.gpu


# ---- large, small, large bad-late, small, small bad-early, odd (and, for the crypt calls, the table without any entry), empty,
# ---- hbs_cenc_subsamples: large an entry short, small roomy; hbs_au_times and hbs_cenc_subsamples: large plan-only; large --------

@pytest.mark.parametrize("call", S.CALLS3)
def test_sequence(call):
    on_one_context(S.sequence3(call))


def test_the_crypt_calls_share_one_buffer():
    """lay_cenc_args lays one buffer out for both calls: each behind the other with more and with fewer samples, the tables without
    any entry behind tables with many, a refused call directly in front of a small good one"""
    on_one_context(S.shared_crypt_steps())


def test_au_times_tables_of_falling_and_rising_size():
    """the small tables hold pyramids, so their walks want neighbours; the large table in front of them holds falling keys, which
    would lower every rank that read one of them"""
    B = S.AUT_BLOCK
    rng = np.random.default_rng(12)
    steps = []
    for k, n in enumerate((3 * B + 11, 1, B + 1, 0, B - 1, 3 * B + 11)):
        keys = (100000 - 3 * np.arange(n)).tolist() if n > 2 * B else T.pyramid(8, n // 8 + 1)[:n]
        c = S.finish(S.Case("aut", "%d AUs (step %d)" % (n, k), dict(au=T.table(keys, junk=rng), kw=dict(tick=1001, base_time=7 * k),
                                                                     outs=tuple(name for name, _ in S.AUT_TABLES))))
        steps.append((c, False))
    R = [S.summary_of(c)["reserved"][1] for c, _ in steps]
    assert R == [3 * B + 10, 0, 3, 0, 3, 3 * B + 10]          # the large tables are turned round, the small ones hold GOPs of 8
    on_one_context(steps)


# ---- a pipeline in rounds, each stage fed the device's own output of the stage in front ----------------------------------------------

def same(got, want, what):
    got, want = (np.ascontiguousarray(x).view(np.uint8).reshape(-1) for x in (got, want))
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s differs at byte %d (%d of %d differ)" % (what, bad[0], len(bad), len(want))


def held(t, nbytes, what):
    """the first nbytes of a canary-backed output, and nothing stored behind them"""
    g = t.cpu().numpy()
    assert (g[nbytes:] == CAN).all(), "stored behind " + what
    return g[:nbytes]


def pipeline(ctx, n_pictures, slices, idr_every):
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import COMPACT, PARSED, SUMMARY
    from tests import _orc
    from tests.hevc_synth import stream_4k30
    from tests.test_gpu_au import host_records, same_records, sps_off
    stream, n = stream_4k30(9, n_pictures=n_pictures, slices_per_picture=slices, idr_every=idr_every, payload_bytes=(60, 200))
    src = np.frombuffer(stream, dtype=np.uint8)
    d = torch.from_numpy(src.copy()).cuda()
    summary = lambda: filled(SUMMARY.itemsize, 0xEE)          # noqa: E731
    # 1. hbs_index_parse_compact: the index against the oracle's (the parsed records are held by what the stages behind make of them)
    cap = n + 8
    index, parsed, cc = (torch.zeros(cap * z, dtype=torch.uint8, device="cuda") for z in (32, PARSED.itemsize, COMPACT.itemsize))
    structs, po = torch.zeros(8 << 20, dtype=torch.uint8, device="cuda"), torch.zeros(cap * 8, dtype=torch.uint8, device="cuda")
    ss, ps = summary(), summary()
    got = ctx.index_parse_compact_async(d, index, cap, parsed, cc, structs, ss, ps, payload_off=po)
    assert got == n and int(ctx.read_summary(ps)["error"]) == 0 and int(ctx.read_summary(ss)["error"]) == 0
    recs = host_records(got, index, parsed, cc, structs)
    want_idx = _orc.oracle().index_extract(src)[0]
    assert len(want_idx) == n and np.array_equal(recs[0]["start"], want_idx["start"]) and np.array_equal(recs[0]["end"], want_idx["end"])
    idx, h_po = index[: got * 32], po[: got * 8].cpu().numpy().view(np.uint64)
    # 2. hbs_access_units
    au, nal_au, s, _ = ctx.access_units(index, parsed, cc, structs, got)
    want_au, want_nal_au, _, _ = AU.access_units(*recs, sps_off(ctx))
    same_records(au, want_au)
    assert np.array_equal(nal_au, want_nal_au) and len(au) == n_pictures
    n_aus = len(au)
    # 3. hbs_au_times
    kw = dict(tick=3003, base_time=900000)
    want_t = T.au_times(au, **kw)
    d_au = dev(au)
    times = {name: canary(n_aus * width) for name, width in S.AUT_TABLES}
    sm = summary()
    assert ctx.au_times_async(d_au, n_aus, T.params_record(**kw), sm, **times) == 0
    au_times_summary_matches(ctx.read_summary(sm), want_t["summary"])
    for name, width in S.AUT_TABLES:
        same(held(times[name], n_aus * width, name), want_t[name], name)
    # 4. hbs_mp4_fragment with those times
    dts, pts = times["dts"][: n_aus * 8], times["pts"][: n_aus * 8]
    out, so, sz, frags, s = ctx.mp4_fragment(d, idx, nal_au, d_au, dts=dts, pts=pts, flags=hbs.MP4_CUT_AT_IRAP, sample_duration=3003, track_id=1)
    want_f = MF.fragment(src, recs[0], None, nal_au, au, want_t["dts"], want_t["pts"], MF.params(flags=MF.CUT_AT_IRAP, sample_duration=3003, track_id=1))
    same(out.cpu().numpy(), want_f[0], "fragments")
    same(so, want_f[1], "sample_off"), same(sz, want_f[2], "sample_size"), same(frags, want_f[3], "frags")
    plain = out.cpu().numpy().copy()
    # 5. hbs_cenc_subsamples
    want_s = CR.subsamples(src, recs[0]["start"].astype(np.int64), recs[0]["end"].astype(np.int64), nal_au, n_aus, 4, payload_off=h_po)
    total = len(want_s["sub"])
    assert want_s["error"] == 0
    sf, sub, sm = canary((n_aus + 1) * 8), canary(total * 8), summary()
    assert ctx.cenc_subsamples_async(d, len(src), idx, got, dev(nal_au), n_aus, hbs.cenc_plan_params(length_size=4), sf, sub, sm,
                                     payload_off=po[: got * 8], sub_cap=total) == 0
    s = ctx.read_summary(sm)
    assert (int(s["error"]), int(s["nal_count"]), int(s["rbsp_bytes"]), int(s["stream_bytes"])) == (0, total, want_s["protected"], int(sz.sum()))
    same(held(sf, (n_aus + 1) * 8, "sub_first"), want_s["sub_first"], "sub_first"), same(held(sub, total * 8, "sub"), want_s["sub"], "sub")
    tables = (dev(so), dev(sz), n_aus, sf[: (n_aus + 1) * 8], sub[: total * 8])
    h_tables = (so, sz, want_s["sub_first"], want_s["sub"])
    key, iv0 = bytes(range(16, 32)), bytes(range(100, 116))

    def crypt_summary(sm, done):
        s = ctx.read_summary(sm)
        assert ([int(s[k]) for k in ("error", "nal_count", "nal_found", "rbsp_bytes", "stream_bytes")], list(s["reserved"])) == \
            ([0, total, n_aus, done, len(plain)], [0, 0, 0])
    # 6. hbs_cbcs_crypt encrypting (1:9, the constant IV)
    other = out.clone()
    want_e, done = CB.crypt_many(plain, *h_tables, key, iv0=iv0)
    sm = summary()
    assert ctx.cbcs_crypt_async(out, len(plain), *tables, None, hbs.cbcs_params(key, iv0=iv0), sm) == 0
    crypt_summary(sm, done)
    same(out.cpu().numpy(), want_e, "cbcs ciphertext")
    # 7. hbs_cenc_crypt on a copy, sequential IVs into a d_iv
    want_c, done_c, used = CR.crypt(plain, *h_tables, key, iv0=bytes(8))
    ivo, sm = canary(n_aus * 16), summary()
    assert ctx.cenc_crypt_async(other, len(plain), *tables, ivo, hbs.cenc_params(key, iv0=bytes(8)), sm) == 0
    crypt_summary(sm, done_c)
    same(other.cpu().numpy(), want_c, "cenc ciphertext"), same(held(ivo, n_aus * 16, "d_iv"), used, "d_iv")
    same(out.cpu().numpy(), want_e, "cbcs ciphertext behind hbs_cenc_crypt")
    # 8. hbs_cbcs_crypt decrypting
    sm = summary()
    assert ctx.cbcs_crypt_async(out, len(plain), *tables, None, hbs.cbcs_params(key, iv0=iv0, flags=hbs.CBCS_DECRYPT), sm) == 0
    crypt_summary(sm, done)
    same(out.cpu().numpy(), plain, "cbcs plaintext")
    # 9. hbs_lenpref_to_annexb gives the source NALs back
    back, _, _ = ctx.lenpref_to_annexb(out, so, sz, length_size=4, startcode_bytes=4)
    assert bytes(back.cpu().numpy()) == b"".join(b"\x00\x00\x00\x01" + bytes(src[int(e["start"]):int(e["end"])]) for e in recs[0])
    return n, n_aus, total


def test_pipeline_in_rounds_on_one_context():
    """as tests/test_gpu_sequences_rtp_mp4.py::test_pipeline_in_rounds_on_one_context: the buffers grow between the first round
    (small) and the second (large); the third is small calls behind large ones, the fourth large ones in buffers that no longer grow"""
    ctx = new_ctx()
    try:
        sizes, grown = [], []
        for which in ("small", "large", "small", "large"):
            sizes.append(pipeline(ctx, 36, 2, 12) if which == "small" else pipeline(ctx, 2 * S.AUT_BLOCK + 8, 4, 40))
            grown.append(ctx.device_bytes())
    finally:
        ctx.close()
    assert sizes[0][1] < S.AUT_BLOCK and sizes[0][0] < S.CENC_NAL_BLOCK and sizes[0][2] < S.CRYPT_RANGES
    assert sizes[1][1] > 2 * S.AUT_BLOCK and sizes[1][0] > S.CENC_NAL_BLOCK and sizes[1][2] > S.CRYPT_RANGES
    assert grown[1] > grown[0] and grown[1] == grown[2] == grown[3], grown


# ---- two contexts at once -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", ("aut", "cenc", "cbcsd"))
def test_two_contexts_at_the_same_time(call):
    """the small and the large case on a context and a stream each, three rounds enqueued alternately, one wait at the end.  The
    crypt calls work in place: three rounds of hbs_cenc_crypt are one (the XOR three times); for hbs_cbcs_crypt decrypting every
    round begins with a copy of the uploaded data, on the device and on the call's stream, so that the reference is the one call's"""
    import torch
    jobs = [S.case(call, "small"), S.case(call, "large")]
    for c in jobs:
        S.want(c)
    streams = [torch.cuda.Stream() for _ in jobs]
    ctxs, bufs, fresh = [], [], []
    try:
        for c, st in zip(jobs, streams):
            with torch.cuda.stream(st):
                ctxs.append(new_ctx())
                bufs.append(alloc(c))
                fresh.append(bufs[-1]["data"].clone() if call == "cbcsd" else None)
        torch.cuda.synchronize()
        for r in range(3):
            for c, st, ctx, b, f in zip(jobs, streams, ctxs, bufs, fresh):
                with torch.cuda.stream(st):
                    if f is not None:
                        b["data"].copy_(f)
                    assert launch(ctx, c, b) == 0
        torch.cuda.synchronize()
        for c, ctx, b in zip(jobs, ctxs, bufs):
            verify(ctx, c, b)
    finally:
        for ctx in ctxs:
            ctx.close()
