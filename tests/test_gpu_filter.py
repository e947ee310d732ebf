"""hbs_filter_annexb on the device against the numpy reference (tests/_filter_ref.py): output bytes, output index and every
summary field, on random streams, rules and keep masks; re-scan of the output; a 4K30 stream with temporal sub-layers; exact
capacity with canaries; errors; dense tiny NALs; tiles whose table does not fit LDS; a stream above 4 GiB; two contexts at the
same time."""
import numpy as np
import pytest

from tests import _filter_ref as F

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
TILE = 65536            # output bytes of one copy workgroup
LDS_UNITS = 2048        # units of a tile the copy stages in LDS; more are read from memory


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def run(ctx, s, idx, rule=None, keep=None, out_cap=None):
    """plan, then filter into an output of exactly out_cap bytes (default: the planned size) with canaries behind it.
    Returns (summary, out bytes [0, out_cap), index_out entries, canaries intact, index_out canaries intact)"""
    import torch
    d_s, d_i = dev(s), dev(idx)
    d_k = dev(np.asarray(keep, dtype=np.uint8)) if keep is not None else None
    summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ctx.filter_annexb_async(d_s, len(s), d_i, len(idx), None, None, summ, rule=rule, keep=d_k)
    plan = ctx.read_summary(summ)
    need = int(plan["stream_bytes"])
    cap = need if out_cap is None else out_cap
    out = torch.full((cap + PAD,), CAN, dtype=torch.uint8, device="cuda")
    io = torch.full((len(idx) * 32 + PAD,), CAN, dtype=torch.uint8, device="cuda")
    summ.fill_(0xEE)
    ctx.filter_annexb_async(d_s, len(s), d_i, len(idx), out, io, summ, rule=rule, keep=d_k, out_cap=cap)
    sm = ctx.read_summary(summ)
    assert int(plan["stream_bytes"]) == int(sm["stream_bytes"])
    o = out.cpu().numpy()
    i = io.cpu().numpy()
    kept = int(sm["nal_count"])
    written = kept * 32 if int(sm["error"]) == 0 else 0          # on an error the output index stays untouched too
    return sm, o[:cap], i[:written].view(F.NAL_ENTRY), bool((o[cap:] == CAN).all()), bool((i[written:] == CAN).all())


def check(ctx, s, idx, keep, rule=None, use_rule=False):
    want_out, want_io, want_s = F.filter_ref(s, idx, keep)
    sm, out, io, ok_out, ok_io = run(ctx, s, idx, rule=rule if use_rule else None, keep=None if use_rule else keep)
    for k, v in want_s.items():
        assert int(sm[k]) == v, (k, int(sm[k]), v)
    assert list(sm["reserved"]) == [0, 0, 0]
    assert np.array_equal(out, want_out)
    assert np.array_equal(io, want_io)
    assert ok_out and ok_io
    return out, io


def random_rule(rng):
    import hevcbitstream_amd as hbs
    pick = int(rng.integers(0, 5))
    types = [hbs.NALMASK_ALL, hbs.NALMASK_IRAP | hbs.NALMASK_PARAM_SETS, hbs.NALMASK_ALL & ~(hbs.NALMASK_SEI | (1 << 35) | (1 << 38)),
             int(rng.integers(0, 1 << 63)) | (int(rng.integers(0, 2)) << 63), hbs.NALMASK_VCL][pick]
    return dict(keep_types=types, max_temporal_id_plus1=int(rng.integers(0, 8)), max_layer_id=int(rng.choice([0, 5, 63])),
                keep_short=bool(rng.integers(0, 2)))


def test_random_streams_rules_and_masks(ctx, orc):
    rng = np.random.default_rng(2024)
    for it in range(60):
        size = int(rng.choice([1, 7, 100, 5000, 70000, 300000, 3 << 20]))
        mean = int(rng.choice([3, 20, 200, 3000, 100000]))
        if mean < 100:
            size = min(size, 200000)
        s = F.random_stream(rng, size, mean)
        idx, _, _ = orc.index_extract(s)
        r = random_rule(rng)
        check(ctx, s, idx, F.rule_keep(s, idx, **r), rule=ctx.nal_filter(**r), use_rule=True)
        check(ctx, s, idx, rng.random(len(idx)) < rng.random())


def test_keep_all_identity_and_rescan(ctx, orc):
    import torch
    rng = np.random.default_rng(5)
    for it in range(12):
        s = F.random_stream(rng, int(rng.choice([3000, 200000, 2 << 20])), int(rng.choice([10, 400, 9000])))
        idx, arena, _ = orc.index_extract(s)
        out, io = check(ctx, s, idx, np.ones(len(idx), bool), rule=ctx.nal_filter(), use_rule=True)
        assert np.array_equal(out, s[: int(idx["end"][-1])] if len(idx) else s[:0])
        # re-scan of a cut: the device's own scan of the output gives the output index, its arena the kept NALs' RBSP
        keep = rng.random(len(idx)) < 0.5
        out, io = check(ctx, s, idx, keep)
        got, arena2, gs = ctx.index_extract(torch.from_numpy(out.copy()).cuda() if len(out) else torch.zeros(0, dtype=torch.uint8, device="cuda"))
        if F.rescan_misses_last(out, io):
            assert np.array_equal(got, io[:-1])
            continue
        assert np.array_equal(got, io)
        want = [arena[int(e["rbsp_off"]): int(e["rbsp_off"]) + int(e["rbsp_len"])] for e in idx[keep]]
        assert np.array_equal(arena2, np.concatenate(want) if want else np.zeros(0, np.uint8))


def test_4k30_temporal_layers_rule_keep_and_reference_agree(ctx):
    import torch
    import hevcbitstream_amd as hbs
    from tests.hevc_synth import Synth, annexb
    g = Synth(3, rich=False)
    rng = np.random.RandomState(4)
    nals = []
    for pic in range(48):
        if pic % 16 == 0:
            nals += [g.vps(), g.sps_nal(3840, 2160, ctb_log2=6), g.pps_nal(force={"tiles": 0})]
        tid = 1 if pic % 4 == 0 else 2 if pic % 4 == 2 else 3           # hierarchical: three temporal sub-layers
        for sl in range(4):
            pay = rng.randint(0, 256, size=int(rng.randint(2000, 6000))).astype(np.uint8).tobytes()
            nt = 19 if pic % 16 == 0 else 1
            nals.append(g.slice_nal(nt, first=(sl == 0), payload=pay, address=sl * 510, tid=tid))
    s = np.frombuffer(annexb(nals), dtype=np.uint8).copy()
    d = torch.from_numpy(s).cuda()
    index, rbsp, summary, cap = ctx.alloc_outputs(len(s))
    ctx.index_extract_async(d, index, cap, rbsp, summary)
    n = int(ctx.read_summary(summary)["nal_count"])
    assert n == len(nals)
    idx = index[: n * 32].cpu().numpy().view(F.NAL_ENTRY).copy()
    parsed, _ = ctx.parse_headers(rbsp, index, n)
    t, layer, tid1, _ = F.header_fields(s, idx)
    assert np.array_equal(parsed["nal_unit_type"], t) and np.array_equal(parsed["nal_temporal_id_plus1"], tid1)
    for types, max_tid in ((hbs.NALMASK_ALL, 2), (hbs.NALMASK_ALL, 1), (hbs.NALMASK_IRAP | hbs.NALMASK_PARAM_SETS, 7)):
        keep = ((types >> parsed["nal_unit_type"].astype(np.uint64)) & 1).astype(bool) & (parsed["nal_temporal_id_plus1"] <= max_tid)
        assert 0 < keep.sum() < n
        assert np.array_equal(keep, F.rule_keep(s, idx, keep_types=types, max_temporal_id_plus1=max_tid))
        a = check(ctx, s, idx, keep, rule=ctx.nal_filter(types, max_tid), use_rule=True)
        b = check(ctx, s, idx, keep)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        out, io, sm = ctx.filter_annexb(d, idx, keep_types=types, max_temporal_id_plus1=max_tid)
        assert np.array_equal(out.cpu().numpy(), a[0]) and np.array_equal(io, a[1])


def test_exact_capacity_one_short_and_plan_only(ctx, orc):
    rng = np.random.default_rng(9)
    for it in range(8):
        s = F.random_stream(rng, int(rng.choice([1000, 100000, 1 << 20])), int(rng.choice([30, 2000])))
        idx, _, _ = orc.index_extract(s)
        keep = rng.random(len(idx)) < 0.6
        want_out, want_io, _ = F.filter_ref(s, idx, keep)
        if not len(want_out):
            continue
        sm, out, io, ok, ok_io = run(ctx, s, idx, keep=keep)
        assert int(sm["error"]) == 0 and np.array_equal(out, want_out) and ok and ok_io
        sm, out, io, ok, ok_io = run(ctx, s, idx, keep=keep, out_cap=len(want_out) - 1)
        assert int(sm["error"]) == F.E_CAPACITY and int(sm["stream_bytes"]) == len(want_out)
        assert (out == CAN).all() and ok and ok_io        # nothing written, output index included


def test_inconsistent_index_and_empty_index(ctx, orc):
    import torch
    rng = np.random.default_rng(13)
    idx = []
    while len(idx) <= 10:                                  # (a stream may stop early at an empty NAL)
        s = F.random_stream(rng, 50000, 300)
        idx, _, _ = orc.index_extract(s)
    bads = []
    a = idx.copy(); a["start"][5] = a["end"][5] + 1; bads.append(a)                 # start > end
    a = idx.copy(); a["end"][-1] = len(s) + 1; bads.append(a)                        # end > stream_bytes
    a = idx.copy(); a["start"][7] = a["end"][6] - 1; bads.append(a)                  # overlaps the NAL in front
    for a in bads:
        assert not F.consistent(a, len(s))
        for use_rule in (True, False):
            sm, out, io, ok, ok_io = run(ctx, s, a, rule=ctx.nal_filter() if use_rule else None,
                                         keep=None if use_rule else np.ones(len(a), bool), out_cap=len(s))
            assert int(sm["error"]) == F.E_ARG
            assert (out == CAN).all() and ok and ok_io
    e = np.zeros(0, dtype=F.NAL_ENTRY)
    sm, out, io, ok, ok_io = run(ctx, s, e, rule=ctx.nal_filter())
    assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == 0 and int(sm["nal_count"]) == 0 and int(sm["stop_reason"]) == 0
    assert ok
    sm, out, io, ok, _ = run(ctx, s, idx, keep=np.zeros(len(idx), bool), out_cap=0)
    assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == 0 and ok
    # exactly one of rule and keep
    summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    import hevcbitstream_amd as hbs
    with pytest.raises(hbs.HbsError):
        ctx.filter_annexb_async(dev(s), len(s), dev(idx), len(idx), None, None, summ)
    with pytest.raises(hbs.HbsError):
        ctx.filter_annexb_async(dev(s), len(s), dev(idx), len(idx), None, None, summ, rule=ctx.nal_filter(),
                                keep=dev(np.ones(len(idx), np.uint8)))


def test_dense_tiny_nals_every_other(ctx, orc):
    rng = np.random.default_rng(17)
    parts = []
    while sum(len(p) for p in parts) < 600000:
        n = int(rng.integers(1, 62))
        parts.append((b"\x00\x00\x00\x01" if rng.random() < 0.3 else b"\x00\x00\x01") + bytes(rng.integers(1, 256, size=n, dtype=np.uint8)))
    s = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    idx, _, _ = orc.index_extract(s)
    assert len(idx) > 15000
    keep = (np.arange(len(idx)) % 2) == 0
    check(ctx, s, idx, keep)
    check(ctx, s, idx, ~keep)
    check(ctx, s, idx, rng.random(len(idx)) < 0.1)


def units_per_tile(io):
    """(non-empty units that overlap each 64 KiB tile of the output, non-empty units) from an output index"""
    en = io["end"].astype(np.int64)
    u = np.concatenate([[0], en[:-1]])
    en, u = en[en > u], u[en > u]
    tiles = -(-int(en[-1]) // TILE)
    return [int(((u < (t + 1) * TILE) & (en > t * TILE)).sum()) for t in range(tiles)], len(en)


def test_table_that_does_not_fit_lds(ctx):
    """Payloads of 0-3 bytes behind 3- and 4-byte start codes: ~4.8 bytes a unit, ~13 600 units in a full output tile, so the
    copy reads the tile's table from memory.  The index is the constructed one (the oracle's walk stops at the first empty
    NAL; with payloads of 1-3 bytes it gives this index).  700 KB, not 300: a tenth of the NALs is then one full tile and a
    last tile of ~3.5 KB, ~700 units, that is staged in LDS -- at this density a tenth of 300 KB is one tile of ~6 000 units."""
    from tests.test_gpu_lenpref import made_stream
    rng = np.random.default_rng(41)
    n = 146000
    s, idx = made_stream(rng, rng.integers(0, 4, size=n))
    assert F.consistent(idx, len(s)) and len(s) > 700000
    for keep, dense in ((np.ones(n, bool), True), (np.arange(n) % 2 == 0, True), (rng.random(n) < 0.1, False)):
        want_out, want_io, _ = F.filter_ref(s, idx, keep)
        per_tile, units = units_per_tile(want_io)
        if dense:
            assert units > LDS_UNITS * (len(want_out) / TILE) and min(per_tile[:-1]) > LDS_UNITS
            check(ctx, s, idx, keep, rule=ctx.nal_filter(), use_rule=bool(keep.all()))
        else:
            assert min(per_tile) < LDS_UNITS < max(per_tile)
            check(ctx, s, idx, keep)


def test_stream_above_4gib(ctx):
    """a few NALs near 1 GiB among small ones: offsets above 4 GiB, units spread over many tiles.  Compared by re-scan (the
    device's index-only scan of the output against the reference index) plus slices of the output against the stream"""
    import torch
    rng = np.random.default_rng(23)
    sizes = []
    for k in range(4):
        sizes += [int(rng.integers(100, 20000)) for _ in range(int(rng.integers(200, 600)))]
        sizes.append((1 << 30) + int(rng.integers(-5000, 5000)))
    sizes += [int(rng.integers(100, 20000)) for _ in range(300)]
    lens = np.array(sizes, dtype=np.int64)
    sc = np.where(rng.random(len(lens)) < 0.3, 4, 3)
    total = int((lens + sc).sum())
    assert total > (4 << 30)
    d = torch.randint(1, 256, (total,), dtype=torch.uint8, device="cuda")          # no zero bytes: no start code but ours
    pos = np.concatenate([[0], np.cumsum(lens + sc)[:-1]])
    st = torch.from_numpy(pos).cuda()
    four = torch.from_numpy(sc == 4).cuda()
    d[st] = 0
    d[st + 1] = 0
    d[st + 2] = torch.where(four, 0, 1).to(torch.uint8)
    d[(st + 3)[four]] = 1
    idx, _, s0 = ctx.index_extract(d, index_cap=len(lens) + 16, want_rbsp=False)
    assert len(idx) == len(lens)
    assert np.array_equal(idx["start"].astype(np.int64), pos + sc)
    for keep in (np.ones(len(idx), bool), rng.random(len(idx)) < 0.5):
        out, io, sm = ctx.filter_annexb(d, idx, keep=keep)
        en = idx["end"].astype(np.int64)
        u = np.concatenate([[0], en[:-1]])
        kk = np.nonzero(keep)[0]
        ulen = en[kk] - u[kk]
        ooff = np.concatenate([[0], np.cumsum(ulen)[:-1]])
        assert int(sm["stream_bytes"]) == int(ulen.sum()) == out.numel() and int(sm["nal_count"]) == len(kk)
        assert np.array_equal(io["start"].astype(np.int64), ooff + idx["start"][kk].astype(np.int64) - u[kk])
        assert np.array_equal(io["end"].astype(np.int64), ooff + ulen)
        assert int(io["end"][-1]) > (1 << 32) or not keep.all()
        got, _, gs = ctx.index_extract(out, index_cap=len(kk) + 16, want_rbsp=False)
        assert np.array_equal(got["start"], io["start"]) and np.array_equal(got["end"], io["end"])
        assert np.array_equal(got["status"], io["status"])
        # slices: every unit's first and last 4 KiB, and 200 random windows inside units
        for j in range(len(kk)):
            a, b, k = int(ooff[j]), int(ooff[j] + ulen[j]), int(kk[j])
            w = min(4096, b - a)
            assert torch.equal(out[a:a + w], d[u[k]:u[k] + w]) and torch.equal(out[b - w:b], d[en[k] - w:en[k]])
        for _ in range(200):
            j = int(rng.integers(0, len(kk)))
            off = int(rng.integers(0, ulen[j]))
            w = min(int(rng.integers(1, 1 << 20)), int(ulen[j]) - off)
            assert torch.equal(out[ooff[j] + off: ooff[j] + off + w], d[u[kk[j]] + off: u[kk[j]] + off + w])
        del out
        torch.cuda.empty_cache()


def test_two_contexts_at_the_same_time(orc):
    import torch
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(29)
    jobs = []
    for k in range(2):
        s = F.random_stream(rng, 4 << 20, 3000)
        idx, _, _ = orc.index_extract(s)
        keep = rng.random(len(idx)) < 0.5
        jobs.append((s, idx, keep, F.filter_ref(s, idx, keep)))
    streams = [torch.cuda.Stream() for _ in jobs]
    ctxs, bufs = [], []
    for (s, idx, keep, want), st in zip(jobs, streams):
        with torch.cuda.stream(st):
            c = hbs.Context(0)
            d_s, d_i, d_k = dev(s), dev(idx), dev(keep.astype(np.uint8))
            out = torch.full((len(want[0]) + PAD,), CAN, dtype=torch.uint8, device="cuda")
            io = torch.empty(len(idx) * 32 + 32, dtype=torch.uint8, device="cuda")
            summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
            ctxs.append(c)
            bufs.append((d_s, d_i, d_k, out, io, summ))
    for r in range(3):
        for (s, idx, keep, want), st, c, (d_s, d_i, d_k, out, io, summ) in zip(jobs, streams, ctxs, bufs):
            with torch.cuda.stream(st):
                c.filter_annexb_async(d_s, len(s), d_i, len(idx), out, io, summ, keep=d_k, out_cap=len(want[0]))
    torch.cuda.synchronize()
    for (s, idx, keep, want), c, (d_s, d_i, d_k, out, io, summ) in zip(jobs, ctxs, bufs):
        o = out.cpu().numpy()
        assert np.array_equal(o[: len(want[0])], want[0]) and (o[len(want[0]):] == CAN).all()
        assert np.array_equal(io[: len(want[1]) * 32].cpu().numpy().view(F.NAL_ENTRY), want[1])
        c.close()


def test_timing_covers_the_call(ctx, orc):
    rng = np.random.default_rng(31)
    s = F.random_stream(rng, 1 << 20, 2000)
    idx, _, _ = orc.index_extract(s)
    ctx.enable_timing(True)
    try:
        run(ctx, s, idx, keep=np.ones(len(idx), bool))
        assert ctx.kernel_ms() > 0 and ctx.kernel_ms_back(1) > 0
        assert ctx.device_bytes() > 0
    finally:
        ctx.enable_timing(False)
