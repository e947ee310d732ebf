"""hbs_access_units / hbs_au_keep on the device, field by field against the sequential reference (tests/_au_ref.py):
fabricated records of every density, the carry, real streams through hbs_index_parse_compact, a GOP cut through
hbs_filter_annexb, exact capacity with canaries, plan only, errors, two contexts, the timing events."""
import numpy as np
import pytest

from tests import _au_ref as R

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
SLOT = 8192          # bytes between the fabricated SPS structs

# Half of the draws are weighted towards the types streams are made of (they keep the densities the cases ask for), the other
# half is uniform over the whole range of the side -- every type 0..63 and -1 -- with a few raw values the call clamps to -1.
VCL_TYPES = np.array([0, 1, 1, 1, 2, 6, 8, 9, 16, 17, 19, 20, 21, 22, 25, 31])
OTHER_TYPES = np.array([32, 33, 33, 34, 35, 36, 37, 38, 39, 40, 41, 45, 48, 55, 60, 63, -1])
ALL_VCL = np.arange(0, 32)
RAW = [-1, -1, -7, 64, 200, -2147483648, 2147483647]
ALL_OTHER = np.array(list(range(32, 64)) + RAW)
CAND_OTHER = set(R.CAND_TYPES)
QUIET_TYPES = np.array([t for t in ALL_OTHER.tolist() if t not in CAND_OTHER] + [40] * 8)      # none of them may begin an AU


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


def sps_off(ctx):
    off = int(ctx.lib.hbs_au_sps_poc_offset())
    assert off + 4 <= SLOT
    return off


def fabricate(rng, n, p_vcl, p_first, quiet=False, poc_bits=None, off=0):
    """random records built directly: any type, layer, temporal id, flags, lsb, rc; SPS NALs with and without a struct"""
    parsed = np.zeros(n, dtype=R.PARSED)
    compact = np.zeros(n, dtype=R.COMPACT)
    index = np.zeros(n, dtype=R.NAL_ENTRY)
    vcl = rng.random(n) < p_vcl
    wide = rng.random(n) < 0.5

    def pick(a):
        return a[rng.integers(0, len(a), n)]
    parsed["nal_unit_type"] = np.where(vcl, np.where(wide, pick(ALL_VCL), pick(VCL_TYPES)),
                                       pick(QUIET_TYPES) if quiet else np.where(wide, pick(ALL_OTHER), pick(OTHER_TYPES)))
    parsed["nal_layer_id"] = np.where(rng.random(n) < 0.05, rng.integers(1, 64, n), 0)
    parsed["nal_temporal_id_plus1"] = np.array([1, 1, 1, 2, 3, 0, 7])[rng.integers(0, 7, n)]
    parsed["rc"] = np.where(rng.random(n) < 0.1, -1, rng.integers(2, 900, n))
    parsed["slice_data_size"] = rng.integers(-5, 5000, n)
    parsed["slice_data_off"] = rng.integers(0, 100, n)
    bits = poc_bits if poc_bits is not None else int(rng.choice([4, 8, 16]))
    compact["first_slice_segment_in_pic_flag"] = rng.random(n) < p_first
    compact["dependent_slice_segment_flag"] = rng.random(n) < 0.2
    compact["slice_type"] = rng.integers(-1, 5, n)
    compact["slice_pic_order_cnt_lsb"] = rng.integers(0, 1 << bits, n)
    compact["slice_qp_delta"] = rng.integers(-20, 20, n)
    end = np.cumsum(rng.integers(4, 200, n, dtype=np.int64)).astype(np.uint64)
    index["end"] = end
    index["start"] = end - np.uint64(1)
    is_sps = parsed["nal_unit_type"] == 33
    with_slot = is_sps & (rng.random(n) < 0.7)
    slots = np.flatnonzero(with_slot)
    if len(slots) > 512:                      # keep the struct arena small: 512 of them, anywhere in the batch
        chosen = np.sort(rng.choice(slots, 512, replace=False))
        with_slot[:] = False
        with_slot[chosen] = True
        slots = chosen
    parsed["struct_off"] = R.NO_SLOT
    parsed["struct_off"][slots] = np.arange(len(slots), dtype=np.uint64) * SLOT
    structs = rng.integers(0, 256, SLOT * max(len(slots), 1), dtype=np.uint8)
    vals = rng.integers(-3, 16, len(slots)).astype("<i4")
    for j in range(len(slots)):
        structs[j * SLOT + off: j * SLOT + off + 4] = np.frombuffer(vals[j].tobytes(), dtype=np.uint8)
    return index, parsed, compact, structs


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(64, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def run(ctx, recs, carry=None, au_cap=None, want_nal_au=True, want_structs=True):
    """plan, then the call into buffers of exactly au_cap records (default: the planned count) with canaries behind them"""
    import torch
    import hevcbitstream_amd as hbs
    index, parsed, compact, structs = recs
    n = len(parsed)
    d = [dev(index), dev(parsed), dev(compact), dev(structs) if want_structs else None]
    summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert ctx.access_units_async(d[0], d[1], d[2], d[3], n, None, 0, None, None, summ, carry) == 0
    plan = ctx.read_summary(summ).copy()
    cap = int(plan["nal_count"]) if au_cap is None else au_cap
    au = torch.full((cap * 64 + PAD,), CAN, dtype=torch.uint8, device="cuda")
    nal_au = torch.full((n * 4 + PAD,), CAN, dtype=torch.uint8, device="cuda")
    carry_out = torch.full((16 + PAD,), CAN, dtype=torch.uint8, device="cuda")
    summ.fill_(0xEE)
    assert ctx.access_units_async(d[0], d[1], d[2], d[3], n, au, cap, nal_au if want_nal_au else None, carry_out, summ, carry) == 0
    sm = ctx.read_summary(summ).copy()
    for f in ("nal_count", "nal_found", "stream_bytes", "rbsp_bytes", "stop_reason"):
        assert int(plan[f]) == int(sm[f]), f
    assert list(plan["reserved"]) == list(sm["reserved"]) and int(plan["error"]) == 0
    return sm, au.cpu().numpy(), nal_au.cpu().numpy(), carry_out.cpu().numpy(), d


def same_records(got, want):
    assert len(got) == len(want)
    for f in want.dtype.names:
        if not np.array_equal(got[f], want[f]):
            bad = int(np.flatnonzero(got[f] != want[f])[0])
            raise AssertionError("%s differs first at AU %d: got %r want %r\n%r\n%r" % (f, bad, got[f][bad], want[f][bad], got[bad], want[bad]))


def check(ctx, recs, carry=None):
    import hevcbitstream_amd as hbs
    off = sps_off(ctx)
    want_au, want_nal_au, want_carry, want_s = R.access_units(recs[0], recs[1], recs[2], recs[3], off, carry)
    sm, au, nal_au, carry_out, d = run(ctx, recs, carry)
    n, aus = len(recs[1]), len(want_au)
    assert int(sm["error"]) == 0
    assert (int(sm["nal_count"]), int(sm["nal_found"]), int(sm["reserved"][0]), int(sm["reserved"][1]), int(sm["stream_bytes"])) == \
        (want_s["nal_count"], want_s["nal_found"], want_s["pictures"], want_s["cvs_starts"], want_s["stream_bytes"])
    assert int(sm["rbsp_bytes"]) == 0 and int(sm["stop_reason"]) == 0 and int(sm["reserved"][2]) == 0
    same_records(au[: aus * 64].view(hbs.ACCESS_UNIT), want_au)
    assert np.array_equal(nal_au[: n * 4].view(np.uint32), want_nal_au)
    got_carry = carry_out[:16].view(hbs.AU_CARRY)
    assert got_carry.tolist() == want_carry.tolist(), (got_carry, want_carry)
    assert (au[aus * 64:] == CAN).all() and (nal_au[n * 4:] == CAN).all() and (carry_out[16:] == CAN).all()
    return want_au, want_nal_au, want_carry, d


DENSITIES = [(1.0, 1.0, False), (0.9, 0.3, False), (0.5, 0.5, False), (0.3, 0.05, False), (0.05, 0.5, False), (0.02, 0.001, True),
             (0.3, 0.0003, True), (0.0, 0.0, False), (0.0, 0.0, True), (1.0, 0.0, False)]


def test_fabricated_records(ctx):
    rng = np.random.default_rng(815)
    off = sps_off(ctx)
    sizes = [0, 1, 2, 63, 64, 255, 256, 257, 2047, 2048, 2049, 4096, 10000, 70000, 300001]
    it = 0
    for n in sizes:
        for p_vcl, p_first, quiet in (DENSITIES if n <= 70000 else DENSITIES[1::3]):
            check(ctx, fabricate(rng, n, p_vcl, p_first, quiet, off=off))
            it += 1
    assert it > 100


def test_access_units_longer_than_a_workgroup_and_a_large_batch(ctx):
    rng = np.random.default_rng(816)
    off = sps_off(ctx)
    # AUs of thousands of NALs: a picture, then nothing that may begin an AU for a long while; several workgroups per AU
    recs = fabricate(rng, 200000, 0.3, 0.0002, quiet=True, off=off)
    want_au, _, _, _ = check(ctx, recs)
    assert int(want_au["nal_count"].max()) > 3 * 2048
    # the picture NAL lies workgroups behind the NAL that began its AU
    n = 30000
    recs = fabricate(rng, n, 0.0, 0.0, quiet=True, off=off)
    recs[1]["nal_layer_id"] = 0
    recs[1]["nal_unit_type"][[0, 9000]] = 35
    recs[1]["nal_unit_type"][[7000, 7001, 20000]] = [1, 1, 21]
    recs[1]["nal_temporal_id_plus1"][[7000, 7001, 20000]] = 1
    recs[2]["first_slice_segment_in_pic_flag"][[7000, 20000]] = 1
    want_au, _, _, _ = check(ctx, recs)
    assert want_au["first_vcl"].tolist() == [7000, 11000]
    # a few million NALs, a picture about every 8
    check(ctx, fabricate(rng, 3000000, 0.6, 0.2, off=off))


def test_more_workgroups_than_one_step_of_the_aggregate_scan(ctx):
    """The scan of the per-workgroup aggregates takes 2048 of them a step and carries its state to the next step; 2048
    workgroups are 4 194 304 NALs.  Batches above that, field by field: every prefix (last VCL / CAND / EOS / SPS / start /
    picture / anchor, the counts, the msb sum with its resets) crosses the step."""
    rng = np.random.default_rng(820)
    off = sps_off(ctx)
    n = 5000000
    recs = fabricate(rng, n, 0.6, 0.2, off=off)
    want_au, _, _, _ = check(ctx, recs)
    behind = want_au[want_au["first_nal"] >= 2048 * 2048]
    assert len(behind) > 10000 and int((behind["flags"] & R.CVS_START != 0).sum()) > 100
    assert int((behind["flags"] & R.END_OF_SEQ != 0).sum()) > 100 and int(recs[1]["struct_off"][2048 * 2048:].min()) != R.NO_SLOT
    # few, long AUs, no SPS at all: the prefixes that cross the step come from far in front
    recs = fabricate(rng, 4500000, 0.02, 0.0001, quiet=True, off=off)
    want_au, _, _, _ = check(ctx, recs)
    assert ((want_au["first_nal"] < 2048 * 2048) & (want_au["first_nal"] + want_au["nal_count"] > 2048 * 2048)).any()


def test_carry_two_calls_give_the_records_of_one(ctx):
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(817)
    off = sps_off(ctx)
    for it in range(12):
        n = int(rng.choice([300, 5000, 40000]))
        p_vcl, p_first, quiet = DENSITIES[int(rng.integers(0, 7))]
        recs = fabricate(rng, n, p_vcl, p_first, quiet, poc_bits=4, off=off)
        recs[1]["struct_off"] = R.NO_SLOT          # the carry holds no SPS: Max stays 16 in both halves
        whole, nal_au, carry_whole, _ = check(ctx, recs)
        if len(whole) < 2:
            continue
        j = int(rng.integers(1, len(whole)))
        cut = int(whole["first_nal"][j])
        head = tuple(r[:cut] for r in recs[:3]) + (recs[3],)
        tail = tuple(r[cut:] for r in recs[:3]) + (recs[3],)
        a, _, carry, _ = check(ctx, head)
        b, _, carry2, _ = check(ctx, tail, carry)
        b = b.copy()
        b["first_nal"] += np.uint64(cut)
        b["unit_begin"][0] = a["unit_end"][-1]      # NAL 0 of a call has nothing in front: its unit begins at 0
        both = np.concatenate([a, b])
        # the EOS rule of a CRA looks at "a picture in front": with the carry that is the same question
        same_records(both, whole)
        assert carry2.tolist() == carry_whole.tolist()


def hier_stream(seed, periods=6, gops=3, slices=3):
    """AUD, SEI, three temporal layers, several slices per picture, IDR and CRA periods, known poc_lsb.
    -> (stream bytes, n_nals, per picture (nal type, temporal id + 1, POC))"""
    from tests.hevc_synth import Synth, BitWriter, annexb
    g = Synth(seed, rich=False)
    rng = np.random.RandomState(seed)
    nals, pics = [], []

    def aud():
        w = BitWriter()
        w.u(3, 2)
        w.trailing()
        return g.nal(35, w)

    def sei(t):
        w = BitWriter()
        w.u(8, 5); w.u(8, 2); w.u(8, 0x55); w.u(8, 0xAA)
        w.trailing()
        return g.nal(t, w)

    def picture(t, tid1, poc):
        nals.append(aud())
        if rng.rand() < 0.5:
            nals.append(sei(39))
        for sl in range(slices):
            payload = rng.randint(0, 256, size=int(rng.randint(20, 300))).astype(np.uint8).tobytes()
            nals.append(g.slice_nal(t, first=(sl == 0), payload=payload, address=sl * 100, tid=tid1, poc_lsb=poc))
        if rng.rand() < 0.3:
            nals.append(sei(40))
        pics.append((t, tid1, poc))

    poc = 0
    for period in range(periods):
        idr = period % 2 == 0
        nals.append(g.vps())
        nals.append(g.sps_nal(3840, 2160, ctb_log2=6))
        nals.append(g.pps_nal(force={"tiles": 0}))
        bits = g.sps["poc_bits"]
        if idr:
            poc = 0
            picture(19, 1, 0)
        else:
            poc += 4
            picture(21, 1, poc)
        for _ in range(gops):
            base = poc
            for o, tid1, t in ((4, 1, 1), (2, 2, 1), (1, 3, 0), (3, 3, 0)):
                picture(t, tid1, base + o)
            poc = base + 4
        assert (1 << bits) >= 16
    return annexb(nals), len(nals), pics


def parse_stream(ctx, stream, n):
    import torch
    from hevcbitstream_amd.api import COMPACT, PARSED, SUMMARY
    d = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda() if not hasattr(stream, "numel") else stream
    cap = n + 8
    index = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    parsed = torch.zeros(cap * PARSED.itemsize, dtype=torch.uint8, device="cuda")
    cc = torch.zeros(cap * COMPACT.itemsize, dtype=torch.uint8, device="cuda")
    structs = torch.zeros(8 << 20, dtype=torch.uint8, device="cuda")
    ss, ps = torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device="cuda"), torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device="cuda")
    got = ctx.index_parse_compact_async(d, index, cap, parsed, cc, structs, ss, ps)
    assert int(ctx.read_summary(ps)["error"]) == 0
    return d, got, index, parsed, cc, structs


def host_records(got, index, parsed, cc, structs):
    return (index[: got * 32].cpu().numpy().view(R.NAL_ENTRY), parsed[: got * 32].cpu().numpy().view(R.PARSED),
            cc[: got * 64].cpu().numpy().view(R.COMPACT), structs.cpu().numpy())


def test_end_to_end_streams(ctx):
    from tests.hevc_synth import stream_4k30
    stream, n = stream_4k30(9, n_pictures=120, slices_per_picture=8, idr_every=30, payload_bytes=(300, 900))
    d, got, index, parsed, cc, structs = parse_stream(ctx, stream, n)
    assert got == n
    recs = host_records(got, index, parsed, cc, structs)
    au, nal_au, s, carry = ctx.access_units(index, parsed, cc, structs, got)
    want_au, want_nal_au, want_carry, want_s = R.access_units(*recs, sps_off(ctx))
    same_records(au, want_au)
    assert np.array_equal(nal_au, want_nal_au) and carry.tolist() == want_carry.tolist()
    assert len(au) == 120 and int(s["reserved"][0]) == 120 and int(s["reserved"][1]) == 4
    assert au["vcl_count"].tolist() == [8] * 120 and au["nal_count"].tolist() == [11 if i % 30 == 0 else 8 for i in range(120)]
    assert int(au["unit_begin"][0]) == 0 and np.array_equal(au["unit_begin"][1:], au["unit_end"][:-1])
    assert int(au["unit_end"][-1]) == int(recs[0]["end"][-1]) == int(s["stream_bytes"])

    stream, n, pics = hier_stream(21)
    d, got, index, parsed, cc, structs = parse_stream(ctx, stream, n)
    assert got == n
    recs = host_records(got, index, parsed, cc, structs)
    au, nal_au, s, carry = ctx.access_units(index, parsed, cc, structs, got)
    want_au, want_nal_au, _, _ = R.access_units(*recs, sps_off(ctx))
    same_records(au, want_au)
    assert len(au) == len(pics)
    assert au["nal_unit_type"].tolist() == [p[0] for p in pics]
    assert au["temporal_id_plus1"].tolist() == [p[1] for p in pics]
    assert au["pic_order_cnt"].tolist() == [p[2] for p in pics]
    assert au["vcl_count"].tolist() == [3] * len(pics)
    assert int(au["unit_begin"][0]) == 0 and np.array_equal(au["unit_begin"][1:], au["unit_end"][:-1])
    assert int(au["unit_end"][-1]) == int(recs[0]["end"][-1])


def test_gop_cut_through_the_filter(ctx):
    import torch
    import hevcbitstream_amd as hbs
    stream, n, pics = hier_stream(33, periods=7)
    d, got, index, parsed, cc, structs = parse_stream(ctx, stream, n)
    recs = host_records(got, index, parsed, cc, structs)
    au, nal_au, s, _ = ctx.access_units(index, parsed, cc, structs, got)
    idr = [j for j in range(len(au)) if int(au["flags"][j]) & hbs.AU_IDR]
    assert len(idr) >= 3
    first_au, count = idr[1], idr[2] - idr[1]
    d_nal_au = torch.from_numpy(nal_au.view(np.int32).copy()).cuda()
    keep = ctx.au_keep(d_nal_au, parsed, got, first_au, count, param_sets=True)
    want_keep = R.au_keep(nal_au, recs[1], first_au, count, True)
    assert np.array_equal(keep.cpu().numpy(), want_keep)
    # the range's own NALs and the three sets in force in front of it (those of the period before)
    assert int(want_keep.sum()) == int(au["nal_count"][first_au: first_au + count].sum()) + 3
    out, io, fs = ctx.filter_annexb(d, index[: got * 32], keep=keep)
    kept = int(fs["nal_count"])
    d2, got2, index2, parsed2, cc2, structs2 = parse_stream(ctx, out.contiguous(), kept)
    assert got2 == kept
    au2, _, s2, _ = ctx.access_units(index2, parsed2, cc2, structs2, got2)
    sel = au[first_au: first_au + count]
    assert len(au2) == count
    for f in ("nal_unit_type", "temporal_id_plus1", "pic_order_cnt", "vcl_count", "slice_types", "poc_lsb"):
        assert np.array_equal(au2[f], sel[f]), f
    assert np.array_equal(au2["flags"] & ~np.uint32(hbs.AU_PARAM_SETS), sel["flags"] & ~np.uint32(hbs.AU_PARAM_SETS))
    # a range that begins at a CRA: the parameter sets in front of it come along
    cra = [j for j in range(len(au)) if int(au["nal_unit_type"][j]) == 21][1]
    for fa, cnt, sets in ((cra + 1, 5, True), (cra + 1, 5, False), (len(au) - 2, 50, True), (len(au), 3, True), (3, 0, True)):
        keep = ctx.au_keep(d_nal_au, parsed, got, fa, cnt, param_sets=sets)
        assert np.array_equal(keep.cpu().numpy(), R.au_keep(nal_au, recs[1], fa, cnt, sets)), (fa, cnt, sets)


def test_capacity_plan_and_errors(ctx):
    import torch
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(818)
    recs = fabricate(rng, 9000, 0.6, 0.3, off=sps_off(ctx))
    want_au, _, _, want_s = R.access_units(*recs, sps_off(ctx))
    aus = len(want_au)
    check(ctx, recs)                                                   # exact capacity, canaries behind both outputs
    sm, au, nal_au, carry_out, d = run(ctx, recs, au_cap=aus - 1)      # one record short
    assert int(sm["error"]) == -4 and int(sm["nal_count"]) == aus and int(sm["reserved"][0]) == want_s["pictures"]
    assert int(sm["reserved"][1]) == want_s["cvs_starts"]
    assert (au == CAN).all() and (nal_au == CAN).all() and (carry_out == CAN).all()
    sm, au, nal_au, carry_out, d = run(ctx, recs, want_nal_au=False)   # d_nal_au is optional
    assert int(sm["error"]) == 0 and (nal_au == CAN).all()
    same_records(au[: aus * 64].view(hbs.ACCESS_UNIT), want_au)
    # d_structs = NULL: every SPS counts as "without a struct", Max is 16 throughout
    want_plain, _, _, _ = R.access_units(recs[0], recs[1], recs[2], None, sps_off(ctx))
    sm, au, nal_au, carry_out, d0 = run(ctx, recs, want_structs=False)
    assert int(sm["error"]) == 0
    same_records(au[: aus * 64].view(hbs.ACCESS_UNIT), want_plain)
    assert not np.array_equal(want_plain["pic_order_cnt"], want_au["pic_order_cnt"])
    # n_nals = 0: valid; the carry passes through
    c = np.zeros(1, dtype=hbs.AU_CARRY)
    c["flags"], c["anchor_poc_lsb"], c["anchor_poc_msb"] = 7, 5, -32
    empty = tuple(r[:0] for r in recs[:3]) + (recs[3],)
    _, _, carry, _ = check(ctx, empty, c)
    assert carry.tolist() == c.tolist()
    # n_nals just past 2^32 - 1: rejected before anything is touched
    summ = torch.full((64,), CAN, dtype=torch.uint8, device="cuda")
    au_t = torch.full((64,), CAN, dtype=torch.uint8, device="cuda")
    assert ctx.access_units_async(d[0], d[1], d[2], d[3], 1 << 32, au_t, 1, None, None, summ) == -3
    torch.cuda.synchronize()
    assert (summ.cpu().numpy() == CAN).all() and (au_t.cpu().numpy() == CAN).all()
    assert ctx.access_units_async(d[0], d[1][8:], d[2], d[3], 10, au_t, 1, None, None, summ) == -3       # misaligned records
    assert ctx.access_units_async(d[0], d[1], d[2], d[3], (1 << 32) - 1, None, 0, None, None, None) == -3  # no summary


def test_two_contexts_and_timing(ctx):
    import threading
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(819)
    off = sps_off(ctx)
    other = hbs.Context(0)
    jobs = [(ctx, [fabricate(rng, 50000, 0.5, 0.3, off=off) for _ in range(3)]), (other, [fabricate(rng, 30000, 0.2, 0.01, True, off=off) for _ in range(3)])]
    errors = []

    def work(c, batches):
        try:
            for _ in range(3):
                for recs in batches:
                    check(c, recs)
        except BaseException as e:          # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    other.close()
    assert not errors, errors
    # the library's events lie around ALL of the call's launches: events of the stream recorded right in front of and behind
    # the call enclose them and nothing else, so the two durations differ by the cost of recording events only -- far below a
    # fifth of a call over three million NALs, whose largest single launch is well under half of it
    import torch
    recs = fabricate(rng, 3000000, 0.6, 0.2, off=off)
    sm, _, _, _, d = run(ctx, recs)
    aus = int(sm["nal_count"])
    au = torch.empty(aus * 64, dtype=torch.uint8, device="cuda")
    nal_au = torch.empty(len(recs[1]) * 4, dtype=torch.uint8, device="cuda")
    summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ctx.enable_timing(True)
    try:
        pairs = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert ctx.access_units_async(d[0], d[1], d[2], d[3], len(recs[1]), au, aus, nal_au, None, summ) == 0
            e1.record()
            torch.cuda.synchronize()
            pairs.append((ctx.kernel_ms(), e0.elapsed_time(e1)))
        inner, outer = sorted(pairs)[len(pairs) // 2]
        print("hbs_ctx_kernel_ms %.4f ms, stream events around the call %.4f ms" % (inner, outer))
        assert 0.0 < inner <= outer * 1.02 + 0.005
        assert inner >= 0.8 * outer
    finally:
        ctx.enable_timing(False)
