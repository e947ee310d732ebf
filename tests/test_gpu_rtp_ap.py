"""hbs_rtp_pack with HBS_RTP_AGGREGATE on the GPU against the plain loop of tests/_rtp_ap_ref.py: every output byte, both tables
and the summary, into outputs of exactly the planned capacity with canaries behind them (the helpers of tests/test_gpu_rtp.py);
then the way back through hbs_rtp_unpack."""
import numpy as np
import pytest

from tests import _rtp_ref as R
from tests import _rtp_ap_ref as A
from tests import test_gpu_rtp as T
from tests._rtp_ref import random_case

pytestmark = pytest.mark.gpu
ctx = T.ctx
W = A.AP_SPAN
AGG = A.AGGREGATE


def run(ctx, stream, index, nal_au, n_aus, pts, prm):
    """the plan, then a run into canary-backed outputs of exactly the planned size, everything against the restatement
    -> (out, the restatement's results, summary, device inputs)"""
    want = A.pack(stream, index, nal_au, n_aus, pts, prm)
    assert want[3]["error"] == 0
    return T.run(ctx, stream, index, nal_au, n_aus, pts, prm, want=want)


def aps(want):
    return want[3]["reserved"][2] >> 32


def lay(sizes, headers=None, gap=0, seed=0):
    """NALs of these sizes, `gap` bytes apart -> (stream, index)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes[:-1] + gap)])
    stream = rng.integers(0, 256, size=int(starts[-1] + sizes[-1]), dtype=np.uint8)
    if headers is None:
        stream[starts] = (rng.integers(0, 48, size=len(sizes)) << 1 | rng.integers(0, 2, size=len(sizes)) |
                          rng.integers(0, 2, size=len(sizes)) << 7).astype(np.uint8)
    else:
        stream[starts], stream[starts + 1] = [h[0] for h in headers], [h[1] for h in headers]
    return stream, R.entries(starts, starts + sizes)


def test_the_flag_is_accepted_by_a_plan_call(ctx):
    """fails on a library without the feature: flags = 4 is refused there"""
    stream, index = lay([3, 2, 5])
    d = T.put(stream, index, None, 0, None, R.params(max_payload=100, flags=AGG))
    s = T.call(ctx, d, None, None, None)
    assert int(s["error"]) == 0 and int(s["nal_count"]) == 1 and int(s["reserved"][2]) == 1 << 32


@pytest.mark.parametrize("framing", (0, 2))
@pytest.mark.parametrize("mp", (19, 100, 1188))
def test_random_parity(ctx, mp, framing):
    rng = np.random.default_rng(100 * framing + mp)
    seen = 0
    for with_aus in (True, False):
        for with_pts in (True, False):
            for open_end in (0, R.OPEN_END):
                prm = R.params(max_payload=mp, framing=framing, flags=AGG | open_end, seq=65535 - int(rng.integers(0, 20)),
                               ts_base=0xFFFFFF00, ts_step=3003)
                stream, index, nal_au, n_aus, pts = random_case(rng, 2 * W + 77, max_nal=900, aus=with_aus, times=with_pts)
                _, want, s, _ = run(ctx, stream, index, nal_au, n_aus, pts, prm)
                seen += aps(want)
    assert seen > 0 or mp == 19


def test_edges_of_the_sum(ctx):
    """a group whose payload is exactly mp and one byte more; mp = 10 with 2-byte NALs and mp = 9; L = mp, mp + 1 and mp - 4 between
    small NALs"""
    for framing in (0, 2):
        stream, index = lay([3, 2, 5, 3, 2, 5], gap=1)
        for mp, packets in ((18, 2), (17, 3)):                              # (17: [3 2] [5 3] [2 5])
            _, want, _, _ = run(ctx, stream, index, None, 0, None, R.params(max_payload=mp, framing=framing, flags=AGG))
            assert want[3]["nal_count"] == packets
        stream, index = lay([2] * 9)
        _, want, _, _ = run(ctx, stream, index, None, 0, None, R.params(max_payload=10, framing=framing, flags=AGG))
        assert aps(want) == 4 and want[3]["nal_count"] == 5
        out9, want9, _, _ = run(ctx, stream, index, None, 0, None, R.params(max_payload=9, framing=framing, flags=AGG))
        plain = R.pack(stream, index, None, 0, None, R.params(max_payload=9, framing=framing))
        assert aps(want9) == 0 and np.array_equal(want9[0], plain[0]) and np.array_equal(want9[1], plain[1])
        for mp in (40, 1188):
            stream, index = lay([2, mp, 2, 2, mp + 1, 2, mp - 4, 2, 3], gap=3)
            _, want, _, _ = run(ctx, stream, index, None, 0, None, R.params(max_payload=mp, framing=framing, flags=AGG))
            assert want[2].tolist() == [0, 1, 2, 2, 3, 5, 6, 7, 7, 8] and want[3]["reserved"][2] == (2 << 32 | 1)


@pytest.mark.parametrize("with_aus", (True, False))
def test_the_cut_at_256(ctx, with_aus):
    """600 NALs of 2..6 bytes in one AU at the largest max_payload: packets break at NAL 256 and 512 and nowhere else, and the
    call on index[:256] and then on index[256:], the seq carried over, writes the same bytes"""
    rng = np.random.default_rng(7)
    stream, index = lay(rng.integers(2, 7, size=600), gap=1, seed=8)
    nal_au = np.full(600, 41, dtype=np.uint32) if with_aus else None
    prm = R.params(max_payload=65523, framing=2, flags=AGG, seq=65535, ts_base=9)
    whole, want, s, _ = run(ctx, stream, index, nal_au, 1, None, prm)
    assert want[2].tolist() == [0] * 256 + [1] * 256 + [2] * 88 + [3] and aps(want) == 3
    first, _, s1, _ = run(ctx, stream, index[:256], None if nal_au is None else nal_au[:256], 1, None, dict(prm, flags=AGG | R.OPEN_END))
    second, _, _, _ = run(ctx, stream, index[256:], None if nal_au is None else nal_au[256:], 1, None,
                          dict(prm, seq=(prm["seq"] + int(s1["reserved"][1])) & 0xFFFF))
    assert np.array_equal(np.concatenate([first.cpu().numpy(), second.cpu().numpy()]), whole.cpu().numpy())


def test_access_units(ctx):
    """AUs of one NAL; an AU boundary inside a would-be group; the marker on an AP; OPEN_END when the last group is an AP"""
    stream, index = lay([5, 4, 3, 6, 2, 7, 3, 3], gap=2, seed=3)
    pts = np.arange(8, dtype=np.uint64) * np.uint64(3003)
    for framing in (0, 2):
        prm = R.params(max_payload=100, framing=framing, flags=AGG, ts_base=77)
        _, want, _, _ = run(ctx, stream, index, np.arange(8, dtype=np.uint32) + 5, 8, pts, prm)
        assert aps(want) == 0 and want[3]["nal_count"] == 8
        nal_au = np.array([3, 3, 3, 4, 4, 5, 6, 6], dtype=np.uint32)
        for flags in (AGG, AGG | R.OPEN_END):
            out, want, _, _ = run(ctx, stream, index, nal_au, 4, pts, dict(prm, flags=flags))
            assert want[2].tolist() == [0, 0, 0, 1, 1, 2, 3, 3, 4]
            offs = A.packet_offsets(want[1], want[2], prm)
            markers = [int(out[int(o) + framing + 1]) >> 7 for o in offs[:-1]]
            assert markers == [1, 1, 1, 0 if flags & R.OPEN_END else 1]


def test_payload_hdr(ctx):
    """units with differing F bits, layer ids (values of 32 and more among them) and TIDs"""
    rng = np.random.default_rng(4)
    headers = [(int(t) << 1 | int(f) << 7 | int(layer) >> 5, (int(layer) & 31) << 3 | int(tid))
               for t, f, layer, tid in zip(rng.integers(0, 48, 120), rng.random(120) < 0.2, rng.integers(0, 64, 120), rng.integers(0, 8, 120))]
    stream, index = lay(rng.integers(2, 30, size=120), headers=headers, seed=5)
    nal_au = (np.arange(120) // 3).astype(np.uint32)
    out, want, _, _ = run(ctx, stream, index, nal_au, 40, None, R.params(max_payload=200, flags=AGG, ts_step=1))
    assert aps(want) == 40
    offs = A.packet_offsets(want[1], want[2], R.params(max_payload=200))
    o = out.cpu().numpy()
    hdrs = {(int(o[int(p) + 12]), int(o[int(p) + 13])) for p in offs[:-1]}
    assert len(hdrs) > 20 and any(h[0] & 0x80 for h in hdrs) and any(h[0] & 1 for h in hdrs) and any(h[1] & 7 for h in hdrs)


def test_aps_across_tile_borders(ctx):
    """about 150 KiB of output from NALs of about 100 bytes: aggregation packets straddle the 64 KiB borders of the copy's tiles"""
    rng = np.random.default_rng(6)
    stream, index, nal_au, n_aus, pts = random_case(rng, 1450, max_nal=200, min_nal=20)
    for framing in (0, 2):
        _, want, _, _ = run(ctx, stream, index, nal_au, n_aus, pts, R.params(max_payload=1188, framing=framing, flags=AGG, seq=65000))
        assert want[3]["stream_bytes"] > 2 * T.TILE + 4096 and aps(want) > 100
        for border in (T.TILE, 2 * T.TILE):                                # a NAL's share of the output lies across the border
            k = int(np.searchsorted(want[1], border, side="right")) - 1
            assert want[1][k] < border < want[1][k + 1]


def test_more_nals_in_a_tile_than_lds_holds(ctx):
    """20 000 NALs of 2..6 bytes: a tile holds more than the 512 NALs the copy stages in LDS, and a 16-byte chunk spans up to five
    NALs"""
    rng = np.random.default_rng(9)
    stream, index, nal_au, n_aus, pts = random_case(rng, 20000, max_nal=7)
    _, want, _, _ = run(ctx, stream, index, nal_au, n_aus, pts, R.params(max_payload=1188, framing=2, flags=AGG, seq=65530))
    assert T.TILE // 9 > T.LDS_NALS and aps(want) > 2000
    assert (np.diff(want[1].astype(np.int64))[:-1] == 4).sum() > 1000                          # units of four output bytes
    stream, index = lay(np.full(20000, 2), seed=10)
    _, want, _, _ = run(ctx, stream, index, None, 0, None, R.params(max_payload=65523, flags=AGG))
    assert aps(want) == 79 and want[3]["nal_count"] == 79


def test_contract(ctx):
    """capacity one byte short and a bad NAL inside a would-be group: the error, the outputs untouched (the plan-only call and the
    canaries behind an output of exactly the total are part of every run above)"""
    rng = np.random.default_rng(11)
    prm = R.params(max_payload=300, framing=2, flags=AGG)
    stream, index, nal_au, n_aus, pts = random_case(rng, 2 * W + 9, max_nal=60)
    want = A.pack(stream, index, nal_au, n_aus, pts, prm)
    need, n = want[3]["stream_bytes"], len(index)
    assert aps(want) > 50
    d = T.put(stream, index, nal_au, n_aus, pts, prm)
    for cap in (need - 1, 0):
        T.untouched_on_error(ctx, d, dict(want[3], error=R.E_CAPACITY), need, n, cap)
    at = int(np.flatnonzero(np.diff(want[2]) == 0)[40]) + 1                     # a unit of an AP that is not its first
    assert want[2][at] == want[2][at - 1]
    for what in ("one byte", "type 48", "AU step 2"):
        s, idx, au, p, aus = stream.copy(), index.copy(), nal_au.copy(), pts, n_aus
        if what == "one byte":
            idx["end"][at] = idx["start"][at] + 1
        elif what == "type 48":
            s[int(idx["start"][at])] = 48 << 1
        else:
            au[at:] += np.uint32(2 - int(au[at] - au[at - 1]))
            aus += 2
            p = np.concatenate([pts, pts[:2]])
        bad = A.pack(s, idx, au, aus, p, prm)[3]
        assert bad["error"] == R.E_ARG and bad["reserved"][0] == at + 1, what
        T.untouched_on_error(ctx, T.put(s, idx, au, aus, p, prm), bad, need, n, need)


@pytest.mark.parametrize("framing", (0, 2))
def test_round_trip_through_rtp_unpack(ctx, framing):
    """the output through hbs_rtp_unpack: the Annex-B stream of the original NALs, their AU numbers, the AUs' timestamps, no breaks,
    no drops"""
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(12 + framing)
    stream, index, nal_au, n_aus, pts = random_case(rng, 700, max_nal=500)
    prm = R.params(max_payload=400, framing=framing, flags=AGG, seq=65000, ts_base=0xFFFF0000)
    out, want, s, _ = run(ctx, stream, index, nal_au, n_aus, pts, prm)
    assert aps(want) > 50 and want[3]["reserved"][2] & 0xFFFFFFFF > 50
    offs = hbs.rtp_packet_offsets(want[1], want[2], 400, framing)
    assert np.array_equal(offs, A.packet_offsets(want[1], want[2], prm))
    got, index_out, au_out, ts_out, su = ctx.rtp_unpack(out, offs[:-1] + np.uint64(framing), np.diff(offs) - np.uint64(framing), startcode_bytes=4)
    nals = [stream[int(a):int(b)].tobytes() for a, b in zip(index["start"], index["end"])]
    assert got.cpu().numpy().tobytes() == b"".join(b"\x00\x00\x00\x01" + x for x in nals)
    rel = (nal_au - nal_au[0]).astype(np.int64)
    assert au_out.tolist() == rel.tolist() and int(su["nal_count"]) == 700 and int(su["reserved"][2]) == 0
    assert ts_out.tolist() == [(prm["ts_base"] + int(pts[a])) & R.M32 for a in range(n_aus)]
    assert int(su["nal_found"]) == want[3]["nal_count"]


def test_one_replay_from_a_graph_on_other_contents(ctx):
    """captured on a side stream after one warm-up call, replayed on other contents of the same buffers that agree in every host
    argument: other bytes, the NAL sizes in another order, other AU numbers and times"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(13)
    n = 3 * W + 11
    sizes = rng.integers(2, 700, size=n)
    prm = R.params(max_payload=1188, framing=2, flags=AGG, seq=65000, ts_base=0xFFFFFFF0)
    members = []
    for order in (sizes, sizes[::-1].copy()):
        starts = np.concatenate([[0], np.cumsum(order[:-1])])
        stream = rng.integers(0, 256, size=int(order.sum()), dtype=np.uint8)
        stream[starts] &= 0x5F
        rel = np.cumsum(rng.random(n) < 0.25)
        nal_au = (rel - rel[0] + int(rng.integers(0, 99))).astype(np.uint32)
        pts = rng.integers(0, R.TIME_LIMIT, size=n, dtype=np.uint64)             # one per NAL: enough for any AU numbering
        index = R.entries(starts, starts + order)
        members.append((stream, index, nal_au, pts, A.pack(stream, index, nal_au, n, pts, prm)))
    cap = max(m[4][3]["stream_bytes"] for m in members)
    assert not np.array_equal(members[0][4][2], members[1][4][2]) and all(aps(m[4]) > 50 for m in members)
    d = T.put(*members[0][:3], n, members[0][3], prm)
    out, no, npk = T.canary(cap), T.canary((n + 1) * 8), T.canary((n + 1) * 8)
    summary = torch.full((SUMMARY.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")

    def launch():
        return ctx.rtp_pack_async(d["stream"], d["nbytes"], d["index"], n, d["nal_au"], n, d["pts"], d["prm"], out, no, npk, summary, out_cap=cap)

    def check(want):
        T.summary_matches(ctx.read_summary(summary), want[3])
        need = want[3]["stream_bytes"]
        o = out.cpu().numpy()
        assert np.array_equal(o[:need], want[0]) and (o[need:] == T.CAN).all()
        for t, w in ((no, want[1]), (npk, want[2])):
            p = t.cpu().numpy()
            assert np.array_equal(p[: (n + 1) * 8].view(np.uint64), w) and (p[(n + 1) * 8:] == T.CAN).all()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert launch() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    check(members[0][4])
    held = ctx.device_bytes()
    for which in (1, 0):
        stream, index, nal_au, pts, want = members[which]
        for name, a in (("stream", stream), ("index", index), ("nal_au", nal_au), ("pts", pts)):
            d[name].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        for t in (out, no, npk):
            t.fill_(T.CAN)
        summary.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        check(want)
    assert ctx.device_bytes() == held


def test_flag_off_is_the_flagless_call(ctx):
    rng = np.random.default_rng(14)
    stream, index, nal_au, n_aus, pts = random_case(rng, 2 * W + 5, max_nal=300)
    prm = R.params(max_payload=100, framing=2, seq=65530)
    want = R.pack(stream, index, nal_au, n_aus, pts, prm)
    T.run(ctx, stream, index, nal_au, n_aus, pts, prm, want=want)
    assert want[3]["reserved"][2] >> 32 == 0
    out, off, s = ctx.rtp_pack(T.dev(stream), index, nal_au=nal_au, n_aus=n_aus, pts=pts, **dict(prm, flags=AGG))
    agg = A.pack(stream, index, nal_au, n_aus, pts, dict(prm, flags=AGG))
    assert np.array_equal(out.cpu().numpy(), agg[0]) and np.array_equal(off, A.packet_offsets(agg[1], agg[2], prm))
    assert len(agg[0]) < len(want[0])
