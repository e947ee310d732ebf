"""hbs_rtp_pack on the GPU against the plain loop of tests/_rtp_ref.py, byte for byte: plan first, then a run into outputs of
exactly the planned capacity with canaries behind d_out, d_nal_off and d_nal_packet, every summary field checked; then the way
back through the reference's receiver."""
import numpy as np
import pytest

from tests import _rtp_ref as R
from tests import _carve as K
from tests._rtp_ref import random_case

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
W = 256                         # NALs of a plan workgroup
PASS = 2048                     # plan workgroups the scan takes in one pass
TILE = 64 * 1024                # output bytes of a copy workgroup
LDS_NALS = 512                  # NALs of a tile the copy stages in LDS; a tile with more reads them from memory


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
    assert int(s["error"]) == want["error"], (s, want)
    assert int(s["stop_reason"]) == 0 and int(s["nal_found"]) == want["nal_found"]
    assert int(s["reserved"][0]) == want["reserved"][0], (s, want)
    if want["error"] != R.E_ARG:
        for k in ("nal_count", "rbsp_bytes", "stream_bytes"):
            assert int(s[k]) == want[k], (k, s, want)
        assert [int(x) for x in s["reserved"]] == want["reserved"], (s, want)


def put(stream, index, nal_au, n_aus, pts, prm, d_stream=None):
    return dict(stream=dev(stream) if d_stream is None else d_stream, nbytes=len(stream), index=dev(index), n=len(index),
                nal_au=dev(nal_au) if nal_au is not None else None, n_aus=n_aus, pts=dev(pts) if pts is not None else None,
                prm=R.params_record(prm))


def call(ctx, d, out, nal_off, nal_packet, out_cap=None):
    """d: the device inputs of a case (put)"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = ctx.rtp_pack_async(d["stream"], d["nbytes"], d["index"], d["n"], d["nal_au"], d["n_aus"], d["pts"], d["prm"], out, nal_off, nal_packet,
                            summary, out_cap=out_cap)
    assert rc == 0, rc
    return ctx.read_summary(summary)


def check_outputs(out, no, npk, want, n, prm):
    want_out, want_off, want_pkt, want_s = want
    need = want_s["stream_bytes"]
    o = out.cpu().numpy()
    bad = np.flatnonzero(o[:need] != want_out)
    if len(bad):
        k = int(np.searchsorted(want_off, bad[0], side="right")) - 1
        raise AssertionError("output differs at byte %d (NAL %d, byte %d of its packets; %d bytes of %d differ)" % (
            bad[0], k, bad[0] - int(want_off[k]), len(bad), need))
    assert (o[need:] == CAN).all(), "stored behind the output"
    for name, t, w in (("d_nal_off", no, want_off), ("d_nal_packet", npk, want_pkt)):
        p = t.cpu().numpy()
        assert np.array_equal(p[: (n + 1) * 8].view(np.uint64), w), name
        assert (p[(n + 1) * 8:] == CAN).all(), "stored behind " + name


def run(ctx, stream, index, nal_au, n_aus, pts, prm, d_stream=None, want=None):
    """plan, then a run into outputs of exactly the planned capacity; everything against the plain loop.
    -> (out, the reference's results, summary, device inputs)"""
    want = want if want is not None else R.pack(stream, index, nal_au, n_aus, pts, prm)
    want_s = want[3]
    d = put(stream, index, nal_au, n_aus, pts, prm, d_stream)
    s = call(ctx, d, None, None, None)
    summary_matches(s, want_s)
    assert want_s["error"] == 0
    need, n = int(s["stream_bytes"]), len(index)
    out, no, npk = canary(need), canary((n + 1) * 8), canary((n + 1) * 8)
    s = call(ctx, d, out, no, npk, out_cap=need)
    summary_matches(s, want_s)
    check_outputs(out, no, npk, want, n, prm)
    return out[:need], want, s, d


def untouched_on_error(ctx, d, want_s, cap_bytes, n, out_cap):
    """the plan and a run both report want_s; the canary-filled outputs are untouched"""
    summary_matches(call(ctx, d, None, None, None), dict(want_s, error=want_s["error"] if want_s["error"] == R.E_ARG else 0))
    out, no, npk = canary(cap_bytes), canary((n + 1) * 8), canary((n + 1) * 8)
    summary_matches(call(ctx, d, out, no, npk, out_cap=out_cap), want_s)
    for t in (out, no, npk):
        assert (t.cpu().numpy() == CAN).all(), "written in spite of the error"


COUNTS = (0, 1, W - 1, W, W + 1, 3 * W + 7)


@pytest.mark.parametrize("framing", (0, 2))
def test_nal_counts(ctx, framing):
    rng = np.random.default_rng(framing)
    for k, n in enumerate(COUNTS):
        prm = R.params(max_payload=(100, 19, 1188)[k % 3], framing=framing, flags=k % 2, seq=int(rng.integers(0, 65536)), ts_base=1000 * k)
        stream, index, nal_au, n_aus, pts = random_case(rng, n, max_nal=700)
        _, want, s, _ = run(ctx, stream, index, nal_au, n_aus, pts, prm)
        if n == 0:
            assert want[1].tolist() == [0] and want[2].tolist() == [0] and int(s["stream_bytes"]) == 0


def test_more_plan_blocks_than_one_scan_pass(ctx):
    """PASS plan workgroups and five NALs more, NALs of 2..5 bytes: 8.9 MB of output, against the vectorised restatement (which
    tests/test_rtp_abi.py holds against the loop); most tiles hold more NALs than the copy stages in LDS"""
    rng = np.random.default_rng(54)
    n = PASS * W + 5
    prm = R.params(max_payload=16, framing=2, seq=65000, ts_base=0xFFFF0000)
    stream, index, nal_au, n_aus, pts = random_case(rng, n, max_nal=6)
    want = R.pack_single_packets(stream, index, nal_au, n_aus, pts, prm)
    assert len(want[0]) < 12_000_000 and TILE // (2 + 12 + 5) > LDS_NALS
    run(ctx, stream, index, nal_au, n_aus, pts, prm, want=want)


def edge_lengths(mp):
    F = mp - 3
    return sorted({L for L in [2, mp - 1, mp, mp + 1] + [2 + k * F + d for k in (2, 3) for d in (-1, 0, 1)] if L >= 2})


@pytest.mark.parametrize("mp", (4, 5, 16, 19, 100, 1188, 65523))
def test_length_edges(ctx, mp):
    """L = 2, mp - 1, mp, mp + 1 and bodies of one byte less than, exactly and one byte more than 2 and 3 full fragments"""
    rng = np.random.default_rng(mp)
    sizes = np.array(edge_lengths(mp) * 2)
    starts = np.concatenate([[0], np.cumsum(sizes[:-1] + rng.integers(0, 3, size=len(sizes) - 1))])
    stream = rng.integers(0, 256, size=int(starts[-1] + sizes[-1]), dtype=np.uint8)
    stream[starts] = (rng.integers(0, 48, size=len(sizes)) << 1 | 0x81).astype(np.uint8)
    nal_au = (np.arange(len(sizes)) // 2).astype(np.uint32)
    pts = rng.integers(0, R.TIME_LIMIT, size=len(sizes), dtype=np.uint64)
    for framing in (0, 2):
        prm = R.params(max_payload=mp, framing=framing, seq=65530, ts_base=0xFFFFFFF0)
        _, want, s, _ = run(ctx, stream, R.entries(starts, starts + sizes), nal_au, len(sizes), pts, prm)
        assert np.diff(want[2]).tolist() == [R.nal_packets(int(L), mp) for L in sizes]
        assert int(s["reserved"][2]) == int((sizes > mp).sum()) > 0


def aligned_starts(rng, sizes):
    """starts that take all 16 residues modulo 16"""
    starts, at = [], 0
    for k, size in enumerate(sizes):
        at += (k % 16 - at) % 16 + 16 * int(rng.integers(0, 3))
        starts.append(at)
        at += int(size)
    return np.array(starts), at


def test_every_source_alignment(ctx):
    """start takes all 16 residues modulo 16, for NALs of one packet and of several; the output alignments come by themselves"""
    rng = np.random.default_rng(50)
    sizes = rng.integers(300, 3000, size=64)
    starts, total = aligned_starts(rng, sizes)
    assert sorted(set(starts % 16)) == list(range(16))
    stream = rng.integers(0, 256, size=total, dtype=np.uint8)
    stream[starts] &= 0x5F
    for mp, framing in ((1188, 0), (1188, 2), (100, 0), (4000, 2)):
        run(ctx, stream, R.entries(starts, starts + sizes), None, 0, None, R.params(max_payload=mp, framing=framing))


def test_gaps_between_nals_and_the_end_of_the_allocation(ctx):
    """gaps of 0, 1, 15, 16, 17 and 100 000 bytes; the last NAL ends at stream_bytes, and the stream is a 12 MiB allocation of
    its own, so that its last byte is the allocation's last"""
    import torch
    rng = np.random.default_rng(51)
    total = 12 << 20
    gaps = [0, 1, 15, 16, 17, 100000] * 20
    sizes = rng.integers(2, 3000, size=len(gaps))
    starts = np.cumsum(np.array(gaps) + np.concatenate([[0], sizes[:-1]]))
    ends = starts + sizes
    shift = total - int(ends[-1])
    assert shift >= 0
    starts, ends = starts + shift, ends + shift
    stream = rng.integers(0, 256, size=total, dtype=np.uint8)
    torch.cuda.empty_cache()                                    # (no cached block to cut the 12 MiB from)
    d_stream = torch.empty(total, dtype=torch.uint8, device="cuda")
    for mp, framing, last in ((1188, 0, 0), (1188, 2, 1), (100, 0, 17), (8948, 2, 5)):
        ends[-1] = total
        starts[-1] = total - 3000 - last
        stream[starts] &= 0x5F
        d_stream.copy_(torch.from_numpy(stream))
        nal_au = (np.arange(len(gaps)) // 4).astype(np.uint32)
        run(ctx, stream, R.entries(starts, ends), nal_au, len(gaps), None, R.params(max_payload=mp, framing=framing, ts_step=3003), d_stream=d_stream)


def test_one_nal_larger_than_three_tiles_next_to_tiny_ones(ctx):
    rng = np.random.default_rng(52)
    L = 3 * TILE + 1000
    sizes = np.array([2, 2, L, 2, 2, 2])
    starts = np.concatenate([[3], 3 + np.cumsum(sizes[:-1] + 1)])
    stream = rng.integers(0, 256, size=int(starts[-1] + sizes[-1]), dtype=np.uint8)
    stream[starts] &= 0x5F
    nal_au = np.array([7, 7, 7, 7, 8, 8], dtype=np.uint32)
    pts = np.array([90000, 93003], dtype=np.uint64)
    for mp, framing in ((1188, 0), (1188, 2), (65523, 0), (4, 2)):
        _, want, s, _ = run(ctx, stream, R.entries(starts, starts + sizes), nal_au, 2, pts, R.params(max_payload=mp, framing=framing))
        assert int(s["reserved"][2]) == 1 and np.diff(want[2]).tolist() == [1, 1, R.nal_packets(L, mp), 1, 1, 1]
        assert int(s["stream_bytes"]) > 3 * TILE


def test_many_nals_of_one_small_packet(ctx):
    """5 000 NALs of one small packet each: no chunk lies wholly inside a payload of less than 16 bytes"""
    rng = np.random.default_rng(53)
    for mp, framing, top in ((100, 0, 31), (1188, 2, 16)):
        stream, index, nal_au, n_aus, pts = random_case(rng, 5000, max_nal=top)
        _, want, s, _ = run(ctx, stream, index, nal_au, n_aus, pts, R.params(max_payload=mp, framing=framing, seq=60000))
        assert int(s["nal_count"]) == 5000 and int(s["reserved"][2]) == 0


def test_a_tile_of_slow_chunks_only_and_a_partial_last_chunk(ctx):
    """4 500 NALs of 3 bytes, framing 0: 15 output bytes a NAL, so no chunk lies behind a 12-byte header and ends inside its
    NAL.  All 4 096 chunks of the first tile are on the copy's slow list; the second tile has 1 964 bytes, 12 in its last chunk"""
    rng = np.random.default_rng(57)
    n = 4500
    starts = 3 * np.arange(n)
    stream = rng.integers(0, 256, size=3 * n, dtype=np.uint8)
    stream[starts] &= 0x5F
    nal_au = (np.arange(n) // 3).astype(np.uint32)
    pts = 3003 * np.arange(n // 3, dtype=np.uint64)
    out, _, s, _ = run(ctx, stream, R.entries(starts, starts + 3), nal_au, n // 3, pts, R.params(max_payload=1188, framing=0, seq=65000))
    assert len(out) == int(s["stream_bytes"]) == 15 * n == TILE + 1964 and 1964 % 16 == 12
    assert int(s["nal_count"]) == n and int(s["reserved"][2]) == 0


def test_sequence_numbers_across_two_calls(ctx):
    """seq starts at 65 530 and wraps; the first call ends inside an access unit (HBS_RTP_OPEN_END), the second is seeded from
    reserved[1] and takes its tables by pointer offset: together they are the one call"""
    rng = np.random.default_rng(56)
    for framing in (0, 2):
        prm = R.params(max_payload=200, framing=framing, seq=65530, ts_base=77)
        stream, index, nal_au, n_aus, pts = random_case(rng, 300, max_nal=900)
        cut = int(np.flatnonzero((nal_au[1:] == nal_au[:-1]) & (np.arange(1, 300) > 150))[0]) + 1          # NAL `cut` continues its AU
        a0 = int(nal_au[cut] - nal_au[0])
        whole, _, _, _ = run(ctx, stream, index, nal_au, n_aus, pts, prm)
        first, _, s1, _ = run(ctx, stream, index[:cut], nal_au[:cut], a0 + 1, pts, dict(prm, flags=R.OPEN_END))
        assert int(s1["reserved"][1]) > 65536 - 65530
        prm2 = dict(prm, seq=(65530 + int(s1["reserved"][1])) & 0xFFFF)
        second, _, _, _ = run(ctx, stream, index[cut:], nal_au[cut:], n_aus - a0, pts[a0:], prm2)
        both = np.concatenate([first.cpu().numpy(), second.cpu().numpy()])
        assert np.array_equal(both, whole.cpu().numpy())


def test_timestamps_that_wrap(ctx):
    rng = np.random.default_rng(57)
    stream, index, nal_au, n_aus, _ = random_case(rng, 400, max_nal=300)
    assert n_aus > 20
    pts = (np.uint64(R.TIME_LIMIT - 10 * 3003) + np.arange(n_aus, dtype=np.uint64) * np.uint64(3003)) % np.uint64(R.TIME_LIMIT)
    for p, step in ((pts, 0), (None, 0x0FFFFFFF), (None, 3003)):
        prm = R.params(max_payload=100, ts_base=0xFFFFFF00 if step != 0x0FFFFFFF else 5, ts_step=step)
        out, want, _, _ = run(ctx, stream, index, nal_au, n_aus, p, prm)
        _, _, times, _ = R.unpack(out.cpu().numpy(), R.packet_offsets(want[1], want[2], prm), prm)
        rel = (nal_au - nal_au[0]).astype(np.int64)
        expect = [(prm["ts_base"] + (int(p[a]) if p is not None else int(a) * step)) & R.M32 for a in rel]
        assert times == expect and len(set(np.array(expect) < 0x80000000)) == 2


def test_without_au_numbers_and_without_times(ctx):
    """d_nal_au == NULL: one access unit, whatever n_aus says; d_pts == NULL: ts_base + a * ts_step"""
    rng = np.random.default_rng(58)
    for with_aus in (True, False):
        for with_pts in (True, False):
            stream, index, nal_au, n_aus, pts = random_case(rng, 500, max_nal=400, aus=with_aus, times=with_pts)
            prm = R.params(max_payload=150, framing=2, ts_base=9, ts_step=3003)
            out, want, _, _ = run(ctx, stream, index, nal_au, n_aus if with_aus else 12345, pts, prm)
            _, aus, _, packets = R.unpack(out.cpu().numpy(), R.packet_offsets(want[1], want[2], prm), prm)
            if not with_aus:
                assert set(aus) == {0} and [p["marker"] for p in packets] == [0] * (len(packets) - 1) + [1]


def test_a_range_by_pointer_offset(ctx):
    """NALs [k0, k1) of a batch: d_index + k0, d_nal_au + k0, d_pts + the first AU of the range; the stream whole"""
    rng = np.random.default_rng(59)
    stream, index, nal_au, n_aus, pts = random_case(rng, 900, max_nal=500)
    k0, k1 = 301, 777
    a0, a1 = int(nal_au[k0] - nal_au[0]), int(nal_au[k1 - 1] - nal_au[0])
    prm = R.params(max_payload=120, ts_base=4)
    d = put(stream, index, nal_au, n_aus, pts, prm)
    want = R.pack(stream, index[k0:k1], nal_au[k0:k1], a1 - a0 + 1, pts[a0:], prm)
    need, n = want[3]["stream_bytes"], k1 - k0
    cutd = dict(d, index=d["index"][k0 * 32:k1 * 32], n=n, nal_au=d["nal_au"][k0 * 4:k1 * 4], n_aus=a1 - a0 + 1, pts=d["pts"][a0 * 8:])
    out, no, npk = canary(need), canary((n + 1) * 8), canary((n + 1) * 8)
    summary_matches(call(ctx, cutd, out, no, npk, out_cap=need), want[3])
    check_outputs(out, no, npk, want, n, prm)


@pytest.mark.parametrize("at", (0, W - 1, W))
def test_malformed_nals(ctx, at):
    rng = np.random.default_rng(60 + at)
    n = 2 * W + 40
    prm = R.params(max_payload=100, framing=(0, 2)[at % 2])
    stream, index0, nal_au0, n_aus, pts0 = random_case(rng, n, max_nal=300)
    clean = R.pack(stream, index0, nal_au0, n_aus, pts0, prm)[3]
    assert clean["error"] == 0
    first_of_au = int(np.flatnonzero(nal_au0 == nal_au0[at])[0])
    cases = {}
    for what in ("one byte", "type 48", "type 63", "start > end", "end > stream_bytes", "start < the end in front", "AU step 2", "AU step -1",
                 "AU number beyond n_aus", "pts 2^33", "pts absent", "two, the lowest is named"):
        s, index, nal_au, pts, aus, named = stream.copy(), index0.copy(), nal_au0.copy(), pts0.copy(), n_aus, at
        if what == "one byte":
            index["end"][at] = index["start"][at] + 1
        elif what == "type 48":
            s[int(index["start"][at])] = 48 << 1
        elif what == "type 63":
            s[int(index["start"][at])] = 0xFF
        elif what == "start > end":
            index["start"][at] = index["end"][at] + 1
        elif what == "end > stream_bytes":
            index["end"][at] = len(stream) + 1
        elif what == "start < the end in front":
            if at == 0:
                continue                                       # (NAL 0 has nothing in front of it)
            index["start"][at] = index["end"][at - 1] - 1
        elif what == "AU step 2":
            if at == 0:
                continue
            nal_au[at:] += np.uint32(2 - int(nal_au[at] - nal_au[at - 1]))
            aus += 2
            pts = np.concatenate([pts, pts[:2]])
        elif what == "AU step -1":
            if at == 0:
                continue
            nal_au[at] = nal_au[at - 1] - 1
        elif what == "AU number beyond n_aus":
            aus = int(nal_au[at] - nal_au[0])
            named = first_of_au
        elif what == "pts 2^33":
            pts[int(nal_au[at] - nal_au[0])] = 1 << 33
            named = first_of_au
        elif what == "pts absent":
            pts[int(nal_au[at] - nal_au[0])] = (1 << 64) - 1
            named = first_of_au
        else:
            s[int(index["start"][at])] = 49 << 1
            index["end"][n - 1] = len(stream) + 9
        want = R.pack(s, index, nal_au, aus, pts, prm)[3]
        assert want["error"] == R.E_ARG and want["reserved"][0] == named + 1, (what, want)
        untouched_on_error(ctx, put(s, index, nal_au, aus, pts, prm), want, clean["stream_bytes"], n, clean["stream_bytes"])
        cases[what] = True
    assert len(cases) >= 9


def test_capacity_one_byte_short(ctx):
    rng = np.random.default_rng(61)
    for framing in (0, 2):
        prm = R.params(max_payload=300, framing=framing)
        stream, index, nal_au, n_aus, pts = random_case(rng, 2 * W + 9, max_nal=900)
        want = R.pack(stream, index, nal_au, n_aus, pts, prm)
        need = want[3]["stream_bytes"]
        d = put(stream, index, nal_au, n_aus, pts, prm)
        for cap in (need - 1, need - 20, 0):
            untouched_on_error(ctx, d, dict(want[3], error=R.E_CAPACITY), need, len(index), cap)
    # the convenience call
    out, off, s = ctx.rtp_pack(d["stream"], index, nal_au=nal_au, n_aus=n_aus, pts=pts, **prm)
    assert np.array_equal(out.cpu().numpy(), want[0]) and int(s["error"]) == 0
    assert np.array_equal(off, R.packet_offsets(want[1], want[2], prm))


def test_argument_refusals(ctx):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(62)
    prm = R.params(max_payload=100)
    stream, index, nal_au, n_aus, pts = random_case(rng, 40)
    big = torch.zeros(len(stream) + 64, dtype=torch.uint8, device="cuda")
    d_index, d_au, d_pts = (torch.cat([dev(x), torch.zeros(64, dtype=torch.uint8, device="cuda")]) for x in (index, nal_au, pts))
    cap = 200_000
    out, no, npk = canary(cap), canary(41 * 8 + 16), canary(41 * 8 + 16)
    summary = torch.full((SUMMARY.itemsize + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(stream=big[16:16 + len(stream)], index=d_index, au=d_au, pts=d_pts, prm=R.params_record(prm), out=out, no=no, npk=npk,
                s=summary[:SUMMARY.itemsize], n=40, cap=cap)
    changes = [dict(stream=big[24:24 + len(stream)]), dict(stream=big[17:17 + len(stream)]), dict(index=d_index[4:]), dict(au=d_au[2:]), dict(au=d_au[1:]),
               dict(pts=d_pts[4:]), dict(out=out[8:]), dict(no=no[4:]), dict(npk=npk[4:]), dict(s=summary[8:8 + SUMMARY.itemsize]), dict(prm=None),
               dict(s=None), dict(index=None), dict(stream=None), dict(n=1 << 32), dict(cap=(1 << 46) + 1)]
    changes += [dict(prm=R.params_record(R.params(**bad))) for bad in (dict(max_payload=3), dict(max_payload=65524), dict(max_payload=-1),
                                                                        dict(payload_type=128), dict(payload_type=-1), dict(framing=1), dict(framing=4),
                                                                        dict(flags=2), dict(flags=0x80000000), dict(seq=65536))]
    p = lambda x: x.data_ptr() if x is not None else None          # noqa: E731
    for change in changes:
        a = dict(good, **change)
        ctx._bind_stream()
        rc = ctx.lib.hbs_rtp_pack(ctx.h, p(a["stream"]), len(stream), p(a["index"]), a["n"], p(a["au"]), n_aus, p(a["pts"]),
                                  a["prm"].ctypes.data if a["prm"] is not None else None, p(a["out"]), a["cap"], p(a["no"]), p(a["npk"]), p(a["s"]))
        assert rc == R.E_ARG, (change, rc)
    torch.cuda.synchronize()
    assert (summary.cpu().numpy() == 0x5A).all()
    for t in (out, no, npk):
        assert (t.cpu().numpy() == CAN).all()
    # 2^46 itself is accepted, and so is a capacity without an output
    assert ctx.rtp_pack_async(good["stream"], len(stream), d_index, 40, d_au, n_aus, d_pts, good["prm"], None, None, None, good["s"], out_cap=1 << 60) == 0
    assert ctx.rtp_pack_async(good["stream"], len(stream), d_index, 40, d_au, n_aus, d_pts, good["prm"], out, no, npk, good["s"], out_cap=cap) == 0
    assert int(ctx.read_summary(good["s"])["error"]) == 0


def test_carved_buffers_at_each_accepted_alignment(ctx):
    """every pointer of the call inside a larger allocation, at each offset from a page boundary its alignment accepts; the bytes
    around every buffer are looked at afterwards, hostile header bytes around the stream"""
    rng = np.random.default_rng(63)
    n = 300
    hostile = b"\x62\x01\x80\x60\xFF\xFF\x00\x00" * 8
    for k in range(len(K.OFFS4)):
        prm = R.params(max_payload=(1188, 100, 19)[k % 3], framing=(0, 2)[k % 2], flags=k % 2, seq=65500 + k)
        stream, index, nal_au, n_aus, pts = random_case(rng, n, max_nal=2500)
        want = R.pack(stream, index, nal_au, n_aus, pts, prm)
        need = want[3]["stream_bytes"]
        o16 = lambda j: K.OFFS16[(k + j) % len(K.OFFS16)]          # noqa: E731
        o8 = lambda j: K.OFFS8[(k + j) % len(K.OFFS8)]             # noqa: E731
        cs = K.Carved(len(stream), o16(0), hostile, K.PAD, True).put(stream).hostile(front=hostile, back=hostile)
        ci = K.Carved(n * 32, o8(5), 0xFF, K.PAD, True).put(index)
        ca = K.Carved(n * 4, K.OFFS4[k], 0xFF, K.PAD, True).put(nal_au)
        cp = K.Carved(n_aus * 8, o8(0), 0xFF, K.PAD, True).put(pts)
        co = K.Carved(need, o16(3), CAN, K.PAD, True)
        cf = K.Carved((n + 1) * 8, o8(2), CAN, K.PAD, True)
        ck = K.Carved((n + 1) * 8, o8(7), CAN, K.PAD, True)
        cm = K.Carved(64, o16(6), 0xEE, K.PAD, True)
        tag = dict(stream=o16(0), index=o8(5), nal_au=K.OFFS4[k], pts=o8(0), out=o16(3), nal_off=o8(2), nal_packet=o8(7), summary=o16(6))
        rc = ctx.rtp_pack_async(cs.view, len(stream), ci.view, n, ca.view, n_aus, cp.view, R.params_record(prm), co.view, cf.view, ck.view, cm.view,
                                out_cap=need)
        assert rc == 0, tag
        summary_matches(ctx.read_summary(cm.view), want[3])
        assert np.array_equal(co.get(), want[0]), tag
        assert np.array_equal(cf.get().view(np.uint64), want[1]) and np.array_equal(ck.get().view(np.uint64), want[2]), tag
        for name, c in (("stream", cs), ("index", ci), ("nal_au", ca), ("pts", cp), ("out", co), ("nal_off", cf), ("nal_packet", ck), ("summary", cm)):
            assert c.intact(), (tag, name, c.damage())


def test_one_replay_from_a_graph_on_other_contents(ctx):
    """captured on a side stream after one warm-up call, replayed on other contents of the same buffers: other bytes, the NAL
    sizes in another order, other AU numbers and times; every host argument is the same"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(64)
    n = 3 * W + 11
    sizes = rng.integers(2, 2600, size=n)
    prm = R.params(max_payload=1188, framing=2, seq=65000, ts_base=0xFFFFFFF0)
    members = []
    for order in (sizes, sizes[::-1].copy()):
        starts = np.concatenate([[0], np.cumsum(order[:-1])])
        stream = rng.integers(0, 256, size=int(order.sum()), dtype=np.uint8)
        stream[starts] &= 0x5F
        rel = np.cumsum(rng.random(n) < 0.25)
        nal_au = (rel - rel[0] + int(rng.integers(0, 99))).astype(np.uint32)
        pts = rng.integers(0, R.TIME_LIMIT, size=n, dtype=np.uint64)             # one per NAL: enough for any AU numbering
        index = R.entries(starts, starts + order)
        members.append((stream, index, nal_au, pts, R.pack(stream, index, nal_au, n, pts, prm)))
    need = members[0][4][3]["stream_bytes"]
    assert need == members[1][4][3]["stream_bytes"] and not np.array_equal(members[0][4][0], members[1][4][0])
    d = put(*members[0][:3], n, members[0][3], prm)
    out, no, npk = canary(need), canary((n + 1) * 8), canary((n + 1) * 8)
    summary = torch.full((SUMMARY.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")

    def launch():
        return ctx.rtp_pack_async(d["stream"], d["nbytes"], d["index"], n, d["nal_au"], n, d["pts"], d["prm"], out, no, npk, summary, out_cap=need)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert launch() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    summary_matches(ctx.read_summary(summary), members[0][4][3])
    check_outputs(out, no, npk, members[0][4], n, prm)
    held = ctx.device_bytes()
    for which in (1, 0):
        stream, index, nal_au, pts, want = members[which]
        for name, a in (("stream", stream), ("index", index), ("nal_au", nal_au), ("pts", pts)):
            d[name].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        for t in (out, no, npk):
            t.fill_(CAN)
        summary.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        summary_matches(ctx.read_summary(summary), want[3])
        check_outputs(out, no, npk, want, n, prm)
    assert ctx.device_bytes() == held


def test_end_to_end(ctx):
    """hevc_synth pictures -> index + parse -> hbs_access_units -> hbs_au_insert -> hbs_rtp_pack with d_nal_au_out -> the
    receiver: the NAL payloads of the inserted stream, grouped into the same AUs, a marker on each AU's last packet, times
    pts + ts_base"""
    import hevcbitstream_amd as hbs
    from tests.hevc_synth import Synth, annexb
    from tests.test_gpu_ts import parse_stream
    g = Synth(3, rich=False)
    rng = np.random.RandomState(4)
    units, n_nals, n_pics = [], 0, 40
    for pic in range(n_pics):
        nals = []
        if pic % 20 == 0:
            nals += [g.vps(), g.sps_nal(1920, 1080, ctb_log2=6), g.pps_nal(force={"tiles": 0})]
        for sl in range(4):
            pay = rng.randint(0, 256, size=int(rng.randint(30, 4000))).astype(np.uint8).tobytes()
            nals.append(g.slice_nal(19 if pic % 20 == 0 else 1, first=(sl == 0), payload=pay, address=sl * 120, tid=1))
        units.append(annexb(nals))
        n_nals += len(nals)
    stream = np.frombuffer(b"".join(units), dtype=np.uint8)
    d_stream = dev(stream)
    n, index, parsed, cc, structs = parse_stream(ctx, d_stream, n_nals)
    assert n == n_nals
    au, nal_au, _, _ = ctx.access_units(index, parsed, cc, structs, n)
    assert len(au) == n_pics
    ins, index_out, _, nal_au_out, _, si = ctx.au_insert(d_stream, index[: n * 32], parsed[: n * 32], n, au, nal_au)
    M = int(si["nal_count"])
    assert M > n
    pts = ((np.arange(n_pics, dtype=np.uint64) + 2) * 3003 + 90000).astype(np.uint64)
    for framing in (0, 2):
        prm = R.params(max_payload=1188, framing=framing, seq=65500, ts_base=0xFFFF0000, payload_type=97)
        out, off, s = ctx.rtp_pack(ins, index_out, n_nals=M, nal_au=nal_au_out, n_aus=n_pics, pts=pts, **prm)
        assert int(s["error"]) == 0 and int(s["nal_found"]) == M and len(off) == int(s["nal_count"]) + 1 and int(s["reserved"][2]) > 0
        nals, aus, times, packets = R.unpack(out.cpu().numpy(), off, prm)
        ents = index_out.cpu().numpy().view(hbs.NAL_ENTRY)
        host, want_au = ins.cpu().numpy(), nal_au_out.cpu().numpy().view(np.uint32)
        assert nals == [host[int(a):int(b)].tobytes() for a, b in zip(ents["start"], ents["end"])]
        assert aus == (want_au - want_au[0]).tolist() and aus[-1] == n_pics - 1
        assert times == [(0xFFFF0000 + int(pts[a])) & R.M32 for a in aus]
        assert sum(p["marker"] for p in packets) == n_pics and packets[-1]["marker"] == 1
        # byte for byte against the plain loop as well
        want = R.pack(host, ents, want_au, n_pics, pts, prm)
        assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(off, R.packet_offsets(want[1], want[2], prm))
