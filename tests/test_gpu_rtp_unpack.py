"""hbs_rtp_unpack on the GPU against the plain loop of tests/_rtp_unpack_ref.py, byte for byte and field for field: plan first,
then a run into outputs of exactly the planned capacities with canaries behind d_out, d_index_out, d_nal_au_out and d_au_ts_out,
every summary field checked.  No tolerances: every comparison is exact."""
import numpy as np
import pytest

from tests import _rtp_ref as R
from tests import _rtp_unpack_ref as U

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
W = 256                         # packets of a plan workgroup
PASS = 2048                     # plan workgroups the scans take in one pass
TILE = 64 * 1024                # output bytes of a copy workgroup


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
    assert int(s["reserved"][0]) == want["reserved"][0], (s, want)
    if want["error"] != U.E_ARG:
        for k in ("nal_count", "nal_found", "rbsp_bytes", "stream_bytes", "stop_reason"):
            assert int(s[k]) == want[k], (k, s, want)
        assert [int(x) for x in s["reserved"]] == want["reserved"], (s, want)


def put(data, off, size, prm, d_data=None):
    return dict(data=dev(data) if d_data is None else d_data, nbytes=len(data), off=dev(np.asarray(off, dtype=np.uint64)),
                size=dev(np.asarray(size, dtype=np.uint64)), n=len(off), prm=U.params_record(prm))


def call(ctx, d, out, index, nal_au, au_ts, **caps):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = ctx.rtp_unpack_async(d["data"], d["nbytes"], d["off"], d["size"], d["n"], d["prm"], out, index, nal_au, au_ts, summary, **caps)
    assert rc == 0, rc
    return ctx.read_summary(summary)


def outputs(need, nals, aus):
    return canary(need), canary(nals * 32), canary(nals * 4), canary(aus * 8)


def check_outputs(bufs, want):
    out, index, nal_au, au_ts = (t.cpu().numpy() for t in bufs)
    need, nals, aus = want["summary"]["stream_bytes"], want["summary"]["nal_count"], want["summary"]["reserved"][1]
    bad = np.flatnonzero(out[:need] != want["out"])
    if len(bad):
        k = int(np.searchsorted(want["index"]["start"], bad[0], side="right")) - 1
        raise AssertionError("output differs at byte %d (NAL %d; %d bytes of %d differ)" % (bad[0], k, len(bad), need))
    assert (out[need:] == CAN).all(), "stored behind the output"
    got = index[: nals * 32].view(U.NAL_ENTRY)
    for f in ("start", "end", "rbsp_off", "rbsp_len", "status"):
        assert np.array_equal(got[f], want["index"][f]), f
    assert (index[nals * 32:] == CAN).all(), "stored behind d_index_out"
    assert np.array_equal(nal_au[: nals * 4].view(np.uint32), want["nal_au"]) and (nal_au[nals * 4:] == CAN).all(), "d_nal_au_out"
    assert np.array_equal(au_ts[: aus * 8].view(np.uint64), want["au_ts"]) and (au_ts[aus * 8:] == CAN).all(), "d_au_ts_out"


def run(ctx, data, off, size, prm, want=None, d_data=None):
    """plan, then a run into outputs of exactly the planned capacities; everything against the plain loop -> (reference, device
    inputs, output buffers)"""
    want = want if want is not None else U.unpack(data, off, size, prm)
    ws = want["summary"]
    assert ws["error"] == 0
    d = put(data, off, size, prm, d_data)
    summary_matches(call(ctx, d, None, None, None, None), ws)
    need, nals, aus = ws["stream_bytes"], ws["nal_count"], ws["reserved"][1]
    bufs = outputs(need, nals, aus)
    summary_matches(call(ctx, d, *bufs, out_cap=need, nal_cap=nals, au_cap=aus), ws)
    check_outputs(bufs, want)
    return want, d, bufs


def untouched_on_error(ctx, d, ws, need, nals, aus, plan_error, **caps):
    """the plan reports plan_error, a run reports ws; the canary-filled outputs are untouched"""
    summary_matches(call(ctx, d, None, None, None, None), dict(ws, error=plan_error))
    bufs = outputs(need, nals, aus)
    summary_matches(call(ctx, d, *bufs, **caps), ws)
    for t in bufs:
        assert (t.cpu().numpy() == CAN).all(), "written in spite of the error"


COUNTS = (0, 1, W - 1, W, W + 1, 3 * W + 7)


@pytest.mark.parametrize("sc", (4, 3))
def test_packet_counts(ctx, sc):
    """random mixes of single NALs, FUs and aggregation packets with payloads of 4..60 bytes"""
    rng = np.random.default_rng(sc)
    for n in COUNTS:
        packets, nals, aus, times = U.random_packets(rng, n)
        data, off, size = U.lay_out(packets, rng)
        want, _, _ = run(ctx, data, off, size, U.params(startcode_bytes=sc))
        assert want["nals"] == nals and want["nal_au"].tolist() == aus and want["au_ts"].tolist() == times
        assert want["summary"]["nal_found"] == n and want["summary"]["reserved"][2] == 0


@pytest.mark.parametrize("at", (W - 1, W))
def test_long_chain_across_two_workgroup_boundaries(ctx, at):
    """one NAL of about 600 fragments of 5 bytes whose first packet is table entry `at`"""
    rng = np.random.default_rng(70 + at)
    front, nals, _, _ = U.random_packets(rng, at, aps=False)
    long_nal = U.random_nal(rng, 2 + 5 * 600 - 2)
    seq = 40000
    chain = [U.packet(p, seq + i, 777, marker=i == 599) for i, p in enumerate(U.fu_payloads(long_nal, 5))]
    assert len(chain) == 600 and at + 600 > 3 * W
    back = [U.packet(U.random_nal(rng, 9), seq + 600, 778)]
    data, off, size = U.lay_out(front + chain + back, rng)
    want, _, _ = run(ctx, data, off, size, U.params())
    assert want["nals"] == nals + [long_nal, back[0][12:]]
    # the same with its first, a middle and its last fragment lost: the NAL is gone, its neighbours are intact
    for gone in (at, at + 300, at + 599):
        keep = np.arange(len(off)) != gone
        lost, _, _ = run(ctx, data, off[keep], size[keep], U.params())
        assert lost["nals"] == nals + [back[0][12:]]
        assert lost["summary"]["reserved"][2] & 0xFFFFFFFF == 599          # the drops; the breaks are the loop's to say
        if gone == at + 300:
            assert lost["summary"]["reserved"][2] >> 32 == (want["summary"]["reserved"][2] >> 32) + 1


def test_more_plan_blocks_than_one_scan_pass(ctx):
    """PASS plan workgroups and some packets more, of about 18 bytes: single NALs of 2..6 bytes, and one chain of eight fragments
    that crosses the boundary between the two scan passes; against the vectorised restatement (which
    tests/test_rtp_unpack_ref.py holds against the loop)"""
    from hevcbitstream_amd.api import rtp_packet_offsets
    rng = np.random.default_rng(71)
    n1 = PASS * W - 3
    prm = R.params(max_payload=16, seq=65000, ts_base=0xFFFF0000)
    parts, tabs, seq = [], [], 65000
    for n, mp, top in ((n1, 16, 7), (1, 5, 19), (40, 16, 7)):            # singles, one NAL of 2 + 8 x 2 bytes as eight FUs, singles
        stream, index, nal_au, n_aus, pts = R.random_case(rng, n, max_nal=top, min_nal=2 if n > 1 else 18)
        p = dict(prm, max_payload=mp, seq=seq & 0xFFFF)
        out, nal_off, nal_packet, s = (R.pack_single_packets if n > 1 else R.pack)(stream, index, nal_au, n_aus, pts, p)
        off = rtp_packet_offsets(nal_off, nal_packet, mp)
        tabs.append((off[:-1] + np.uint64(sum(len(x) for x in parts)), np.diff(off)))
        parts.append(out)
        seq += len(off) - 1
    data = np.concatenate(parts)
    off, size = np.concatenate([t[0] for t in tabs]), np.concatenate([t[1] for t in tabs])
    assert len(off) == n1 + 8 + 40 > PASS * W and len(data) < 12_000_000
    uprm = U.params(ssrc=prm["ssrc"])
    want = U.unpack_plain(data, off, size, uprm)
    assert want["summary"]["nal_count"] == n1 + 1 + 40 and want["summary"]["reserved"][2] == 0
    run(ctx, data, off, size, uprm, want=want)


def test_reordering(ctx):
    """the same packets stored back to front in the buffer, the table in sequence order: the same output"""
    rng = np.random.default_rng(72)
    packets, nals, _, _ = U.random_packets(rng, 2 * W + 50)
    a = U.lay_out(packets, rng)
    b = U.lay_out(packets, rng, reverse=True)
    assert b[1][0] > b[1][-1]
    want, _, bufs_a = run(ctx, *a, U.params())
    _, _, bufs_b = run(ctx, *b, U.params(), want=want)
    assert want["nals"] == nals


def test_foreign_packets(ctx):
    rng = np.random.default_rng(73)
    packets, nals, _, _ = U.random_packets(rng, W + 40, aps=False)
    clean, _, _ = run(ctx, *U.lay_out(packets), U.params())
    kinds = [U.classify(p, U.params())[0] for p in packets]
    inside = [i for i in range(1, len(packets)) if kinds[i] == U.FU and not R.read_packet(packets[i])["fu_start"]]       # in front of i: in a chain
    between = [i for i in range(1, len(packets)) if i not in inside]
    assert len(between) > 20 and len(inside) > 20
    other_pt = U.packet(b"\x40\x01\xAA", 5, 5, pt=97)
    other_ssrc = U.packet(b"\x40\x01\xBB", 5, 5, ssrc=77)
    # another payload type between NALs changes nothing but the packets counted
    pk = list(packets)
    for i in sorted(between[::5], reverse=True):
        pk.insert(i, other_pt)
    got, _, _ = run(ctx, *U.lay_out(pk), U.params())
    assert got["nals"] == clean["nals"] and np.array_equal(got["out"], clean["out"]) and got["summary"]["nal_found"] == len(packets)
    # inside a chain it drops that NAL
    i = inside[len(inside) // 2]
    pk = packets[:i] + [other_pt] + packets[i:]
    got, _, _ = run(ctx, *U.lay_out(pk), U.params())
    assert len(got["nals"]) == len(nals) - 1 and got["summary"]["reserved"][2] & 0xFFFFFFFF > 0
    # another ssrc: a NAL of its own without HBS_RTPU_MATCH_SSRC, not this stream's with it
    pk = packets[:between[3]] + [other_ssrc] + packets[between[3]:]
    got, _, _ = run(ctx, *U.lay_out(pk), U.params())
    assert len(got["nals"]) == len(nals) + 1
    got, _, _ = run(ctx, *U.lay_out(pk), U.params(flags=U.MATCH_SSRC))
    assert got["nals"] == clean["nals"] and got["summary"]["nal_found"] == len(packets)
    got, _, _ = run(ctx, *U.lay_out(pk), U.params(flags=U.MATCH_SSRC, ssrc=77))
    assert got["nals"] == [b"\x40\x01\xBB"] and got["summary"]["nal_found"] == 1


def test_odd_headers_at_every_alignment(ctx):
    """packets with 0..15 CSRC entries, a header extension and padding, among them FUs and aggregation packets; a packet's first
    byte at every residue modulo 16, and the unsupported kinds among them"""
    rng = np.random.default_rng(74)
    packets, nals, aus, times = U.random_packets(rng, W + 90, odd_headers=True)
    heads = {p[0] & 0x3F for p in packets}
    assert len({h & 15 for h in heads}) == 16 and any(h & 0x10 for h in heads) and any(h & 0x20 for h in heads)
    for shift in (0, 5):
        data, off, size = U.lay_out(packets, align=lambda p: (p + shift) % 16)
        assert sorted(set((off % 16).tolist())) == list(range(16))
        want, _, _ = run(ctx, data, off, size, U.params(startcode_bytes=4 - (shift > 0)))
        assert want["nals"] == nals and want["nal_au"].tolist() == aus
    extra = [U.packet(bytes([50 << 1, 1, 9, 9]), 1, 1, csrc=2), U.packet(b"\x40", 2, 1, pad=3), U.packet(b"", 3, 1),
             U.packet(bytes([0x62, 1, 0xC0 | 20]), 4, 1, ext=1), U.packet(bytes([63 << 1, 1]), 5, 1)]
    data, off, size = U.lay_out(packets[:40] + extra + packets[40:], align=lambda p: (3 * p) % 16)
    want, _, _ = run(ctx, data, off, size, U.params())
    assert want["summary"]["reserved"][2] & 0xFFFFFFFF >= 4 and bytes([0x28, 1]) in want["nals"]


def test_aggregation_packets(ctx):
    rng = np.random.default_rng(75)
    packets, nals = [], []
    for units in range(1, 13):                                     # the last unit ends exactly at the payload's end
        u = [U.random_nal(rng, int(rng.integers(2, 70))) for _ in range(units)]
        packets.append(U.packet(U.ap_payload(u), 100 + units, 9000, marker=units % 3 == 0, csrc=units % 4, pad=(0, 4)[units % 2]))
        nals += u
    data, off, size = U.lay_out(packets, rng)
    want, _, _ = run(ctx, data, off, size, U.params(startcode_bytes=3))
    assert want["nals"] == nals
    # the marker of an aggregation packet belongs to its last unit: units 1+2+3 in AU 0, 4+5+6 in AU 1, ...
    assert want["nal_au"].tolist() == [(units - 1) // 3 for units in range(1, 13) for _ in range(units)]
    assert want["summary"]["reserved"][1] == 4


MALFORMED = {
    "a size beyond the end": lambda: U.packet(U.ap_payload([b"\x40\x01\x02"])[:-1], 1, 1),
    "one trailing byte": lambda: U.packet(U.ap_payload([b"\x40\x01\x02"]) + b"\x00", 1, 1),
    "size 0": lambda: U.packet(U.ap_payload([b"\x40\x01"]) + b"\x00\x00", 1, 1),
    "size 1": lambda: U.packet(U.ap_payload([b"\x40\x01"]) + b"\x00\x01\x40", 1, 1),
    "no unit": lambda: U.packet(U.ap_payload([]), 1, 1),
    "inner type 48": lambda: U.packet(U.ap_payload([b"\x40\x01", bytes([48 << 1, 1, 0, 2, 0x40, 1])]), 1, 1),
    "inner type 63": lambda: U.packet(U.ap_payload([bytes([63 << 1, 1])]), 1, 1),
    "FU of type 48": lambda: U.packet(bytes([0x62, 1, 0x80 | 48, 5]), 1, 1),
    "FU payload of 2 bytes": lambda: U.packet(bytes([0x62, 1]), 1, 1),
    "version 1": lambda: b"\x40" + U.packet(b"\x40\x01", 1, 1)[1:],
    "11 bytes": lambda: U.packet(b"", 1, 1)[:11],
    "CSRC entries beyond the end": lambda: U.packet(b"\x40\x01", 1, 1, csrc=1)[:15],
    "padding beyond the payload": lambda: bytes([0xA0]) + U.packet(b"\x40\x01\x0F", 1, 1)[1:],
    "padding 0": lambda: bytes([0xA0]) + U.packet(b"\x40\x01\x00", 1, 1)[1:],
}


@pytest.mark.parametrize("at", (0, W - 1, W))
def test_malformed_packets(ctx, at):
    """each malformed form is a fault at packet `at`; with a second fault in another workgroup the lowest is reported; the
    canary-filled outputs stay untouched"""
    rng = np.random.default_rng(76 + at)
    packets, _, _, _ = U.random_packets(rng, 2 * W + 30)
    clean = U.unpack(*U.lay_out(packets), U.params())["summary"]
    need, nals, aus = clean["stream_bytes"] + 64, clean["nal_count"] + 8, clean["reserved"][1] + 8
    for k, (what, make) in enumerate(MALFORMED.items()):
        pk = packets[:at] + [make()] + packets[at:]
        if k % 2:
            pk[2 * W + 9] = MALFORMED["no unit"]()
        data, off, size = U.lay_out(pk, rng)
        want = U.unpack(data, off, size, U.params())["summary"]
        assert want["error"] == U.E_ARG and want["reserved"] == [at + 1, 0, 0], (what, want)
        untouched_on_error(ctx, put(data, off, size, U.params()), want, need, nals, aus, U.E_ARG, out_cap=need, nal_cap=nals, au_cap=aus)
    # entry faults: a packet that leaves the buffer, off + size that wraps
    data, off, size = U.lay_out(packets, rng)
    for o, s in ((int(off[at]), len(data) - int(off[at]) + 1), ((1 << 64) - 8, 16), (len(data) + 1, 0), (0, (1 << 64) - 1)):
        off2, size2 = off.copy(), size.copy()
        off2[at], size2[at] = o, s
        want = U.unpack(data, off2, size2, U.params())["summary"]
        assert want["error"] == U.E_ARG and want["reserved"][0] == at + 1
        untouched_on_error(ctx, put(data, off2, size2, U.params()), want, need, nals, aus, U.E_ARG, out_cap=need, nal_cap=nals, au_cap=aus)


def test_the_last_packet_ends_at_the_end_of_the_allocation(ctx):
    """the input is an allocation of its own whose last byte is the last packet's, and the first packet begins at byte 0"""
    import torch
    rng = np.random.default_rng(77)
    packets, nals, _, _ = U.random_packets(rng, 700, lo=4, hi=200)
    data, off, size = U.lay_out(packets)
    total = 12 << 20
    shift = total - len(data)
    big = np.concatenate([data[:int(size[0])], np.full(shift, 0xEE, dtype=np.uint8), data[int(size[0]):]])
    off2 = off + np.uint64(shift)
    off2[0] = 0
    torch.cuda.empty_cache()
    d_data = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_data.copy_(torch.from_numpy(big))
    want, _, _ = run(ctx, big, off2, size, U.params(), d_data=d_data)
    assert want["nals"] == nals


@pytest.mark.parametrize("sc", (4, 3))
def test_literals_around_a_tile_boundary(ctx, sc):
    """an output above 64 KiB in which the literal of a chain's first packet (start code + two rebuilt bytes), and that of a single
    NAL, begins at each position around the 64 KiB boundary"""
    rng = np.random.default_rng(78 + sc)
    nal = U.random_nal(rng, 40)
    chain = U.fu_payloads(nal, 13)
    for kind in ("chain", "single"):
        for back in range(0, sc + 3):
            first = U.random_nal(rng, TILE - back - sc)            # the next NAL's literal begins at TILE - back
            pk = [U.packet(first, 7, 1)]
            if kind == "chain":
                pk += [U.packet(p, 8 + i, 2, marker=i == len(chain) - 1) for i, p in enumerate(chain)]
            else:
                pk += [U.packet(nal, 8, 2, marker=1)]
            pk.append(U.packet(U.random_nal(rng, 30), 20, 3))
            data, off, size = U.lay_out(pk, rng)
            want, _, _ = run(ctx, data, off, size, U.params(startcode_bytes=sc))
            assert int(want["index"]["start"][1]) == TILE - back + sc and want["nals"][1] == nal and len(want["out"]) > TILE


def test_capacities_one_short(ctx):
    rng = np.random.default_rng(79)
    packets, _, _, _ = U.random_packets(rng, 2 * W + 9)
    data, off, size = U.lay_out(packets, rng)
    prm = U.params()
    want = U.unpack(data, off, size, prm)
    ws = want["summary"]
    need, nals, aus = ws["stream_bytes"], ws["nal_count"], ws["reserved"][1]
    assert aus > 3
    d = put(data, off, size, prm)
    for caps in (dict(out_cap=need - 1, nal_cap=nals, au_cap=aus), dict(out_cap=need, nal_cap=nals - 1, au_cap=aus),
                 dict(out_cap=need, nal_cap=nals, au_cap=aus - 1), dict(out_cap=0, nal_cap=0, au_cap=0)):
        assert U.unpack(data, off, size, prm, **caps)["summary"]["error"] == U.E_CAPACITY
        untouched_on_error(ctx, d, dict(ws, error=U.E_CAPACITY), need, nals, aus, 0, **caps)
    # au_cap is looked at only with a d_au_ts_out
    out, index, nal_au, au_ts = outputs(need, nals, aus)
    summary_matches(call(ctx, d, out, index, nal_au, None, out_cap=need, nal_cap=nals, au_cap=0), ws)
    check_outputs((out, index, nal_au, canary(0)), dict(want, au_ts=np.zeros(0, dtype=np.uint64), summary=dict(ws, reserved=[0, 0, ws["reserved"][2]])))
    # the convenience call
    o, idx, au_of, ts_of, s = ctx.rtp_unpack(d["data"], off, size, **prm)
    assert np.array_equal(o.cpu().numpy(), want["out"]) and np.array_equal(au_of, want["nal_au"]) and np.array_equal(ts_of, want["au_ts"])
    assert np.array_equal(idx.cpu().numpy().view(U.NAL_ENTRY)["end"], want["index"]["end"]) and int(s["error"]) == 0
    import hevcbitstream_amd as hbs
    bad = off.copy()
    bad[5] = len(data)
    with pytest.raises(hbs.HbsError, match="packet 5"):
        ctx.rtp_unpack(d["data"], bad, size, **prm)


def test_argument_refusals(ctx):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(80)
    packets, _, _, _ = U.random_packets(rng, 40)
    data, off, size = U.lay_out(packets)
    big = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    big[16:16 + len(data)] = dev(data)
    d_off, d_size = (torch.cat([dev(x), torch.zeros(64, dtype=torch.uint8, device="cuda")]) for x in (off, size))
    cap = 100_000
    out, index, nal_au, au_ts = canary(cap), canary(3000 * 32 + 16), canary(3000 * 4 + 16), canary(3000 * 8 + 16)
    summary = torch.full((SUMMARY.itemsize + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(data=big[16:16 + len(data)], off=d_off, size=d_size, prm=U.params_record(U.params()), out=out, index=index, nal_au=nal_au,
                au_ts=au_ts, s=summary[:SUMMARY.itemsize], n=40, cap=cap)
    changes = [dict(data=big[24:24 + len(data)]), dict(data=big[17:17 + len(data)]), dict(off=d_off[4:]), dict(size=d_size[4:]), dict(out=out[8:]),
               dict(index=index[4:]), dict(nal_au=nal_au[2:]), dict(nal_au=nal_au[1:]), dict(au_ts=au_ts[4:]), dict(s=summary[8:8 + SUMMARY.itemsize]),
               dict(prm=None), dict(s=None), dict(off=None), dict(size=None), dict(data=None), dict(n=1 << 32), dict(cap=(1 << 46) + 1)]
    changes += [dict(prm=U.params_record(U.params(**bad))) for bad in (dict(payload_type=128), dict(payload_type=-1), dict(startcode_bytes=2),
                                                                       dict(startcode_bytes=5), dict(startcode_bytes=0), dict(flags=2),
                                                                       dict(flags=0x80000001))]
    p = lambda x: x.data_ptr() if x is not None else None          # noqa: E731
    for change in changes:
        a = dict(good, **change)
        ctx._bind_stream()
        rc = ctx.lib.hbs_rtp_unpack(ctx.h, p(a["data"]), len(data), p(a["off"]), p(a["size"]), a["n"],
                                    a["prm"].ctypes.data if a["prm"] is not None else None, p(a["out"]), a["cap"], p(a["index"]), p(a["nal_au"]), 3000,
                                    p(a["au_ts"]), 3000, p(a["s"]))
        assert rc == U.E_ARG, (change, rc)
    torch.cuda.synchronize()
    assert (summary.cpu().numpy() == 0x5A).all()
    for t in (out, index, nal_au, au_ts):
        assert (t.cpu().numpy() == CAN).all()
    # 2^46 itself is accepted without an output, and the good arguments are
    assert ctx.rtp_unpack_async(good["data"], len(data), d_off, d_size, 40, good["prm"], None, None, None, None, good["s"], out_cap=1 << 60) == 0
    assert ctx.rtp_unpack_async(good["data"], len(data), d_off, d_size, 40, good["prm"], out, index, nal_au, au_ts, good["s"], out_cap=cap,
                                nal_cap=3000, au_cap=3000) == 0
    assert int(ctx.read_summary(good["s"])["error"]) == 0


def packed_on_device(ctx, stream, index, nal_au, n_aus, pts, prm):
    out, off, s = ctx.rtp_pack(dev(stream), index, nal_au=nal_au, n_aus=n_aus, pts=pts, **prm)
    fr = prm["framing"]
    return out, off[:-1] + np.uint64(fr), np.diff(off) - np.uint64(fr)


@pytest.mark.parametrize("framing,mp", ((0, 1188), (2, 1188), (0, 19), (2, 19)))
def test_round_trip_on_the_device(ctx, framing, mp):
    """hbs_rtp_pack, the packet offsets from rtp_packet_offsets, hbs_rtp_unpack: the NALs, their AU numbers and the AUs' times
    come back"""
    rng = np.random.default_rng(81 + mp + framing)
    prm = R.params(max_payload=mp, framing=framing, seq=65000, ts_base=0xFFFFF000, payload_type=101)
    stream, index, nal_au, n_aus, _ = R.random_case(rng, 400, max_nal=2600 if mp > 100 else 120)
    pts = np.sort(rng.choice(1 << 24, size=n_aus, replace=False)).astype(np.uint64)
    packed, pkt_off, pkt_size = packed_on_device(ctx, stream, index, nal_au, n_aus, pts, prm)
    uprm = U.params(payload_type=101, startcode_bytes=(4, 3)[framing // 2], flags=U.MATCH_SSRC, ssrc=prm["ssrc"])
    host = packed.cpu().numpy()
    want, _, _ = run(ctx, host, pkt_off, pkt_size, uprm, d_data=packed)
    assert want["nals"] == [stream[int(a):int(b)].tobytes() for a, b in zip(index["start"], index["end"])]
    assert np.array_equal(want["nal_au"], nal_au - nal_au[0])
    assert want["au_ts"].tolist() == [(prm["ts_base"] + int(t)) & R.M32 for t in pts]
    assert want["summary"]["reserved"][2] == 0
    if framing:
        import hevcbitstream_amd as hbs
        f_off, f_size, used, frames = hbs.rtp_frames(host)
        assert np.array_equal(f_off, pkt_off) and np.array_equal(f_size, pkt_size) and used == len(host) and frames == len(pkt_off)


def test_synth_stream_through_pack_unpack_and_the_scan(ctx):
    """hevc_synth pictures -> hbs_index_extract -> hbs_rtp_pack -> hbs_rtp_unpack -> hbs_index_extract: the scan of the output finds
    the NALs where d_index_out says they are, and they are the NALs that went in"""
    from tests.hevc_synth import Synth, annexb
    g = Synth(5, rich=False)
    rng = np.random.RandomState(6)
    units = []
    for pic in range(30):
        nals = [g.vps(), g.sps_nal(1920, 1080, ctb_log2=6), g.pps_nal(force={"tiles": 0})] if pic % 10 == 0 else []
        for sl in range(3):
            pay = rng.randint(0, 256, size=int(rng.randint(30, 5000))).astype(np.uint8).tobytes()
            nals.append(g.slice_nal(19 if pic % 10 == 0 else 1, first=(sl == 0), payload=pay, address=sl * 120, tid=1))
        units.append(annexb(nals))
    stream = np.frombuffer(b"".join(units), dtype=np.uint8)
    d_stream = dev(stream)
    idx, _, s = ctx.index_extract(d_stream, want_rbsp=False)
    n = len(idx)
    assert int(s["error"]) == 0 and n > 90
    prm = R.params(max_payload=1188, framing=2, ts_step=3003)
    out, off, _ = ctx.rtp_pack(d_stream, idx, **prm)
    pkt_off, pkt_size = off[:-1] + np.uint64(2), np.diff(off) - np.uint64(2)
    want, _, bufs = run(ctx, out.cpu().numpy(), pkt_off, pkt_size, U.params(ssrc=prm["ssrc"]), d_data=out)
    assert want["nals"] == [stream[int(a):int(b)].tobytes() for a, b in zip(idx["start"], idx["end"])]
    need = want["summary"]["stream_bytes"]
    idx2, _, s2 = ctx.index_extract(bufs[0][:need].clone(), want_rbsp=False)
    assert int(s2["error"]) == 0 and len(idx2) == n
    assert np.array_equal(idx2["start"], want["index"]["start"]) and np.array_equal(idx2["end"], want["index"]["end"])
    assert np.array_equal(idx2["status"] & U.ST_UNTERMINATED, want["index"]["status"])


def test_back_to_back_with_pack_and_filter_on_one_context(ctx):
    """hbs_rtp_pack, hbs_rtp_unpack and hbs_filter_annexb alternating on one live context with changing sizes"""
    rng = np.random.default_rng(82)
    for n, mp in ((300, 60), (40, 1188), (900, 19), (5, 100), (600, 200)):
        prm = R.params(max_payload=mp, framing=2 * (n % 2), seq=int(rng.integers(0, 65536)))
        stream, index, nal_au, n_aus, pts = R.random_case(rng, n, max_nal=6 * mp if mp < 1000 else 3000)
        packed, pkt_off, pkt_size = packed_on_device(ctx, stream, index, nal_au, n_aus, pts, prm)
        want, _, bufs = run(ctx, packed.cpu().numpy(), pkt_off, pkt_size, U.params(ssrc=prm["ssrc"]), d_data=packed)
        need = want["summary"]["stream_bytes"]
        keep = (rng.random(n) < 0.6).astype(np.uint8)
        kept, ents, _ = ctx.filter_annexb(bufs[0][:need], bufs[1][: n * 32], keep=keep)
        nals = [stream[int(a):int(b)].tobytes() for a, b in zip(index["start"], index["end"])]
        host = kept.cpu().numpy()
        assert [host[int(a):int(b)].tobytes() for a, b in zip(ents["start"], ents["end"])] == [x for x, k in zip(nals, keep) if k]


def test_one_replay_from_a_graph_on_other_contents(ctx):
    """captured on a side stream after one warm-up call, replayed on other contents of the same buffers: other packets of the
    same count in a buffer of the same size, other chains, other access units; every host argument is the same"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(83)
    n = 3 * W + 11
    members = []
    for k in range(2):
        packets, _, _, _ = U.random_packets(rng, n, lo=4, hi=300)
        data, off, size = U.lay_out(packets, rng)
        members.append([data, off, size])
    nbytes = max(len(m[0]) for m in members)
    prm = U.params()
    for m in members:
        m[0] = np.concatenate([m[0], np.zeros(nbytes - len(m[0]), dtype=np.uint8)])
        m.append(U.unpack(m[0], m[1], m[2], prm))
    need = max(m[3]["summary"]["stream_bytes"] for m in members)
    nals = max(m[3]["summary"]["nal_count"] for m in members)
    aus = max(m[3]["summary"]["reserved"][1] for m in members)
    assert not np.array_equal(members[0][3]["out"], members[1][3]["out"])
    d = put(*members[0][:3], prm)
    out, index, nal_au, au_ts = outputs(need, nals, aus)
    summary = torch.full((SUMMARY.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")

    def launch():
        return ctx.rtp_unpack_async(d["data"], nbytes, d["off"], d["size"], n, d["prm"], out, index, nal_au, au_ts, summary, out_cap=need,
                                    nal_cap=nals, au_cap=aus)

    def check(want):
        ws = want["summary"]
        summary_matches(ctx.read_summary(summary), ws)
        o = out.cpu().numpy()
        assert np.array_equal(o[: ws["stream_bytes"]], want["out"]) and (o[ws["stream_bytes"]:] == CAN).all()
        got = index.cpu().numpy()[: ws["nal_count"] * 32].view(U.NAL_ENTRY)
        assert np.array_equal(got["start"], want["index"]["start"]) and np.array_equal(got["end"], want["index"]["end"])
        assert np.array_equal(got["status"], want["index"]["status"])
        assert (index.cpu().numpy()[ws["nal_count"] * 32:] == CAN).all()
        assert np.array_equal(nal_au.cpu().numpy()[: ws["nal_count"] * 4].view(np.uint32), want["nal_au"])
        assert np.array_equal(au_ts.cpu().numpy()[: ws["reserved"][1] * 8].view(np.uint64), want["au_ts"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert launch() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    check(members[0][3])
    held = ctx.device_bytes()
    for which in (1, 0):
        data, off, size, want = members[which]
        for name, a in (("data", data), ("off", off), ("size", size)):
            d[name].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        for t in (out, index, nal_au, au_ts):
            t.fill_(CAN)
        summary.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        check(want)
    assert ctx.device_bytes() == held
