"""hbs_rtp_order on the GPU against the plain loop of tests/_rtp_order_ref.py, entry for entry and field for field: plan first,
then a run into outputs of exactly the planned capacity with canaries behind d_off_out, d_size_out, d_src_out and d_ext_out, every
summary field checked.  No tolerances: every comparison is exact."""
import numpy as np
import pytest

from tests import _rtp_order_ref as O
from tests import _rtp_unpack_ref as U

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
W = 256                         # packets, or slots, of a workgroup
PASS = 2048                     # workgroups the scans take in one pass
K = 1 << 48


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
    for k in ("nal_count", "nal_found", "rbsp_bytes", "stream_bytes", "stop_reason", "error"):
        assert int(s[k]) == want[k], (k, s, want)
    assert [int(x) for x in s["reserved"]] == want["reserved"], (s, want)


def put(data, off, size, prm, d_data=None):
    return dict(data=dev(data) if d_data is None else d_data, nbytes=len(data), off=dev(np.asarray(off, dtype=np.uint64)),
                size=dev(np.asarray(size, dtype=np.uint64)), n=len(off), prm=O.params_record(prm))


def call(ctx, d, off_out, size_out, src_out, ext_out, out_cap=None):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = ctx.rtp_order_async(d["data"], d["nbytes"], d["off"], d["size"], d["n"], d["prm"], off_out, size_out, src_out, ext_out, summary,
                             out_cap=out_cap)
    assert rc == 0, rc
    return ctx.read_summary(summary)


def outputs(kept):
    return canary(kept * 8), canary(kept * 8), canary(kept * 4), canary(kept * 8)


def check_outputs(bufs, want):
    kept = want["summary"]["nal_count"]
    for t, name, width, dt in zip(bufs, ("off", "size", "src", "ext"), (8, 8, 4, 8), (np.uint64, np.uint64, np.uint32, np.uint64)):
        got = t.cpu().numpy()
        bad = np.flatnonzero(got[: kept * width].view(dt) != want[name])
        assert len(bad) == 0, "%s differs at entry %d (%d of %d differ)" % (name, bad[0], len(bad), kept)
        assert (got[kept * width:] == CAN).all(), "stored behind d_%s_out" % name


def run(ctx, data, off, size, prm, want=None, d_data=None):
    """plan, then a run into outputs of exactly the planned capacity; everything against the plain loop -> (reference, device
    inputs, output buffers)"""
    want = want if want is not None else O.order(data, off, size, prm)
    ws = want["summary"]
    assert ws["error"] == 0
    d = put(data, off, size, prm, d_data)
    summary_matches(call(ctx, d, None, None, None, None), ws)
    kept = ws["nal_count"]
    bufs = outputs(kept)
    summary_matches(call(ctx, d, *bufs, out_cap=kept), ws)
    check_outputs(bufs, want)
    # the two optional tables left out: the same two tables
    two = outputs(kept)[:2]
    summary_matches(call(ctx, d, *two, None, None, out_cap=kept), ws)
    check_outputs(two, want)
    return want, d, bufs


def untouched_on_error(ctx, d, ws, kept, plan, out_cap):
    """the plan reports `plan`, a run reports ws; the canary-filled outputs are untouched"""
    summary_matches(call(ctx, d, None, None, None, None), plan)
    bufs = outputs(kept)
    summary_matches(call(ctx, d, *bufs, out_cap=out_cap), ws)
    for t in bufs:
        assert (t.cpu().numpy() == CAN).all(), "written in spite of the error"


def stream_packets(rng, n, seq0):
    """n single NAL unit packets of 14..40 bytes with consecutive sequence numbers from seq0"""
    return [U.packet(U.random_nal(rng, int(rng.integers(2, 29))), (seq0 + k) & 0xFFFF, 90 * k) for k in range(n)]


def ordered(ctx, arrived, prm, rng=None, origin=None, sent=None):
    data, off, size = U.lay_out(arrived, rng)
    want, _, _ = run(ctx, data, off, size, prm)
    if origin is not None:
        assert [origin[i] for i in want["src"]] == list(sent)
    return want


COUNTS = (0, 1, W - 1, W, W + 1, 3 * W + 7)


@pytest.mark.parametrize("n", COUNTS)
def test_packet_counts(ctx, n):
    rng = np.random.default_rng(100 + n)
    packets = stream_packets(rng, n, int(rng.integers(0, 65536)))
    want = ordered(ctx, packets, O.params(), rng)
    assert want["src"].tolist() == list(range(n))
    assert want["summary"]["nal_count"] == n == want["summary"]["stream_bytes"] and want["summary"]["reserved"] == [0, 0, 0]
    arrived, origin = O.arrive(packets, rng, window=8, duplicates=3 if n else 0, others=0.05)
    want = ordered(ctx, arrived, O.params(), rng, origin, range(n))
    assert want["summary"]["nal_found"] == n + (3 if n else 0) and want["summary"]["reserved"][2] >> 32 == (3 if n else 0)


@pytest.mark.parametrize("at", (W - 2, W - 1, W))
def test_wrap_between_table_positions(ctx, at):
    """seq 65535 is table entry `at`, seq 0 the next; in order, and shuffled around it"""
    rng = np.random.default_rng(200 + at)
    n = 2 * W + 20
    packets = stream_packets(rng, n, 65535 - at)
    want = ordered(ctx, packets, O.params(), rng)
    assert want["src"].tolist() == list(range(n)) and int(want["ext"][at + 1]) == K + 65536 and want["summary"]["reserved"] == [0, 0, 0]
    arrived, origin = O.arrive(packets, rng, window=8, duplicates=4)
    want = ordered(ctx, arrived, O.params(), rng, origin, range(n))
    assert want["summary"]["reserved"][2] & 0xFFFFFFFF > 0 and want["summary"]["stream_bytes"] == n


def test_displacement_across_workgroups(ctx):
    rng = np.random.default_rng(300)
    n = 3 * W + 30
    packets = stream_packets(rng, n, 65000)
    # entry 5 arrives at 2 W + 5, entry 2 W + 9 at 7
    order = list(range(n))
    order.insert(2 * W + 5, order.pop(5))
    order.insert(7, order.pop(order.index(2 * W + 9)))
    want = ordered(ctx, [packets[i] for i in order], O.params(), rng, order, range(n))
    # entry 5 and everything behind position 7 but 2 W + 9 itself have a higher number in front of them
    moved = want["summary"]["reserved"][2]
    assert want["summary"]["reserved"][:2] == [0, 0] and moved == 2 * W + 2 and want["summary"]["stream_bytes"] == n
    # the whole workgroup W .. 2 W - 1 is another stream's
    others = [O.other_packet(rng, "pt") for _ in range(W)]
    arrived = [packets[i] for i in order[:W]] + others + [packets[i] for i in order[W:]]
    origin = order[:W] + [-1] * W + order[W:]
    want = ordered(ctx, arrived, O.params(), rng, origin, range(n))
    assert want["summary"]["nal_found"] == n and want["summary"]["reserved"] == [0, 0, moved]
    # the first accepted packet is not entry 0, nor in the first workgroup
    for lead in (3, W + 2):
        arrived = [O.other_packet(rng, "ssrc") for _ in range(lead)] + [packets[i] for i in order]
        want = ordered(ctx, arrived, O.params(flags=O.MATCH_SSRC), rng, [-1] * lead + order, range(n))
        assert int(want["ext"][0]) == K + 65000
    # nothing is this stream's
    want = ordered(ctx, others + others[:9], O.params(), rng)
    assert want["summary"] == O.empty_summary()
    # W + 5 arrivals of one packet
    want = ordered(ctx, [packets[3]] * (W + 5), O.params(max_span=1), rng)
    assert want["src"].tolist() == [0] and want["summary"]["reserved"] == [0, 0, (W + 4) << 32] and want["summary"]["stream_bytes"] == 1


@pytest.mark.parametrize("span", (255, 256, 257, 3 * 256 + 1))
def test_span_and_capacities(ctx, span):
    """the kept sequence numbers span exactly `span` slots, about half of them lost"""
    rng = np.random.default_rng(400 + span)
    packets = stream_packets(rng, span, 65300)
    lose = sorted(int(x) for x in rng.choice(np.arange(1, span - 1), size=span // 2, replace=False))
    arrived, origin = O.arrive(packets, rng, window=8, duplicates=5, lose=lose)
    data, off, size = U.lay_out(arrived, rng)
    want, d, _ = run(ctx, data, off, size, O.params(max_span=span))
    ws = want["summary"]
    kept = span - len(lose)
    assert ws["stream_bytes"] == span and ws["nal_count"] == kept and ws["reserved"][1] == len(lose)
    # max_span one short: the span and the accepted packets, nothing else
    short = O.order(data, off, size, O.params(max_span=span - 1))["summary"]
    assert short == dict(O.empty_summary(), error=O.E_CAPACITY, nal_found=len(arrived), stream_bytes=span)
    untouched_on_error(ctx, put(data, off, size, O.params(max_span=span - 1)), short, kept, short, kept)
    # out_cap one short: all counts
    short = O.order(data, off, size, O.params(max_span=span), out_cap=kept - 1)["summary"]
    assert short == dict(ws, error=O.E_CAPACITY)
    untouched_on_error(ctx, d, short, kept, ws, kept - 1)
    untouched_on_error(ctx, d, short, kept, ws, 0)


def test_after(ctx):
    rng = np.random.default_rng(500)
    a_seq = 65400
    after = K + 5 * 65536 + a_seq
    old = stream_packets(rng, 31, a_seq - 30)                        # ... up to and with the packet after_ext names
    new = stream_packets(rng, 300, a_seq + 1)
    prm = O.params(flags=O.AFTER, after_ext=after)

    def shuffled(part):
        return [part[i] for i in O.arrival_order(len(part), 8, rng)]
    # late packets in front, between and behind
    arrived = old[:5] + shuffled(new[:150]) + old[5:10] + shuffled(new[150:]) + old[28:]
    want = ordered(ctx, arrived, prm, rng)
    ws = want["summary"]
    assert ws["nal_count"] == 300 == ws["stream_bytes"] and ws["nal_found"] == 313 and ws["rbsp_bytes"] == after + 300 and ws["reserved"][1] == 0
    assert want["ext"].tolist() == list(range(after + 1, after + 301))
    # the first arrival is not late; a late one between
    want = ordered(ctx, shuffled(new[:150]) + old[30:] + shuffled(new[150:]), prm, rng)
    assert want["summary"]["nal_count"] == 300 and want["summary"]["nal_found"] == 301
    # a leading loss: after_ext + 1 and + 2 never come, and count
    want = ordered(ctx, old[20:] + shuffled(new[2:]), prm, rng)
    assert want["summary"]["stream_bytes"] == 300 and want["summary"]["nal_count"] == 298 and want["summary"]["reserved"][1] == 2
    assert int(want["ext"][0]) == after + 3
    # everything is late
    want = ordered(ctx, old, prm, rng)
    assert want["summary"] == dict(O.empty_summary(), nal_found=31)


def test_chaining_three_calls(ctx):
    """a table cut where no packet is displaced across the cut: three calls, each behind the last, are one call on the whole"""
    rng = np.random.default_rng(501)
    seq0 = 65200
    packets = stream_packets(rng, 700, seq0)
    parts, sent = [], []
    for lo, hi in ((0, 250), (250, 300), (300, 700)):
        lose = [lo + 3, hi - 1] if hi - lo > 100 else []
        arrived, origin = O.arrive(packets[lo:hi], rng, window=8, duplicates=4, lose=[x - lo for x in lose])
        parts.append(arrived)
        sent += [i for i in range(lo, hi) if i not in lose]
    whole = ordered(ctx, parts[0] + parts[1] + parts[2], O.params(), rng)
    assert [int(e) - K - seq0 for e in whole["ext"]] == sent
    after, ext, dups = K + seq0 - 1, [], 0
    for arrived in parts:
        want = ordered(ctx, arrived, O.params(flags=O.AFTER, after_ext=after), rng)
        after = want["summary"]["rbsp_bytes"]
        ext += want["ext"].tolist()
        dups += want["summary"]["reserved"][2] >> 32
    assert ext == whole["ext"].tolist() and after == whole["summary"]["rbsp_bytes"] and dups == whole["summary"]["reserved"][2] >> 32 == 12


def test_adversarial_sequence_numbers(ctx):
    rng = np.random.default_rng(600)
    # random 16-bit values
    arrived = O.seq_packets(rng.integers(0, 65536, size=700), size=5)
    data, off, size = U.lay_out(arrived, rng)
    ref = O.order(data, off, size, O.params(max_span=1 << 33))
    span = ref["summary"]["stream_bytes"]
    assert span > 65536 and ref["summary"]["reserved"][2] & 0xFFFFFFFF > 100
    run(ctx, data, off, size, O.params(max_span=span))
    # a strictly descending run of 400 from seq 100: ext falls below 2^48
    arrived = O.seq_packets(100 - np.arange(400), size=3)
    want = ordered(ctx, arrived, O.params(max_span=400), rng)
    assert want["src"].tolist() == list(range(399, -1, -1)) and int(want["ext"][0]) == K + 100 - 399 and want["summary"]["reserved"][2] == 399
    # the difference 0x8000 is a step back by 32768, both times: 7, 8, 8 - 32768, 9 - 32768, 9 - 65536
    seqs = [7, 8, (8 + 0x8000) & 0xFFFF, (9 + 0x8000) & 0xFFFF, 9]
    data, off, size = U.lay_out(O.seq_packets(seqs))
    ref = O.order(data, off, size, O.params(max_span=1 << 33))
    assert ref["ext"].tolist() == [K + 9 - 65536, K + 8 - 32768, K + 9 - 32768, K + 7, K + 8] and ref["summary"]["stream_bytes"] == 65536
    want, _, _ = run(ctx, data, off, size, O.params(max_span=65536))
    assert want["src"].tolist() == [4, 2, 3, 0, 1]
    want, _, _ = run(ctx, data, off, size, O.params(flags=O.AFTER, after_ext=K + 6))
    assert want["src"].tolist() == [0, 1] and want["summary"]["nal_found"] == 5


@pytest.mark.parametrize("at", (0, W - 1, W, 2 * W + 3))
def test_faults(ctx, at):
    rng = np.random.default_rng(700 + at)
    packets = stream_packets(rng, 2 * W + 30, 10)
    version1 = b"\x40" + packets[at][1:]
    short = packets[at][:11]
    kept = len(packets)
    for k, bad in enumerate((version1, short)):
        pk = packets[:at] + [bad] + packets[at + 1:]
        if k == 0 and at < 2 * W:
            pk[2 * W + 9] = pk[2 * W + 9][:11]                       # a second fault in another workgroup: the lowest is reported
        data, off, size = U.lay_out(pk, rng)
        want = O.order(data, off, size, O.params())["summary"]
        assert want == dict(O.empty_summary(), error=O.E_ARG, reserved=[at + 1, 0, 0])
        untouched_on_error(ctx, put(data, off, size, O.params()), want, kept, want, kept)
    # entry faults: a packet that leaves the buffer, off + size that wraps
    data, off, size = U.lay_out(packets, rng)
    for o, s in ((int(off[at]), len(data) - int(off[at]) + 1), ((1 << 64) - 8, 16), (len(data) + 1, 0), (0, (1 << 64) - 1), (len(data) - 5, 14)):
        off2, size2 = off.copy(), size.copy()
        off2[at], size2[at] = o, s
        want = O.order(data, off2, size2, O.params())["summary"]
        assert want == dict(O.empty_summary(), error=O.E_ARG, reserved=[at + 1, 0, 0])
        untouched_on_error(ctx, put(data, off2, size2, O.params()), want, kept, want, kept)


def test_argument_refusals(ctx):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(800)
    packets = stream_packets(rng, 40, 5)
    data, off, size = U.lay_out(packets)
    big = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    big[16:16 + len(data)] = dev(data)
    d_off, d_size = (torch.cat([dev(x), torch.zeros(64, dtype=torch.uint8, device="cuda")]) for x in (off, size))
    off_out, size_out, src_out, ext_out = canary(40 * 8 + 16), canary(40 * 8 + 16), canary(40 * 4 + 16), canary(40 * 8 + 16)
    summary = torch.full((SUMMARY.itemsize + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(data=big[16:16 + len(data)], off=d_off, size=d_size, prm=O.params_record(O.params()), off_out=off_out, size_out=size_out,
                src_out=src_out, ext_out=ext_out, s=summary[:SUMMARY.itemsize], n=40)
    changes = [dict(data=big[24:24 + len(data)]), dict(data=big[17:17 + len(data)]), dict(off=d_off[4:]), dict(size=d_size[4:]),
               dict(off_out=off_out[4:]), dict(size_out=size_out[4:]), dict(ext_out=ext_out[4:]), dict(src_out=src_out[2:]), dict(src_out=src_out[1:]),
               dict(s=summary[8:8 + SUMMARY.itemsize]), dict(prm=None), dict(s=None), dict(off=None), dict(size=None), dict(data=None),
               dict(n=(1 << 32) - 1), dict(n=1 << 32), dict(off_out=None), dict(size_out=None), dict(off_out=None, size_out=None),
               dict(off_out=None, size_out=None, ext_out=None), dict(off_out=None, size_out=None, src_out=None)]
    changes += [dict(prm=O.params_record(O.params(**bad))) for bad in (
        dict(payload_type=128), dict(payload_type=-1), dict(flags=4), dict(flags=0x80000001), dict(reserved=1), dict(max_span=0),
        dict(max_span=(1 << 33) + 1), dict(max_span=(1 << 64) - 1), dict(flags=O.AFTER, after_ext=0), dict(flags=O.AFTER, after_ext=K - 1),
        dict(flags=O.AFTER, after_ext=(1 << 62) + 1), dict(flags=O.AFTER | O.MATCH_SSRC, after_ext=(1 << 64) - 1))]
    p = lambda x: x.data_ptr() if x is not None else None          # noqa: E731

    def raw(a):
        ctx._bind_stream()
        return ctx.lib.hbs_rtp_order(ctx.h, p(a["data"]), len(data), p(a["off"]), p(a["size"]), a["n"],
                                     a["prm"].ctypes.data if a["prm"] is not None else None, p(a["off_out"]), p(a["size_out"]),
                                     p(a["src_out"]), p(a["ext_out"]), 40, p(a["s"]))
    for change in changes:
        assert raw(dict(good, **change)) == O.E_ARG, change
    torch.cuda.synchronize()
    assert (summary.cpu().numpy() == 0x5A).all()
    for t in (off_out, size_out, src_out, ext_out):
        assert (t.cpu().numpy() == CAN).all()
    # the limits themselves are accepted, a plan needs no output, and the good arguments are
    for fine in (dict(max_span=1), dict(flags=O.AFTER, after_ext=K), dict(flags=O.AFTER, after_ext=1 << 62), dict(after_ext=5)):
        assert raw(dict(good, prm=O.params_record(O.params(**fine)), off_out=None, size_out=None, src_out=None, ext_out=None)) == 0, fine
    assert raw(good) == 0
    s = ctx.read_summary(good["s"])
    assert int(s["error"]) == 0 and int(s["nal_count"]) == 40


def test_more_blocks_than_one_scan_pass(ctx):
    """PASS workgroups and 300 packets more, of 14 bytes, shuffled inside a window of 8: the second segment of every scan over
    the workgroups; against the vectorised restatement (which tests/test_rtp_order_ref.py holds against the loop)"""
    rng = np.random.default_rng(900)
    n = PASS * W + 300
    seqs = 64000 + O.arrival_order(n, 8, rng)
    data, off, size = O.header_table(n, seqs)
    assert len(data) < 8_000_000
    prm = O.params(max_span=n)
    want = O.order_plain(seqs & 0xFFFF, np.ones(n, dtype=bool), prm, off, size)
    ws = want["summary"]
    assert ws["nal_count"] == n == ws["stream_bytes"] and ws["reserved"][2] & 0xFFFFFFFF > n // 4 and ws["rbsp_bytes"] == K + 64000 + n - 1
    assert np.array_equal(seqs[want["src"]], 64000 + np.arange(n))
    d = put(data, off, size, prm)
    summary_matches(call(ctx, d, None, None, None, None), ws)
    bufs = outputs(n)
    summary_matches(call(ctx, d, *bufs, out_cap=n), ws)
    check_outputs(bufs, want)


def test_alignment(ctx):
    """d_in 16 bytes, the 64-bit tables 8 bytes and d_src_out 4 bytes off a 256-byte boundary"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(1000)
    packets = stream_packets(rng, W + 40, 65500)
    arrived, origin = O.arrive(packets, rng, window=8, duplicates=3)
    data, off, size = U.lay_out(arrived, rng)
    want = O.order(data, off, size, O.params())
    kept, n = want["summary"]["nal_count"], len(off)

    def shifted(a, by, fill=0):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        t = torch.full((by + len(a) + PAD,), fill, dtype=torch.uint8, device="cuda")
        assert t.data_ptr() % 256 == 0
        t[by:by + len(a)] = torch.from_numpy(a.copy()).cuda()
        return t[by:]
    d_data, d_off, d_size = shifted(data, 16), shifted(off, 8), shifted(size, 8)
    bufs = [shifted(np.full(kept * w, CAN, dtype=np.uint8), by, CAN) for w, by in ((8, 8), (8, 8), (4, 4), (8, 8))]
    summary = shifted(np.full(SUMMARY.itemsize, 0x5A, dtype=np.uint8), 16)[:SUMMARY.itemsize]
    assert [t.data_ptr() % 256 for t in (d_data, d_off, d_size, *bufs, summary)] == [16, 8, 8, 8, 8, 4, 8, 16]
    assert ctx.rtp_order_async(d_data, len(data), d_off, d_size, n, O.params_record(O.params()), *bufs, summary, out_cap=kept) == 0
    summary_matches(ctx.read_summary(summary), want["summary"])
    check_outputs(bufs, want)


def test_the_last_packet_ends_at_the_end_of_the_allocation(ctx):
    """the input is an allocation of its own whose last byte is the last packet's, and the first packet begins at byte 0"""
    import torch
    rng = np.random.default_rng(1001)
    packets = stream_packets(rng, 700, 1)
    arrived, origin = O.arrive(packets, rng, window=8, duplicates=2)
    data, off, size = U.lay_out(arrived)
    total = 12 << 20
    shift = total - len(data)
    big = np.concatenate([data[:int(size[0])], np.full(shift, 0xEE, dtype=np.uint8), data[int(size[0]):]])
    off2 = off + np.uint64(shift)
    off2[0] = 0
    assert int(off2[-1] + size[-1]) == total
    torch.cuda.empty_cache()
    d_data = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_data.copy_(torch.from_numpy(big))
    want, _, _ = run(ctx, big, off2, size, O.params(), d_data=d_data)
    assert [origin[i] for i in want["src"]] == list(range(700))


def test_into_rtp_unpack_on_the_device(ctx):
    """single NALs, FUs and aggregation packets with a chain of 600 fragments among them: shuffled, duplicated, some lost, then
    hbs_rtp_order -> hbs_rtp_unpack is hbs_rtp_unpack of the in-order table without the lost entries"""
    rng = np.random.default_rng(1100)
    front, _, _, _ = U.random_packets(rng, 100, seq=65300)
    long_nal = U.random_nal(rng, 2 + 5 * 600 - 2)
    seq = 65300 + len(front)
    chain = [U.packet(p, (seq + i) & 0xFFFF, 4_000_000, marker=i == 599) for i, p in enumerate(U.fu_payloads(long_nal, 5))]
    back, _, _, _ = U.random_packets(rng, 3 * W + 7 - len(front) - 600, seq=(seq + 600) & 0xFFFF)
    packets = front + chain + back
    assert len(packets) == 3 * W + 7 and len(chain) == 600
    lose = sorted(int(x) for x in rng.choice(np.arange(1, len(packets) - 1), size=12, replace=False))
    left = [p for i, p in enumerate(packets) if i not in lose]
    l_data, l_off, l_size = U.lay_out(left)
    w_out, w_index, w_nal_au, w_au_ts, w_s = ctx.rtp_unpack(dev(l_data), l_off, l_size, **U.params())
    arrived, origin = O.arrive(packets, rng, window=8, duplicates=10, lose=lose, others=0.03)
    data, off, size = U.lay_out(arrived, rng)
    d_data = dev(data)
    o_off, o_size, src, ext, s = ctx.rtp_order(d_data, off, size, **{k: v for k, v in O.params().items() if k != "reserved"})
    assert int(s["reserved"][2]) & 0xFFFFFFFF > 0 and int(s["reserved"][2]) >> 32 == 10 and int(s["reserved"][1]) == 12
    assert [origin[i] for i in src] == [i for i in range(len(packets)) if i not in lose]
    assert np.array_equal(ext, K + 65300 + np.array([i for i in range(len(packets)) if i not in lose], dtype=np.uint64))
    out, index, nal_au, au_ts, us = ctx.rtp_unpack(d_data, o_off, o_size, **U.params())
    assert np.array_equal(out.cpu().numpy(), w_out.cpu().numpy())
    assert np.array_equal(index.cpu().numpy(), w_index.cpu().numpy())
    assert np.array_equal(nal_au, w_nal_au) and np.array_equal(au_ts, w_au_ts)
    for k in ("nal_count", "nal_found", "rbsp_bytes", "stream_bytes", "stop_reason", "error"):
        assert int(us[k]) == int(w_s[k]), k
    assert [int(x) for x in us["reserved"]] == [int(x) for x in w_s["reserved"]]
    # the convenience call names the faulty packet and the span
    import hevcbitstream_amd as hbs
    bad = off.copy()
    bad[5] = len(data)
    with pytest.raises(hbs.HbsError, match="packet 5"):
        ctx.rtp_order(d_data, bad, size)
    with pytest.raises(hbs.HbsError, match="span %d" % len(packets)):
        ctx.rtp_order(d_data, off, size, max_span=len(packets) - 1)


def test_one_replay_from_a_graph_on_other_contents(ctx):
    """captured on a side stream after one warm-up call, replayed on other contents of the same buffers: another shuffle of packets
    of the same sizes, other duplicates; every host argument is the same"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    rng = np.random.default_rng(1200)
    n = 3 * W + 11
    sizes = rng.integers(2, 29, size=n)
    members = []
    for k in range(2):
        packets = [U.packet(U.random_nal(rng, int(sizes[i])), (65000 + 300 * k + i) & 0xFFFF, 90 * i) for i in range(n)]
        take = O.arrival_order(n, 8, rng)
        arrived = [packets[i] for i in take]
        for at in rng.choice(n - 20, size=6 + 5 * k, replace=False):        # duplicates over packets of the same size keep every size in place
            same = [j for j in range(int(at) + 1, int(at) + 12) if len(arrived[j]) == len(arrived[int(at)])]
            if same:
                arrived[same[0]] = arrived[int(at)]
        data, off, size = U.lay_out(arrived)
        members.append([data, off, size])
    assert len(members[0][0]) == len(members[1][0]) and not np.array_equal(members[0][2], members[1][2])
    prm = O.params(max_span=n + 50)
    for m in members:
        m.append(O.order(m[0], m[1], m[2], prm))
    assert members[0][3]["summary"] != members[1][3]["summary"] and not np.array_equal(members[0][3]["src"], members[1][3]["src"])
    cap = max(m[3]["summary"]["nal_count"] for m in members)
    nbytes = len(members[0][0])
    d = put(*members[0][:3], prm)
    bufs = outputs(cap)
    summary = torch.full((SUMMARY.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")

    def launch():
        return ctx.rtp_order_async(d["data"], nbytes, d["off"], d["size"], n, d["prm"], *bufs, summary, out_cap=cap)

    def check(want):
        summary_matches(ctx.read_summary(summary), want["summary"])
        check_outputs(bufs, want)
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
        for t in bufs:
            t.fill_(CAN)
        summary.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        check(want)
    assert ctx.device_bytes() == held
