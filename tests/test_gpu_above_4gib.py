"""hbs_rtp_pack, hbs_rtp_unpack, hbs_ts_mux, hbs_ts_demux and hbs_au_insert on streams and outputs of more than 2^32 bytes: every
output byte against the plans of the references (tests/_big.py; tests/test_big_checks.py holds the checkers against the
references' own bytes and against the corruptions a lost high word would cause), every table and summary whole.  Each call is
planned first (d_out NULL), then run with out_cap exactly the planned size.  Layout A (4.6 GiB of access units around source
offset 2^32) is made on the device once; each test frees what it made."""
import numpy as np
import pytest

from tests import _auins_ref as I
from tests import _big as G
from tests import _rtp_ref as R
from tests import _rtp_unpack_ref as U
from tests import _ts_ref as D
from tests import _tsmux_ref as T

pytestmark = pytest.mark.gpu
TWO32 = 1 << 32
RTP_A = R.params(max_payload=1188, framing=2, seq=65000, ts_base=(1 << 32) - 200000)
RTP_B = R.params(max_payload=8947, framing=0, seq=7)
TS = {188: T.params(packet_bytes=188, flags=T.PCR | T.PSI_AT_IRAP, cc_es=9, pcr_lead=1000), 192: T.params(packet_bytes=192, flags=0, cc_es=3)}
INS = I.AUD | I.PARAM_SETS


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def raw(nbytes):
    import torch
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")


def host(t, dtype, count):
    return t.cpu().numpy()[:count * np.dtype(dtype).itemsize].view(dtype).copy()


@pytest.fixture(autouse=True)
def release():
    """what a test left in the allocator's cache goes back to the device before the next one"""
    import gc
    import torch
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


class World:
    def __init__(self, L):
        self.L, self.stream = L, G.make_stream(L, "cuda")
        self.index, self.nal_au = dev(L.index), dev(L.nal_au)
        self.parsed = dev(L.parsed) if L.parsed is not None else None
        self.au = dev(L.au)


@pytest.fixture(scope="module")
def world():
    import torch
    w = World(G.layout_a(1))
    yield w
    w.stream = None
    torch.cuda.empty_cache()


def summary_of(ctx, call):
    """call(summary tensor) -> the summary record"""
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = call(summary)
    assert rc == 0, rc
    return ctx.read_summary(summary)


def rescan(ctx, out, index):
    """hbs_index_extract of `out` (index only) finds the NALs of `index`"""
    got, _, s = ctx.index_extract(out, index_cap=len(index) + 16, want_rbsp=False)
    assert int(s["error"]) == 0 and len(got) == len(index)
    for f in ("start", "end"):
        G.table_equal("the output scanned again: " + f, got[f], index[f])
    G.table_equal("the output scanned again: status", got["status"] & I.ST_UNTERMINATED, index["status"] & I.ST_UNTERMINATED)


def test_layout_a_on_the_device_is_the_layout(ctx, world):
    L = world.L
    assert world.stream.numel() == L.total > TWO32
    rescan(ctx, world.stream, L.index)


# ---- RTP ---------------------------------------------------------------------------------------------------------------------------

def rtp_pack(ctx, w, prm, n_aus, pts):
    """plan, then a run into exactly the planned bytes -> (out, nal_off, nal_packet, summary, the expected plan)"""
    L, n = w.L, len(w.L.index)
    want = R.plan(L.total, L.hdr, L.index, L.nal_au, n_aus, pts, prm)
    d_pts = dev(pts) if pts is not None else None
    args = (w.stream, L.total, w.index, n, w.nal_au, n_aus, d_pts, R.params_record(prm))
    s = summary_of(ctx, lambda sm: ctx.rtp_pack_async(*args, None, None, None, sm))
    G.summary_equal(s, want[3])
    need = int(s["stream_bytes"])
    out, no, npk = raw(need), raw((n + 1) * 8), raw((n + 1) * 8)
    s = summary_of(ctx, lambda sm: ctx.rtp_pack_async(*args, out, no, npk, sm, out_cap=need))
    return out[:need], host(no, np.uint64, n + 1), host(npk, np.uint64, n + 1), s, want


def rtp_unpack(ctx, w, packets, nal_off, nal_packet, prm, want):
    """hbs_rtp_unpack of hbs_rtp_pack's output through the vectorised packet table -> (out, index, nal_au, au_ts, summary)"""
    off, size = G.packet_table(nal_off, nal_packet, prm)
    n, m = len(want[1]), len(want[3])
    args = (packets, packets.numel(), dev(off), dev(size), len(off), U.params_record(U.params(startcode_bytes=4)))
    s = summary_of(ctx, lambda sm: ctx.rtp_unpack_async(*args, None, None, None, None, sm))
    G.summary_equal(s, want[4])
    need = int(s["stream_bytes"])
    out, index, nal_au, au_ts = raw(need), raw(n * 32), raw(n * 4), raw(m * 8)
    s = summary_of(ctx, lambda sm: ctx.rtp_unpack_async(*args, out, index, nal_au, au_ts, sm, out_cap=need, nal_cap=n, au_cap=m))
    return out[:need], host(index, I.NAL_ENTRY, n), host(nal_au, np.uint32, n), host(au_ts, np.uint64, m), s


def test_rtp_pack_layout_a(ctx, world):
    """max_payload 1188, 16-bit length fields, sequence numbers and timestamps that wrap, AU numbers and times given"""
    out, nal_off, nal_packet, s, want = rtp_pack(ctx, world, RTP_A, world.L.n_aus, G.rtp_times(world.L))
    assert out.numel() > TWO32
    assert G.check_pack(out, nal_off, nal_packet, s, world.stream, want) == out.numel()
    del out


@pytest.mark.parametrize("framing", (0, 2))
def test_rtp_unpack_layout_a(ctx, world, framing):
    """the packets of layout A back to its NALs behind 4-byte start codes"""
    import torch
    L, prm, pts = world.L, dict(RTP_A, framing=framing), G.rtp_times(world.L)
    packets, nal_off, nal_packet, s, want = rtp_pack(ctx, world, prm, L.n_aus, pts)
    G.summary_equal(s, want[3])
    G.table_equal("d_nal_off", nal_off, want[1])
    G.table_equal("d_nal_packet", nal_packet, want[2])
    uw = G.unpack_plan(L, int(want[3]["nal_count"]), prm["ts_base"], pts)
    out, index, nal_au, au_ts, s = rtp_unpack(ctx, world, packets, nal_off, nal_packet, prm, uw)
    del packets
    torch.cuda.empty_cache()
    assert out.numel() > TWO32
    assert G.check_unpack(out, index, nal_au, au_ts, s, world.stream, uw) == out.numel()
    rescan(ctx, out, index)
    del out


def test_rtp_one_nal_above_4gib_there_and_back(ctx):
    """layout B: the packets of one NAL pass 2^32 bytes of output (packet_of()'s 64-bit division), full packets of 8959 bytes"""
    import torch
    L = G.layout_b(1)
    assert G.giant_output(L, RTP_B["max_payload"], RTP_B["framing"]) > TWO32
    w = World(L)
    out, nal_off, nal_packet, s, want = rtp_pack(ctx, w, RTP_B, 6, None)
    assert int(nal_off[L.giant + 1] - nal_off[L.giant]) > TWO32
    assert G.check_pack(out, nal_off, nal_packet, s, w.stream, want) == out.numel()
    uw = G.unpack_plan(L, int(want[3]["nal_count"]), 0, np.zeros(6, dtype=np.uint64))
    back, index, nal_au, au_ts, s = rtp_unpack(ctx, w, out, nal_off, nal_packet, RTP_B, uw)
    del out
    torch.cuda.empty_cache()
    assert G.check_unpack(back, index, nal_au, au_ts, s, w.stream, uw) == back.numel() > TWO32
    del back, w
    torch.cuda.empty_cache()


# ---- MPEG-TS -----------------------------------------------------------------------------------------------------------------------

def ts_mux(ctx, w, prm, pts, dts):
    """plan, then a run into exactly the planned bytes -> (out, au_packet, summary, the expected plan)"""
    L, m = w.L, w.L.n_aus
    want = T.plan(L.total, L.au, pts, dts, prm)
    args = (w.stream, L.total, w.au, m, dev(pts), dev(dts), T.params_record(prm))
    s = summary_of(ctx, lambda sm: ctx.ts_mux_async(*args, None, None, sm))
    G.summary_equal(s, want[2])
    need = int(s["stream_bytes"])
    out, au_packet = raw(need), raw((m + 1) * 4)
    s = summary_of(ctx, lambda sm: ctx.ts_mux_async(*args, out, au_packet, sm, out_cap=need))
    return out[:need], host(au_packet, np.uint32, m + 1), s, want


def ts_demux(ctx, ts, B, pid, want):
    """plan, then a run into exactly the planned bytes and PES entries -> (out, pes, summary)"""
    m = len(want[1])
    s = summary_of(ctx, lambda sm: ctx.ts_demux_async(ts, ts.numel(), B, pid, None, None, sm))
    G.summary_equal(s, want[2])
    need = int(s["stream_bytes"])
    out, pes = raw(need), raw(m * D.TS_PES.itemsize)
    s = summary_of(ctx, lambda sm: ctx.ts_demux_async(ts, ts.numel(), B, pid, out, pes, sm, out_cap=need, pes_cap=m))
    return out[:need], host(pes, D.TS_PES, m), s


@pytest.mark.parametrize("B", (188, 192))
def test_ts_mux_layout_a(ctx, world, B):
    """188-byte packets with PCRs and PAT / PMT in front of every IRAP access unit; 192-byte packets without either"""
    pts, dts = G.times(world.L)
    out, au_packet, s, want = ts_mux(ctx, world, TS[B], pts, dts)
    assert out.numel() > TWO32
    assert G.check_mux(out, au_packet, s, world.stream, want) == out.numel()
    del out


@pytest.mark.parametrize("B", (188, 192))
def test_ts_demux_layout_a(ctx, world, B):
    """hbs_ts_mux's packets back to the access units back to back, the PES table whole (out_off beyond 2^32)"""
    import torch
    L, prm = world.L, TS[B]
    pts, dts = G.times(L)
    ts, au_packet, s, want = ts_mux(ctx, world, prm, pts, dts)
    G.summary_equal(s, want[2])
    G.table_equal("d_au_packet", au_packet, want[1])
    dw = G.demux_plan(L, pts, dts, au_packet, int(s["reserved"][1]))
    assert (dw[1]["out_off"] > TWO32).sum() > 40 and dw[2]["reserved"] == [0, 0, 0]
    out, pes, s = ts_demux(ctx, ts, B, prm["pid"], dw)
    del ts
    torch.cuda.empty_cache()
    assert G.check_demux(out, pes, s, world.stream, dw) == out.numel() > TWO32
    del out


def test_ts_demux_among_foreign_packets(ctx, world):
    """the 188-byte stream with a packet of PID 0x1FFF in front of every ninth packet: the same bytes, `packet` moved"""
    import torch
    L, prm = world.L, TS[188]
    pts, dts = G.times(L)
    ts, au_packet, s, want = ts_mux(ctx, world, prm, pts, dts)
    dw = G.demux_plan(L, pts, dts, au_packet, int(s["reserved"][1]))
    n = ts.numel() // 188
    mixed, moved = G.with_foreign_packets(ts)
    del ts
    torch.cuda.empty_cache()
    assert mixed.numel() == (n + -(-n // 9)) * 188
    out, pes, s = ts_demux(ctx, mixed, 188, prm["pid"], dw)
    del mixed
    torch.cuda.empty_cache()
    assert G.check_demux(out, pes, s, world.stream, dw, packet=moved(au_packet[:-1].astype(np.int64))) == out.numel() > TWO32
    del out


# ---- hbs_au_insert ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("above", (False, True))
def test_au_insert_layout_a(ctx, world, above):
    """AUDs and parameter sets over the whole stream, and over the access units from the first that begins above 2^32 (ub0 >
    2^32: every output offset is a difference of large numbers); sets from source offsets below 2^32 either way"""
    L = world.L
    first = L.cross + 1 if above else 0
    n, m = len(L.index), L.n_aus
    want = I.plan(L.total, L.index, L.parsed, L.au, L.nal_au, first, m, INS)
    assert int(L.au["unit_begin"][first]) > TWO32 or not above
    sets_end = int(L.au["unit_begin"][1])                      # the parameter sets stand in AU 0
    assert sum(seg[0] == "copy" and seg[2] + seg[3] <= sets_end and (above or seg[1] > TWO32) for seg in want[0][1:]) >= 6
    args = (world.stream, L.total, world.index, world.parsed, n, world.au, world.nal_au, m, first, m, INS)
    s = summary_of(ctx, lambda sm: ctx.au_insert_async(*args, None, None, None, None, None, sm))
    G.summary_equal(s, want[5])
    need, M, cnt = int(s["stream_bytes"]), int(s["nal_count"]), int(s["reserved"][2])
    out, index_out, nal_src, nal_au_out, au_out = raw(need), raw(M * 32), raw(M * 4), raw(M * 4), raw(cnt * 64)
    s = summary_of(ctx, lambda sm: ctx.au_insert_async(*args, out, index_out, nal_src, nal_au_out, au_out, sm, out_cap=need, index_cap=M))
    out = out[:need]
    assert need > TWO32 or above
    index_host = host(index_out, I.NAL_ENTRY, M)
    got = G.check_insert(out, index_host, host(nal_src, np.uint32, M), host(nal_au_out, np.uint32, M), host(au_out, I.ACCESS_UNIT, cnt), s, world.stream, want)
    assert got == need
    # neither exception of rescan_exceptions can apply: no byte in front of the first start code, a last NAL of three bytes or more
    assert int(L.index["start"][0]) == int(L.gap[0]) and int(L.index["end"][-1] - L.index["start"][-1]) >= 3
    rescan(ctx, out, index_host)
    del out
