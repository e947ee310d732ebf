"""Every enqueue-only call replayed from a HIP graph.  A replay differs from a second call: what the host computed at enqueue
time keeps the value it had at capture (counts, capacities, grid sizes, the emit call's number), what a call leaves in the
context's scratch is seen by the next replay together with those frozen values, and no host side of the call runs at all.  So a
call is captured once on the first sibling of a family of tests/_graph_cases.py -- inputs that agree in every host argument and
differ only in device memory -- and replayed on each sibling in the same buffers: every sibling, the captured one again, each
erroneous sibling directly in front of a good one.  After every replay the output bytes, every table, the whole summary and the
canaries are held against the plain loops of tests/_*_ref.py and the oracle, byte for byte; tests/test_graph_cases.py holds on
the CPU that the families are what this needs.  Every graph is one linear chain on one stream; nothing is allocated and nothing
waits inside a capture; timing stays off."""
import numpy as np
import pytest

from tests import _graph_cases as G
from tests import _seq_cases as S
from tests import test_gpu_sequences as Q

pytestmark = pytest.mark.gpu
CAN = Q.CAN
OUTPUTS = dict(Q.OUTPUTS, flt=(("out", 0), ("io", 1)), emit=(("out", 0), ("io", 1)), keep=(("keep", 0),))
REPLAYS = {}                                           # family -> replays that ran and matched (printed with -s)


def fill(t, byte):
    if t is not None:
        t.fill_(byte)


def alloc(c):
    """the sibling's inputs on the device, outputs of c.room bytes with canaries behind them, a summary full of 0xEE"""
    if c.call in S.CALLS:
        return Q.alloc(c)
    from hevcbitstream_amd.api import SUMMARY
    b = dict(summary=Q.filled(SUMMARY.itemsize, 0xEE))
    for name in G.INPUTS[c.call]:
        b[name] = Q.dev(c.a[name])
    if c.call == "parse":
        b["arena"] = Q.dev(np.concatenate([c.a["arena"], np.zeros(16, dtype=np.uint8)]))
        b["parsed"], b["structs"] = Q.canary(c.room["parsed"]), Q.canary(c.room["structs"])
        return b
    if c.call == "ext":
        b["parsed"], b["ext"] = Q.canary(c.room["parsed"]), Q.canary(c.room["ext"])
        return b
    for name, _ in OUTPUTS[c.call]:
        b[name] = Q.canary(c.room[name])
    return b


def launch(ctx, c, b):
    """the one call of the family on the current torch stream, by the *_async methods alone"""
    a, caps = c.a, c.caps
    if c.call in S.CALLS:
        return Q.launch(ctx, c, b)
    if c.call == "flt":
        return ctx.filter_annexb_async(b["s"], len(a["s"]), b["idx"], len(a["idx"]), b["out"], b["io"], b["summary"], keep=b["keep"], out_cap=caps["out_cap"])
    if c.call == "emit":
        return ctx.emit_annexb_async(b["arena"], len(a["arena"]), b["idx"], len(a["idx"]), a["gap_mode"], b["out"][: caps["out_cap"]], b["io"], b["summary"])
    if c.call == "ext":                                    # (api.py has no async form: the library itself)
        import ctypes as C
        ctx._bind_stream()
        ctx.lib.hbs_parse_extended.argtypes = [C.c_void_p] * 3 + [C.c_uint64, C.c_void_p, C.c_void_p]
        return ctx.lib.hbs_parse_extended(ctx.h, *(C.c_void_p(b[k].data_ptr()) for k in ("arena", "idx")), len(a["idx"]),
                                          C.c_void_p(b["parsed"].data_ptr()), C.c_void_p(b["ext"].data_ptr()))
    if c.call == "keep":
        return ctx.au_keep_async(b["nal_au"], b["parsed"], len(a["nal_au"]), a["first"], a["count"], b["keep"], param_sets=bool(a["param_sets"]))
    return ctx.parse_headers_async(b["arena"], b["idx"], len(a["idx"]), b["parsed"], b["structs"][: caps["structs_cap"]], b["summary"])


def upload(c, b):
    """the sibling's inputs into the captured buffers, every output back to canaries, the summary to 0xEE"""
    import torch
    for name in G.INPUTS[c.call]:
        if c.a[name] is not None:
            src = torch.from_numpy(G.as_bytes(c.a[name]).copy())
            assert b[name].numel() >= src.numel() and (c.call == "parse" or b[name].numel() == src.numel()), (c, name)
            b[name][: src.numel()].copy_(src)
    for name in [n for n, _ in OUTPUTS.get(c.call, ())] + dict(parse=["parsed", "structs"], ext=["parsed", "ext"]).get(c.call, []):
        fill(b[name], CAN)
    b["summary"].fill_(0xEE)


def same_bytes(name, got, want_array):
    x = np.ascontiguousarray(want_array)
    item, want_bytes = x.itemsize, x.view(np.uint8).reshape(-1)
    bad = np.flatnonzero(got[: len(want_bytes)] != want_bytes)
    assert len(bad) == 0, "%s differs at entry %d (byte %d; %d bytes of %d differ)" % (name, bad[0] // item, bad[0], len(bad), len(want_bytes))
    assert (got[len(want_bytes):] == CAN).all(), "stored behind " + name


def verify(ctx, c, b):
    """the summary with error and reserved[], every output and the canaries against the reference"""
    if c.call == "parse":
        return verify_parse(ctx, c, b)
    if c.call == "ext":
        return verify_ext(ctx, c, b)
    w = G.want(c)
    ws = w[-1]
    s = ctx.read_summary(b["summary"])
    if c.call == "keep":                                   # hbs_au_keep writes no summary
        assert (b["summary"].cpu().numpy() == 0xEE).all(), "the summary nobody passed was written"
    elif c.call in S.CALLS:
        if c.call == "a2l" and ws["error"] == S.E_ARG:          # the header leaves the sizes open for HBS_E_ARG
            ws = {k: v for k, v in ws.items() if k not in ("nal_count", "rbsp_bytes", "stream_bytes")}
        dict(a2l=Q.LP, l2a=Q.LP, tsd=Q.TS, tsm=Q.TM, ins=Q.AI)[c.call].summary_matches(s, ws)
        assert int(s["reserved"][0]) == S.reserved0(ws), (s, ws)
        if c.bad is not None:
            assert int(s["error"]) == S.E_ARG and int(s["reserved"][0]) == (c.bad + 1 if S.names_the_entry(c.call) else 0), (c, s)
    else:
        for k, v in ws.items():
            assert int(s[k]) == v, (k, int(s[k]), v)
        assert list(s["reserved"]) == [0, 0, 0], s
    for name, place in OUTPUTS[c.call]:
        got = b[name].cpu().numpy()
        if ws["error"]:                                    # nothing is written then
            assert (got == CAN).all(), "%s written by a call that reports error %d" % (name, ws["error"])
            continue
        same_bytes(name, got, w[place])                    # and canaries behind the sibling's own bytes, below the capacity too
    return s


def verify_parse(ctx, c, b):
    from tests._parsecmp import PARSED, compare
    n, need = len(c.a["idx"]), G.parse_need(c)
    s = ctx.read_summary(b["summary"])
    want = dict(nal_count=n, nal_found=n, rbsp_bytes=0, stream_bytes=0, stop_reason=0, error=0)
    for k, v in want.items():
        assert int(s[k]) == v, (k, int(s[k]), v)
    assert list(s["reserved"]) == [need, 0, 0], (s, need)
    parsed, structs = b["parsed"].cpu().numpy(), b["structs"].cpu().numpy()
    assert (parsed[n * PARSED.itemsize:] == CAN).all() and (structs[need:] == CAN).all(), "stored behind an output"
    compare(parsed[: n * PARSED.itemsize].view(PARSED), structs[:need], c.a["arena"], c.a["idx"], G.want(c)[0])
    return s


def verify_ext(ctx, c, b):
    """rc of the NALs of types 35..40 and nothing else of d_parsed (the canaries it was filled with stay), every hbs_ext_nal
    record: the oracle's for those NALs, zeros for the others; no summary"""
    from tests._parsecmp import PARSED
    from tests.test_ext_types import EXT, as_tuple
    rcs, recs = G.want(c)[:2]
    n = len(rcs)
    assert (b["summary"].cpu().numpy() == 0xEE).all(), "the summary nobody passed was written"
    want = np.full(n * PARSED.itemsize, CAN, dtype=np.uint8)
    extended = np.flatnonzero(rcs != G.NOT_EXTENDED)
    want.view(PARSED)["rc"][extended] = rcs[extended]
    same_bytes("parsed", b["parsed"].cpu().numpy(), want)
    raw = b["ext"].cpu().numpy()
    assert (raw[n * EXT.itemsize:] == CAN).all(), "stored behind ext"
    got = raw[: n * EXT.itemsize].view(EXT)
    for k in range(n):
        if rcs[k] == G.NOT_EXTENDED:
            assert not G.as_bytes(got[k: k + 1]).any(), (k, "the record of a NAL of another type is not zeros")
        else:
            assert as_tuple(int(rcs[k]), got[k]) == as_tuple(int(rcs[k]), recs[k]), (k, c.a["nals"][k].hex())
            assert int(got[k]["reserved"]) == 0, k


def captured(ctx, fam, after_replay=None):
    """allocate everything and upload sibling 0; one warm-up call on a side stream (it sizes the scratch); synchronise; capture
    exactly that call once; then replay on every sibling of the family's list"""
    import torch
    first = fam.members[fam.first()]
    for c in fam.members.values():                     # the references, before anything runs
        G.want(c)
    b = alloc(first)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert launch(ctx, first, b) in (0, None)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch(ctx, first, b)
    verify(ctx, first, b)                              # the warm-up call itself (a capture runs nothing)
    held = ctx.device_bytes()
    ran = 0
    for k, label in enumerate(fam.replays()):
        c = fam.members[label]
        upload(c, b)
        g.replay()
        torch.cuda.synchronize()
        try:
            verify(ctx, c, b)
            if after_replay is not None:
                after_replay(label)
        except AssertionError as e:
            raise AssertionError("%s: replay %d of %d, on %r: %s" % (fam, k + 1, len(fam.replays()), label, e)) from e
        ran += 1
    assert ctx.device_bytes() == held                  # no replay made the scratch grow
    REPLAYS[fam.name] = ran
    print("%s: %d replays matched the reference" % (fam, ran))
    return b


def run_family(name, B=188, setup=None, after_replay=None):
    import hevcbitstream_amd as hbs
    ctx = hbs.Context(0)
    try:
        if setup is not None:
            setup(ctx)
        captured(ctx, G.family(name, B), (lambda label: after_replay(ctx, label)) if after_replay else None)
    finally:
        ctx.close()


# ---- hbs_emit_annexb -----------------------------------------------------------------------------------------------------------

def test_emit_by_arena_tiles_with_dense_tiles_counted_ahead():
    """the call's number is a host counter, frozen in a graph: every replay carries the number of the captured call, so an entry of
    the count-ahead table left by the replay before looks like this replay's own unless the sample clears it"""
    def pinned(ctx):
        ctx.set_emit_path(2)
        ctx.set_count_ahead(2)

    def by_tiles(ctx, label):
        assert ctx.lib.hbs_ctx_last_emit_by_tiles(ctx.h) == 1, "the arena tiles did not do the whole call"
    run_family("emit pinned", setup=pinned, after_replay=by_tiles)


def test_emit_on_the_automatic_path():
    """sparse arenas, a zero-heavy one and an index with holes behind one another on the automatic path.  What is held is the
    bytes, the output index and the summary of every replay; WHICH chain a replay took (the single pass by NALs or count / scan /
    emit) is not observable from outside and is not checked.  hbs_ctx_last_emit_by_tiles is 0 after every replay: an arena of
    2 MB is never given to the arena tiles by the automatic path, whatever its bytes."""
    def not_by_tiles(ctx, label):
        assert ctx.lib.hbs_ctx_last_emit_by_tiles(ctx.h) == 0
    run_family("emit auto", after_replay=not_by_tiles)


def test_emit_arenas_of_tiny_nals():
    """groups of 64, a lane per NAL and an entry outside the arena behind one another in one captured chain"""
    run_family("emit tiny")


# ---- hbs_parse_headers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["parse large", "parse few"])
def test_parse_headers(name):
    """div_flag, fix_count, the lists, masks and own rows in the workspace: a replay on an ordinary stream behind one on an
    out-of-spec stream must not inherit them"""
    run_family(name)


# ---- the piece-table calls and the transport calls ----------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["small", "large"])
def test_filter_annexb(which):
    run_family("flt " + which)


@pytest.mark.parametrize("which", ["small", "large"])
def test_annexb_to_lenpref(which):
    run_family("a2l " + which)


@pytest.mark.parametrize("which", ["small", "large"])
def test_lenpref_to_annexb(which):
    run_family("l2a " + which)


@pytest.mark.parametrize("B", G.PACKET_SIZES)
def test_ts_demux(B):
    run_family("tsd", B)


@pytest.mark.parametrize("B", G.PACKET_SIZES)
def test_ts_mux(B):
    run_family("tsm", B)


def test_au_insert():
    run_family("ins")


def test_parse_extended():
    run_family("ext")


def test_au_keep():
    """the numbers of the last VPS, SPS and PPS in front of the range are cleared in front of the call's kernels: a replay whose
    range has no parameter set in front of it must not keep those of the replay before"""
    run_family("keep")


# ---- without a graph: no host wait between the calls ---------------------------------------------------------------------------

def test_ts_demux_back_to_back_without_a_host_wait():
    """small, large, small on a side stream, each into outputs of its own, enqueued one behind the other: the large call makes the
    scratch grow while the first small call may still run, and the second small call follows in the larger buffer; one wait at the
    end, then all three against the plain loop"""
    import torch
    import hevcbitstream_amd as hbs
    small, large = S.case("tsd", "small"), S.case("tsd", "large")
    jobs = [small, large, small]
    for c in jobs:
        S.want(c)
    bufs = [Q.alloc(c) for c in jobs]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx = hbs.Context(0)
    try:
        held = []
        with torch.cuda.stream(side):
            for c, b in zip(jobs, bufs):
                assert Q.launch(ctx, c, b) == 0
                held.append(ctx.device_bytes())
        torch.cuda.synchronize()
        assert held[0] < held[1] == held[2], held
        for c, b in zip(jobs, bufs):
            Q.verify(ctx, c, b)
    finally:
        ctx.close()
