"""The device logic single-stepped on the CPU (tests/sim) on buffers carved out of larger arrays (tests/_carve.py): the stream,
the arena, the index and the output lie at odd offsets inside an allocation, with bytes of the test's choosing around them.
What lies in front of a stream or behind its end (halves of start codes, emulation bytes, zeros) must not reach the result;
nothing in front of or behind an output may change; the index is cleared up to its capacity.  Against the oracle on the
exact-size array.  The GPU's own version of these cases is tests/test_gpu_carved.py."""
import numpy as np
import pytest

from tests import _carve as K
from tests import _sim
from tests._orc import NAL_ENTRY

FIELDS = ("start", "end", "rbsp_off", "rbsp_len", "status")
SCANS = {"lds-image": "sim_index_extract", "register": "sim3_index_extract", "event-sparse": "sim4_index_extract"}


def scan(fn, s, off_stream, off_index, off_rbsp, index_cap, rbsp_cap, front=b"", back=b"", want_rbsp=True):
    """one scan on carved buffers -> (entries [0, index_cap), arena bytes [0, rbsp_cap), summary, damage report)"""
    n = len(s)
    _, cs = K.carve_host(n, off_stream, fill=0x00)
    cs.put(s).hostile(front, back)
    _, ci = K.carve_host(index_cap * 32, off_index)
    ci.put(np.full(index_cap * 32, 0xC3, dtype=np.uint8))
    _, cr = K.carve_host(rbsp_cap, off_rbsp)
    _, cm = K.carve_host(64, 16)
    rc = getattr(_sim.lib(), fn)(cs.ptr if n else None, n, ci.ptr, index_cap, cr.ptr if want_rbsp else None, rbsp_cap, cm.ptr)
    assert rc == 0, rc
    damage = "; ".join(x for x in (("stream: " + cs.damage()) if cs.damage() else "", ("index: " + ci.damage()) if ci.damage() else "",
                                   ("arena: " + cr.damage()) if cr.damage() else "", ("summary: " + cm.damage()) if cm.damage() else "") if x)
    assert np.array_equal(cs.get(), s), "the stream was written"
    return ci.get().view(NAL_ENTRY), cr.get(), cm.get().view(_sim.SUMMARY)[0], damage


def same_scan(got, want, n, tag, arena=True):
    idx, rbsp, sm, damage = got
    w_idx, w_arena, why, found, kept = want
    assert damage == "", (tag, damage)
    assert int(sm["error"]) == 0 and int(sm["stop_reason"]) == why, (tag, sm)
    assert int(sm["nal_count"]) == len(w_idx) and int(sm["stream_bytes"]) == n and list(sm["reserved"]) == [0, 0, 0], (tag, sm)
    if found is not None:
        assert int(sm["nal_found"]) == found, (tag, sm, found)
        if arena:
            assert int(sm["rbsp_bytes"]) == kept, (tag, sm, kept)
    for f in FIELDS:
        assert np.array_equal(idx[f][: len(w_idx)], w_idx[f]), (tag, f)
    # (a walk that stops at an empty NAL leaves the NALs found behind it in [nal_count, nal_found): zero from there on)
    assert not idx[max(len(w_idx), int(sm["nal_found"])):].view(np.uint8).any(), (tag, "index entries behind the NALs found are not zero")
    if why != 1:
        assert int(sm["nal_found"]) == len(w_idx), (tag, sm)
    if arena:
        assert np.array_equal(rbsp[: len(w_arena)], w_arena), (tag, "arena")


@pytest.mark.parametrize("kernel", list(SCANS))
def test_hostile_bytes_around_the_stream(orc, kernel):
    rng = np.random.default_rng(4001)
    offs = K.OFFS16
    k = 0
    for front, back, begin, end in K.hostile_cases():
        for n in (64 + k % 3, 97, 240 + (15 if k % 2 else 1), 65536 + 16 * (k % 2) + 33 * (k % 3 == 0)):
            if n > 65536 and k % 6:
                continue                                           # a tile and a bit: every sixth case
            s = K.edge_stream(rng, n, begin, end)
            want = K.expected_scan(orc, s)
            cap = len(want[0]) + 1 + k % 2
            o = (offs[k % len(offs)], K.OFFS8[(k // 2) % len(K.OFFS8)], offs[(k // 3) % len(offs)])
            tag = (kernel, n, front, back, begin, end, "offsets stream/index/arena", o)
            same_scan(scan(SCANS[kernel], s, o[0], o[1], o[2], cap, len(want[1]) + 16 * (k % 2), front, back), want, n, tag)
            k += 1
    assert k >= 48 * 3


@pytest.mark.parametrize("kernel", list(SCANS))
def test_index_is_cleared_up_to_its_capacity(orc, kernel):
    """prefilled with C3, more entries than NALs, at 0 and 8 mod 16, an odd and an even number of entries"""
    rng = np.random.default_rng(4002)
    for off in (0, 8, 16, 24, 56, 4080 + 8):
        for extra in (1, 2, 5, 64):
            for n in (0, 3, 200, 5000):
                s = K.body(rng, n) if n > 8 else np.zeros(n, dtype=np.uint8)
                want = K.expected_scan(orc, s)
                tag = (kernel, off, extra, n)
                same_scan(scan(SCANS[kernel], s, 16, off, 48, len(want[0]) + extra, len(want[1]) + 16), want, n, tag)
                same_scan(scan(SCANS[kernel], s, 16, off, 48, len(want[0]) + extra, 0, want_rbsp=False), want, n, tag, arena=False)


ARENA_ENDS = (b"\x00\x00", b"\x00", b"\x80")
ARENA_BACKS = (b"\x00", b"\x00\x00", b"\x03", b"\x01", b"\xff")
ARENA_FRONTS = (b"\x00\x00", b"\x00", b"\x00\x00\x00", b"\xff")


def emit_case(rng, nn, end, first_off=0):
    """an arena of nn NALs whose last bytes are `end`, some NALs ending in zeros, some beginning with a byte <= 3"""
    lens = [int(x) for x in rng.integers(1, 120, size=nn)]
    lens[-1] = max(lens[-1], 8)
    arena = rng.integers(0, 256, size=first_off + sum(lens), dtype=np.uint8)
    arena[rng.random(len(arena)) < 0.2] = 0
    off = first_off
    for k, ln in enumerate(lens):
        if k % 3 == 0:
            arena[off] = k % 4                                     # 00 .. 03 right at a NAL's first byte
        if k % 4 == 1 and ln >= 2:
            arena[off + ln - 2: off + ln] = 0
        off += ln
    arena[len(arena) - len(end):] = np.frombuffer(end, dtype=np.uint8)
    idx = np.zeros(nn, dtype=NAL_ENTRY)
    pos, off = 0, first_off
    for k, ln in enumerate(lens):
        g = 3 + k % 3
        idx["start"][k], idx["end"][k], idx["rbsp_off"][k], idx["rbsp_len"][k] = pos + g, pos + g + ln, off, ln
        pos += g + ln
        off += ln
    return arena, idx


def test_emit_with_hostile_bytes_around_the_arena(orc):
    rng = np.random.default_rng(4003)
    k = 0
    for end in ARENA_ENDS:
        for back in ARENA_BACKS:
            for front in ARENA_FRONTS:
                for gap_mode in (0, 1):
                    arena, idx = emit_case(rng, 1 + k % 7, end)
                    want_idx = idx.copy()
                    if gap_mode == 1:
                        pos = 0
                        for j in range(len(idx)):
                            g = 4 if j % 4 == 0 else 3
                            want_idx["start"][j], want_idx["end"][j] = pos + g, pos + g + int(idx["rbsp_len"][j])
                            pos = int(want_idx["end"][j])
                    want = orc.emit_annexb(arena, want_idx)
                    oa, oo, oi = K.OFFS1[k % len(K.OFFS1)], K.OFFS1[(k // 2) % len(K.OFFS1)], K.OFFS8[k % len(K.OFFS8)]
                    _, ca = K.carve_host(len(arena), oa, fill=0x00)
                    ca.put(arena).hostile(front, back)
                    _, ci = K.carve_host(len(idx) * 32, oi)
                    ci.put(idx)
                    cap = len(arena) * 3 // 2 + 16 * len(idx) + 64
                    _, co = K.carve_host(cap, oo)
                    _, cx = K.carve_host(len(idx) * 32, 8 if k % 2 else 0)
                    n = _sim.lib().sim_emit_annexb(ca.ptr, ci.ptr, len(idx), gap_mode, co.ptr, cap, cx.ptr)
                    tag = (end, back, front, gap_mode, "offsets arena/out/index", (oa, oo, oi))
                    assert n == len(want), (tag, n, len(want))
                    out = co.get()
                    assert np.array_equal(out[:n], want), tag
                    assert (out[n:] == K.FILL).all(), (tag, "bytes behind the emitted stream were written")
                    for c, what in ((ca, "arena"), (ci, "index"), (co, "output"), (cx, "output index")):
                        assert c.damage() == "", (tag, what, c.damage())
                    got = cx.get().view(NAL_ENTRY)
                    assert int(got["end"][-1]) == n and np.array_equal(got["rbsp_len"], idx["rbsp_len"]), tag
                    k += 1
