"""Every device call on buffers at each alignment the C ABI accepts (tests/_carve.py): no buffer starts its allocation, every
pointer goes through the offsets its entry point lets through -- 16-byte pointers 0, 16, 32, 48, 80, 240, 1008, 4080 from a page,
8-byte pointers also 8, 24, 56, 4-byte pointers also 4, 12, 60, hbs_emit_annexb's arena and output every offset 0..15 -- while the
other pointers of the call rotate through their own sets (the assignment is part of every assertion message).  Outputs are
prefilled, of exactly the size the call needs, with 4 KiB of known bytes on BOTH sides that must not change; inputs have halves
of start codes, emulation bytes and zeros in front of them and behind their end, which must not reach the result.

References: the oracle on the exact-size numpy array (scan, extract, emit), tests/_filter_ref.py, tests/_au_ref.py, the oracle's
parser (tests/_parsecmp.py).  The same call on ordinary torch buffers is a second witness only.

The last test prints the table entry point x kernel or path x pointer x offsets exercised and asserts that it is complete."""
import os

import numpy as np
import pytest

from tests import _carve as K
from tests import _au_ref as R
from tests import _filter_ref as F
from tests._orc import NAL_ENTRY

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("start", "end", "rbsp_off", "rbsp_len", "status")
E_ARG = -3
# a stream's surroundings when the case does not choose them: start codes, an emulation byte, zeros
HOSTILE_FILL = b"\x00\x00\x01\x00\x00\x03\x00\x00\x00\x01"
# tiles of the scan kernels: LDS image (hbs_common.h kTileBytes), event-sparse (hbs_sparse.h k4TileBytes: scan4_tile_bytes, and
# scan4r24_tile_bytes for its 24-row geometry), index-only streaming (hbs_scan5.hip: k5MinTileRows rows of 1 KiB on a small stream)
TILE = {2: 64 << 10, 4: 192 << 10, 6: 96 << 10, 5: 64 << 10, 0: 192 << 10}

TABLE = {}          # (entry point, kernel or path, pointer) -> offsets exercised
RAN = set()


def note(entry, path, **offs):
    for ptr, off in offs.items():
        if off is not None:
            TABLE.setdefault((entry, path, ptr), set()).add(int(off))


def covered(entry, path, ptr, want):
    got = TABLE.get((entry, path, ptr), set())
    assert set(want) <= got, (entry, path, ptr, "offsets never exercised", sorted(set(want) - got))


def G(nbytes, off, fill=K.FILL, prefill=None):
    """a carved device buffer; prefill: the byte its own bytes start with (outputs: C3 / EE)"""
    c = K.carve(nbytes, off, fill)[1]
    if prefill is not None and nbytes:
        c.view.fill_(prefill)
    return c


def damages(**bufs):
    return "; ".join("%s: %s" % (k, c.damage()) for k, c in bufs.items() if c is not None and c.damage())


def rot(seq, k, mul=1, add=0):
    return seq[(k * mul + add) % len(seq)]


def new_ctx(kernel=0, ahead=1, emit_path=None):
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    c.set_kernel(kernel)
    c.set_count_ahead(ahead)
    if emit_path is not None:
        c.set_emit_path(emit_path)
    return c


def failed_with(code, fn, *a, **kw):
    """the call must be refused on the host with `code`"""
    import hevcbitstream_amd as hbs
    try:
        rc = fn(*a, **kw)
    except hbs.HbsError as e:
        assert "failed: %d " % code in str(e), str(e)
        return
    assert rc == code, rc


# ---- hbs_index_extract --------------------------------------------------------------------------------------------------------

# name -> (kernel, count-ahead mode, with an arena, tile)
SCAN_CONFIGS = {
    "auto": (0, 1, True, TILE[0]), "auto-ahead0": (0, 0, True, TILE[0]), "auto-ahead2": (0, 2, True, TILE[0]),
    "k2": (2, 1, True, TILE[2]), "k4-ahead0": (4, 0, True, TILE[4]), "k4-ahead2": (4, 2, True, TILE[4]), "k6": (6, 1, True, TILE[6]),
    "small": (0, 1, True, 0), "auto-noarena": (0, 1, False, TILE[0]), "k5-noarena": (5, 1, False, TILE[5]),
}
PATS = [bytes([0, 0, 1]), bytes([0, 0, 0, 1]), bytes([0, 0, 3]), bytes([0, 0, 3, 0, 0, 3]), bytes([0, 0, 0]),
        bytes([0, 0, 2]), bytes([0, 0, 3, 9]), bytes([0] * 9)]


def no_empty_nals(s):
    """a start code right behind a start code is an empty NAL, which ends the walk (and a call with exact capacities then
    answers HBS_E_CAPACITY for the NALs found behind it): put a byte between them"""
    while True:
        z = (s[:-5] == 0) & (s[1:-4] == 0) & (s[2:-3] == 1) & (s[3:-2] == 0) & (s[4:-1] == 0) & (s[5:] <= 1)
        at = np.nonzero(z)[0]
        if not len(at):
            break
        s[at + 3] = 0x77
    if len(s) >= 3 and s[-1] == 1 and s[-2] == 0 and s[-3] == 0:
        s[-1] = 0x77
    return s


def stream_of(rng, kind, n, tile):
    """kind 0: fuzz with start codes and emulation bytes on chunk, row and tile borders; 1: NALs of ~200 bytes; 2: zero-heavy"""
    if kind == 0:
        s = rng.integers(4, 256, size=n, dtype=np.uint8)
        edges = set([16, 64, 128, 256, 1024, 4096, 16384]) | set(range(65536, n, 65536))
        if tile:
            edges |= set(range(tile, n + 1, tile))
        for edge in sorted(edges):
            for _ in range(2):
                p = PATS[int(rng.integers(len(PATS)))]
                at = edge - int(rng.integers(0, len(p) + 2))
                if at >= 4 and at + len(p) < n:
                    s[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    elif kind == 1:
        s = rng.integers(1, 256, size=n, dtype=np.uint8)
        at = 5
        while at + 8 < n:
            s[at:at + 4] = (0, 0, 1, 0x42) if at & 2 else (0, 0, 0, 1)
            at += int(rng.integers(150, 251))
    else:
        s = rng.integers(1, 256, size=n, dtype=np.uint8)
        s[rng.random(n) < 0.12] = 0
        for p in rng.integers(8, max(n - 8, 9), size=n // 3000 + 1):
            s[p:p + 4] = (0, 0, 1, 0x42)
    s[0:4] = (0, 0, 1, 0x40)
    return no_empty_nals(s)


def scan_call(ctx, s, o, index_cap, rbsp_cap, front=b"", back=b"", fill=HOSTILE_FILL):
    """hbs_index_extract on carved buffers; o: offsets of stream / index / rbsp / summary; rbsp_cap None: no arena.
    -> (entries [0, index_cap), arena bytes or None, summary, damage report)"""
    n = len(s)
    cs = G(n, o["stream"], fill).put(s).hostile(front, back)
    ci = G(index_cap * 32, o["index"], prefill=0xC3)
    cr = G(rbsp_cap, o["rbsp"], prefill=0xC3) if rbsp_cap is not None else None
    cm = G(64, o["summary"], prefill=0xEE)
    ctx.index_extract_async(cs.view, ci.view, index_cap, cr.view if cr is not None else None, cm.view)
    sm = ctx.read_summary(cm.view).copy()
    assert np.array_equal(cs.get(), s), (o, "the stream was written")
    return ci.get().view(NAL_ENTRY), cr.get() if cr is not None else None, sm, damages(stream=cs, index=ci, arena=cr, summary=cm)


def same_scan(got, want, n, tag, strict_tail=True):
    idx, rbsp, sm, damage = got
    w_idx, w_arena, why, found, kept = want
    print(tag, "nal_count", int(sm["nal_count"]), "nal_found", int(sm["nal_found"]), "rbsp_bytes", int(sm["rbsp_bytes"]), "error", int(sm["error"]), damage)
    assert damage == "", (tag, damage)
    assert int(sm["error"]) == 0 and int(sm["stop_reason"]) == why, (tag, sm)
    assert int(sm["nal_count"]) == len(w_idx) and int(sm["stream_bytes"]) == n and list(sm["reserved"]) == [0, 0, 0], (tag, sm)
    if found is not None:
        assert int(sm["nal_found"]) == found, (tag, sm, found)
        if rbsp is not None:
            assert int(sm["rbsp_bytes"]) == kept, (tag, sm, kept)
    for f in FIELDS:
        assert np.array_equal(idx[f][: len(w_idx)], w_idx[f]), (tag, f)
    # "the call zeroes it": what no NAL was written to is zero (a walk that stops at an empty NAL leaves the NALs found behind
    # the stop in [nal_count, nal_found))
    if strict_tail or why != 1:
        assert int(sm["nal_found"]) == len(w_idx), (tag, sm)
    assert not idx[max(len(w_idx), int(sm["nal_found"])):].view(np.uint8).any(), (tag, "index entries behind the NALs found are not zero")
    if rbsp is not None:
        assert np.array_equal(rbsp[: len(w_arena)], w_arena), (tag, "arena")


def witness(ctx, s, cap, arena, got, tag):
    """the same call on ordinary torch buffers: every summary field and entry equal"""
    import torch
    d = torch.from_numpy(s).cuda() if len(s) else torch.empty(0, dtype=torch.uint8, device="cuda")
    w_idx, w_arena, w = ctx.index_extract(d, index_cap=cap, want_rbsp=arena)
    sm = got[2]
    for f in ("nal_count", "nal_found", "rbsp_bytes", "stream_bytes", "stop_reason", "error"):
        assert int(sm[f]) == int(w[f]), (tag, f, "against ordinary buffers", int(sm[f]), int(w[f]))
    assert np.array_equal(got[0][: len(w_idx)], w_idx), (tag, "entries against ordinary buffers")
    if arena:
        assert np.array_equal(got[1][: len(w_arena)], w_arena), (tag, "arena against ordinary buffers")


def scan_offsets(k):
    return dict(stream=rot(K.OFFS16, k), index=rot(K.OFFS8, k), rbsp=rot(K.OFFS16, k, 3, 1), summary=rot(K.OFFS16, k, 5, 2))


@pytest.mark.parametrize("config", list(SCAN_CONFIGS))
def test_index_extract_at_every_alignment(orc, config):
    """streams around a whole number of the kernel's tiles, n % 16 in {0, 1, 15}; the arena exactly the RBSP bytes and + 16;
    the index prefilled with C3 and one or two entries longer than the NALs found"""
    kernel, ahead, arena, tile = SCAN_CONFIGS[config]
    rng = np.random.default_rng(5000 + sorted(SCAN_CONFIGS).index(config))
    if tile:
        lens = [tile - 16, tile - 1, tile, tile + 1, tile + 16, 2 * tile - 1, 2 * tile, 2 * tile + 1, 2 * tile + 16, 3 * tile + 15, 3 * tile + 777]
    else:               # the one-workgroup path of the automatic mode: at most 64 KiB and 16384 entries
        lens = [1000, 1001, 1007, 4096, 20000, 65536 - 16, 65535, 65536, 33, 16385, 50001]
    ctx = new_ctx(kernel, ahead)
    try:
        for k, n in enumerate(lens):
            s = stream_of(rng, k % 3, n, tile)
            want = K.expected_scan(orc, s)
            assert want[2] != 1
            cap = len(want[0]) + 1 + k % 2
            rcap = (len(want[1]) + 16 * (k % 2)) if arena else None
            o = scan_offsets(k)
            if not arena:
                o["rbsp"] = None
            tag = ("hbs_index_extract", config, "n", n, "kind", k % 3, "offsets", o, "index_cap", cap, "rbsp_cap", rcap)
            got = scan_call(ctx, s, o, cap, rcap)
            same_scan(got, want, n, tag)
            witness(ctx, s, cap, arena, got, tag)
            if config == "small":
                assert ctx.last_kernel() == 2
            note("hbs_index_extract", config, **o)
    finally:
        ctx.close()
    covered("hbs_index_extract", config, "stream", K.OFFS16)
    covered("hbs_index_extract", config, "index", K.OFFS8)
    covered("hbs_index_extract", config, "summary", K.OFFS16)
    if arena:
        covered("hbs_index_extract", config, "rbsp", K.OFFS16)
    RAN.add("scan-" + config)


@pytest.mark.parametrize("config", list(SCAN_CONFIGS))
def test_index_is_cleared_up_to_its_capacity(orc, config):
    """The index at 0 and 8 mod 16, prefilled with C3, with capacities (odd and even numbers of entries) above the NALs found --
    none at all, one, many.  An entry is four 8-byte words, so the index always holds an even number of them: at 8 mod 16 the
    prologue's clear takes a head word, 16-byte stores, and a rest word; at 0 mod 16 neither.  With no NAL found, the head word
    (entry 0's start) is written by nobody else."""
    kernel, ahead, arena, tile = SCAN_CONFIGS[config]
    rng = np.random.default_rng(5100)
    n_big = 70001 if config != "small" else 9001
    plain = rng.integers(4, 256, size=n_big, dtype=np.uint8)          # no start code: no NAL
    one = plain.copy()
    one[100:104] = (0, 0, 1, 0x40)
    many = stream_of(rng, 1, n_big, tile)
    ctx = new_ctx(kernel, ahead)
    try:
        k = 0
        for off in (0, 8, 16, 24, 56, 4080, 1008):
            for extra in (1, 2, 64, 1001):
                for s in (plain, one, many):
                    want = K.expected_scan(orc, s)
                    cap = len(want[0]) + extra
                    o = dict(stream=rot(K.OFFS16, k), index=off, rbsp=rot(K.OFFS16, k, 3, 1) if arena else None, summary=rot(K.OFFS16, k, 5, 2))
                    tag = ("hbs_index_extract", config, "index clear", "offsets", o, "index_cap", cap, "nals", len(want[0]))
                    same_scan(scan_call(ctx, s, o, cap, (len(want[1]) + 16) if arena else None), want, len(s), tag)
                    note("hbs_index_extract", config, **o)
                    k += 1
    finally:
        ctx.close()
    RAN.add("clear-" + config)


@pytest.mark.parametrize("config", list(SCAN_CONFIGS))
def test_hostile_bytes_around_the_stream(orc, config):
    """00 00 / 00 00 00 / 00 00 01 / 00 00 03 in front of the stream, 01 / 00 01 / 03 / 00 00 01 42 / zeros / FF behind it,
    crossed with streams that begin with 01, 00 01, 00 00 01, 03 and end with a payload byte, 00, 00 00, 00 00 00, 00 00 03,
    00 00 01 or an empty last NAL: the oracle's answer on the exact-size array, every time"""
    kernel, ahead, arena, tile = SCAN_CONFIGS[config]
    rng = np.random.default_rng(5200)
    ctx = new_ctx(kernel, ahead)
    # the automatic mode sends a small stream with a small index down its one-workgroup path: the other configurations of
    # kernel 0 get an index too large for it
    big_index = kernel == 0 and config != "small"
    try:
        k = 0
        for front, back, begin, end in K.hostile_cases():
            sizes = [64 + k % 3, 240 + (15 if k % 2 else 1)]
            if tile and k % 3 == 0:
                sizes.append(tile + 16 * (k % 2) + 33 * (k % 4))
            for n in sizes:
                s = K.edge_stream(rng, n, begin, end)
                want = K.expected_scan(orc, s)
                cap = (16385 if big_index else len(want[0])) + 3 + k % 2
                o = scan_offsets(k)
                if not arena:
                    o["rbsp"] = None
                tag = ("hbs_index_extract", config, "n", n, "front", front, "back", back[:4], "begins", begin, "ends", end, "offsets", o)
                got = scan_call(ctx, s, o, cap, (n + 16) if arena else None, front, back, fill=0x00 if k % 2 else 0xFF)
                same_scan(got, want, n, tag, strict_tail=False)
                witness(ctx, s, cap, arena, got, tag)
                k += 1
        assert k >= 96
    finally:
        ctx.close()
    RAN.add("hostile-" + config)


@pytest.mark.parametrize("config", [c for c in SCAN_CONFIGS if SCAN_CONFIGS[c][3]])
def test_hostile_bytes_behind_a_nearly_full_last_tile(orc, config):
    """the same surroundings behind streams that end 1 to 5 bytes short of a whole number of tiles: the kernels' last-tile
    paths (the event-sparse kernels read a padded copy of the last tile) see the bytes behind the end inside their last chunk"""
    kernel, ahead, arena, tile = SCAN_CONFIGS[config]
    rng = np.random.default_rng(5250)
    ctx = new_ctx(kernel, ahead)
    try:
        for k, (front, back, begin, end) in enumerate(K.hostile_cases()):
            n = (1 + k % 2) * tile - 1 - k % 5
            s = K.edge_stream(rng, n, begin, end)
            want = K.expected_scan(orc, s)
            cap = len(want[0]) + 3 + k % 2
            o = scan_offsets(k)
            if not arena:
                o["rbsp"] = None
            tag = ("hbs_index_extract", config, "n", n, "front", front, "back", back[:4], "begins", begin, "ends", end, "offsets", o)
            same_scan(scan_call(ctx, s, o, cap, (n + 16) if arena else None, front, back, fill=0x00 if k % 2 else 0xFF), want, n, tag, strict_tail=False)
    finally:
        ctx.close()
    RAN.add("hostile-tile-" + config)


# ---- hbs_emit_annexb ----------------------------------------------------------------------------------------------------------

EMIT_PATHS = {"auto": -1, "by-nals": 0, "three-step": 1, "arena-tiles": 2}
ARENA_ENDS = (b"\x00\x00", b"\x00", b"\x80")
ARENA_BACKS = (b"\x00", b"\x00\x00", b"\x03", b"\x01", b"\xff")
ARENA_FRONTS = (b"\x00\x00", b"\x00", b"\x00\x00\x00", b"\xff")


def emit_arena(rng, lens, end=b"\x80"):
    """an arena of NALs of these lengths: 20 % zeros in some, 00..03 at some first bytes, some ending in 00 00; the last bytes `end`"""
    lens = np.asarray(lens, dtype=np.int64)
    total = int(lens.sum())
    arena = rng.integers(1, 256, size=total, dtype=np.uint8)
    off = np.cumsum(lens) - lens
    arena[rng.random(total) < 0.003] = 0
    for k in range(0, len(lens), 3):
        if lens[k]:
            arena[off[k]] = k % 4
    for k in range(1, len(lens), 4):
        if lens[k] >= 2:
            arena[off[k] + lens[k] - 2: off[k] + lens[k]] = 0
    if total >= 16:
        for q in rng.integers(0, total - 8, size=total // 3000 + 2):
            arena[q:q + 3] = (0, 0, int(rng.integers(0, 4)))
    assert total >= len(end)
    arena[total - len(end):] = np.frombuffer(end, dtype=np.uint8)
    return arena, lens


def emit_index(lens, gaps, first_off=0):
    lens = np.asarray(lens, dtype=np.int64)
    gaps = np.asarray(gaps, dtype=np.int64)
    idx = np.zeros(len(lens), dtype=NAL_ENTRY)
    idx["end"] = np.cumsum(lens + gaps)
    idx["start"] = idx["end"] - lens
    idx["rbsp_off"] = np.cumsum(lens) - lens + first_off
    idx["rbsp_len"] = lens
    return idx


def emit_call(ctx, arena, idx, gap_mode, want, o, first_off=0, front=b"", back=b""):
    """hbs_emit_annexb on carved buffers, the output exactly len(want) bytes; the arena's first `first_off` bytes are nobody's.
    -> (out bytes, index_out entries, summary, damage)"""
    lead = np.full(first_off, 0, dtype=np.uint8)
    ca = G(first_off + len(arena), o["rbsp"], 0x00).put(np.concatenate([lead, arena])).hostile(front, back)
    ci = G(len(idx) * 32, o["index_in"]).put(idx)
    co = G(len(want), o["out"], prefill=0xC3)
    cx = G(len(idx) * 32, o["index_out"], prefill=0xC3)
    cm = G(64, o["summary"], prefill=0xEE)
    ctx.emit_annexb_async(ca.view, first_off + len(arena), ci.view, len(idx), gap_mode, co.view, cx.view, cm.view)
    sm = ctx.read_summary(cm.view).copy()
    return co.get(), cx.get().view(NAL_ENTRY), sm, damages(arena=ca, index_in=ci, out=co, index_out=cx, summary=cm)


def same_emit(got, want, idx, gaps, tag):
    out, io, sm, damage = got
    print(tag, "stream_bytes", int(sm["stream_bytes"]), "error", int(sm["error"]), damage)
    assert damage == "", (tag, damage)
    assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == len(want), (tag, sm, len(want))
    assert np.array_equal(out, want), (tag, "output bytes", int(np.flatnonzero(out != want)[0]))
    prev_end = np.concatenate([[0], io["end"][:-1].astype(np.int64)])
    assert np.array_equal(io["start"].astype(np.int64), prev_end + np.asarray(gaps)), (tag, "index_out.start")
    assert int(io["end"][-1]) == len(want), (tag, "index_out.end")
    assert np.array_equal(io["rbsp_len"], idx["rbsp_len"]) and np.array_equal(io["rbsp_off"], idx["rbsp_off"]), (tag, "index_out.rbsp_*")


def synth_gaps(n):
    return np.array([4 if k % 4 == 0 else 3 for k in range(n)], dtype=np.int64)


def emit_offsets(k):
    return dict(rbsp=rot(K.OFFS1, k), out=rot(K.OFFS1, k, 7, 3), index_in=rot(K.OFFS8, k, 3), index_out=rot((0, 8, 16, 24, 56), k), summary=rot(K.OFFS16, k, 5, 2))


@pytest.mark.parametrize("path", list(EMIT_PATHS))
def test_emit_at_every_alignment(orc, path):
    """the arena and the output at every offset 0..15 and at 48, 1008, 4080; gap modes 0 and 1; a handful of small NALs (the
    automatic path's one launch) and an arena of three tiles of 192 KiB; on the arena-tile path also with the first NAL where
    the ADDRESS is a multiple of 16 (so that the tiles run at every arena offset)"""
    rng = np.random.default_rng(5300)
    small = emit_arena(rng, rng.integers(0, 300, size=24))
    large = emit_arena(rng, np.concatenate([rng.integers(2000, 9000, size=110), [0, 1, 15, 16, 17, 70001]]))
    ctx = new_ctx(emit_path=EMIT_PATHS[path])
    try:
        k = 0
        for arena, lens in (small, large):
            gaps0 = rng.integers(3, 9, size=len(lens))
            for rep in range(len(K.OFFS1)):
                gap_mode = rep % 2
                gaps = synth_gaps(len(lens)) if gap_mode else gaps0
                o = emit_offsets(k)
                first_off = (-o["rbsp"]) % 16 if (path == "arena-tiles" and rep % 2 == 0) else 0
                idx = emit_index(lens, gaps, first_off)
                want = orc.emit_annexb(arena, emit_index(lens, gaps))
                tag = ("hbs_emit_annexb", path, "gap_mode", gap_mode, "arena", len(arena), "first rbsp_off", first_off, "offsets", o)
                same_emit(emit_call(ctx, arena, idx, gap_mode, want, o, first_off), want, idx, gaps, tag)
                if path == "arena-tiles" and len(arena) > 32768:
                    assert ctx.lib.hbs_ctx_last_emit_by_tiles(ctx.h) == (1 if (o["rbsp"] + first_off) % 16 == 0 else 0), tag
                note("hbs_emit_annexb", path, **o)
                k += 1
    finally:
        ctx.close()
    for ptr in ("rbsp", "out"):
        covered("hbs_emit_annexb", path, ptr, K.OFFS1)
    covered("hbs_emit_annexb", path, "index_out", (0, 8))
    RAN.add("emit-" + path)


def test_emit_tiles_eligible_by_address_not_by_offset(orc):
    """what no ordinary buffer reaches: the arena at 8 mod 16 with the first rbsp_off at 8 mod 16 -- the arena-tile kernel is
    eligible by ADDRESS while every offset counted from the buffer's start is odd -- and the mirror: base 0, rbsp_off 8"""
    rng = np.random.default_rng(5301)
    arena, lens = emit_arena(rng, np.concatenate([rng.integers(3000, 12000, size=80), [5, 0, 40000]]))
    gaps = rng.integers(3, 9, size=len(lens))
    want = orc.emit_annexb(arena, emit_index(lens, gaps))
    ctx = new_ctx(emit_path=2)
    try:
        for k, (base, first_off, tiles) in enumerate(((8, 8, 1), (0, 8, 0), (1032, 24, 1), (4088 - 4096 + 4096, 8, 1), (16, 8, 0))):
            for gap_mode in (0, 1):
                g = synth_gaps(len(lens)) if gap_mode else gaps
                w = orc.emit_annexb(arena, emit_index(lens, g)) if gap_mode else want
                o = dict(rbsp=base, out=rot(K.OFFS1, k, 7, 5), index_in=rot(K.OFFS8, k), index_out=8 * (k % 2), summary=rot(K.OFFS16, k))
                idx = emit_index(lens, g, first_off)
                tag = ("hbs_emit_annexb", "arena-tiles by address", "first rbsp_off", first_off, "gap_mode", gap_mode, "offsets", o)
                same_emit(emit_call(ctx, arena, idx, gap_mode, w, o, first_off), w, idx, g, tag)
                assert ctx.lib.hbs_ctx_last_emit_by_tiles(ctx.h) == tiles, tag
                note("hbs_emit_annexb", "arena-tiles", **o)
    finally:
        ctx.close()
    RAN.add("emit-by-address")


def test_emit_groups_kernel_at_every_alignment(orc):
    """~100-byte NALs in one stretch of the arena on the automatic path: the group kernel (64 NALs a wavefront, the stretch staged
    in LDS, the output written by aligned chunks)"""
    rng = np.random.default_rng(5302)
    lens = rng.integers(0, 201, size=30000)
    lens[:8] = (0, 1, 2, 15, 16, 17, 0, 0)
    arena, lens = emit_arena(rng, lens)
    gaps0 = rng.integers(3, 16, size=len(lens))
    wants = {0: orc.emit_annexb(arena, emit_index(lens, gaps0)), 1: orc.emit_annexb(arena, emit_index(lens, synth_gaps(len(lens))))}
    ctx = new_ctx(emit_path=-1)
    try:
        for k in range(len(K.OFFS1)):
            gap_mode = k % 2
            gaps = synth_gaps(len(lens)) if gap_mode else gaps0
            o = emit_offsets(k)
            idx = emit_index(lens, gaps)
            tag = ("hbs_emit_annexb", "groups", "gap_mode", gap_mode, "offsets", o)
            same_emit(emit_call(ctx, arena, idx, gap_mode, wants[gap_mode], o), wants[gap_mode], idx, gaps, tag)
            note("hbs_emit_annexb", "groups", **o)
    finally:
        ctx.close()
    for ptr in ("rbsp", "out"):
        covered("hbs_emit_annexb", "groups", ptr, K.OFFS1)
    RAN.add("emit-groups")


@pytest.mark.parametrize("path", list(EMIT_PATHS))
def test_emit_with_hostile_bytes_around_the_arena(orc, path):
    """00 / 00 00 / 03 / 01 behind rbsp_bytes, behind an arena that ends in 00 00 and in 00, and zeros in front of the arena:
    nothing at or behind d_rbsp + rbsp_bytes is read into the result"""
    rng = np.random.default_rng(5303)
    ctx = new_ctx(emit_path=EMIT_PATHS[path])
    try:
        k = 0
        for end in ARENA_ENDS:
            for back in ARENA_BACKS:
                for front in ARENA_FRONTS:
                    lens = rng.integers(1, 120, size=1 + k % 7) if k % 3 else rng.integers(500, 30000, size=9)
                    lens[-1] = max(int(lens[-1]), 8)
                    arena, lens = emit_arena(rng, lens, end)
                    gap_mode = k % 2
                    gaps = synth_gaps(len(lens)) if gap_mode else rng.integers(3, 9, size=len(lens))
                    o = emit_offsets(k)
                    first_off = (-o["rbsp"]) % 16 if k % 4 == 0 else 0
                    idx = emit_index(lens, gaps, first_off)
                    want = orc.emit_annexb(arena, emit_index(lens, gaps))
                    tag = ("hbs_emit_annexb", path, "arena ends", end, "behind it", back, "in front", front, "gap_mode", gap_mode, "offsets", o)
                    # (with a lead in front of the first NAL the hostile front lies in front of the lead: put it into the lead too)
                    same_emit(emit_call(ctx, arena, idx, gap_mode, want, o, first_off, front, back), want, idx, gaps, tag)
                    k += 1
    finally:
        ctx.close()
    RAN.add("emit-hostile-" + path)


# ---- hbs_filter_annexb --------------------------------------------------------------------------------------------------------

def filter_call(ctx, s, idx, o, rule=None, keep=None, front=b"", back=b"", plan_only=False, need=None):
    cs = G(len(s), o["stream"], HOSTILE_FILL).put(s).hostile(front, back)
    ci = G(len(idx) * 32, o["index"]).put(idx)
    ck = G(len(idx), o["keep"]).put(np.asarray(keep, dtype=np.uint8)) if keep is not None else None
    cm = G(64, o["summary"], prefill=0xEE)
    co = G(need if need else 64, o["out"], prefill=0xC3)                    # (nothing to write: a buffer that must stay as it is)
    cx = G(len(idx) * 32, o["index_out"], prefill=0xC3)
    if plan_only:
        ctx.filter_annexb_async(cs.view, len(s), ci.view, len(idx), None, None, cm.view, rule=rule, keep=ck.view if ck else None)
    else:
        ctx.filter_annexb_async(cs.view, len(s), ci.view, len(idx), co.view, cx.view, cm.view, rule=rule, keep=ck.view if ck else None, out_cap=need)
    sm = ctx.read_summary(cm.view).copy()
    return co.get(), cx.get(), sm, damages(stream=cs, index=ci, keep=ck, out=co, index_out=cx, summary=cm)


def test_filter_at_every_alignment(orc):
    """stream and output through the 16-byte set, index and output index through the 8-byte set, the keep mask at 0..15; a rule
    and a mask; keep-all, every other NAL, ~10 %; hostile bytes around the stream; the output exactly the planned size; the plan
    writes nothing but the summary"""
    rng = np.random.default_rng(5400)
    ctx = new_ctx()
    try:
        streams = []
        for size, mean in ((5000, 60), (300000, 900), (70000, 20)):
            idx = []
            while len(idx) < 10:
                s = F.random_stream(rng, size, mean)
                idx, _, _ = orc.index_extract(s)
            streams.append((s, idx))
        k = 0
        for rep in range(16):
            for s, idx in streams:
                mode = k % 4                    # 0: a rule that keeps everything, 1: a rule, 2: every other NAL, 3: ~10 %
                rule = None
                if mode == 0:
                    rule, keep = ctx.nal_filter(), np.ones(len(idx), bool)
                elif mode == 1:
                    r = dict(keep_types=int(rng.integers(0, 1 << 63)), max_temporal_id_plus1=int(rng.integers(2, 8)), max_layer_id=63, keep_short=bool(k & 4))
                    rule, keep = ctx.nal_filter(**r), F.rule_keep(s, idx, **r)
                elif mode == 2:
                    keep = (np.arange(len(idx)) % 2) == 0
                else:
                    keep = rng.random(len(idx)) < 0.1
                want_out, want_io, want_s = F.filter_ref(s, idx, keep)
                j = 2 * (k // 4) + k % 2                # the call's number among those with a rule / with a mask
                o = dict(stream=rot(K.OFFS16, j), out=rot(K.OFFS16, j, 3, 1), index=rot(K.OFFS8, j), index_out=rot(K.OFFS8, j, 3, 2),
                         keep=j % 16 if rule is None else None, summary=rot(K.OFFS16, j, 5, 2))
                front, back = rot(K.STREAM_FRONTS, k), rot(K.STREAM_BACKS, k)
                tag = ("hbs_filter_annexb", "rule" if rule is not None else "mask", "mode", mode, "stream", len(s), "nals", len(idx), "offsets", o)
                kw = dict(rule=rule, keep=None if rule is not None else keep, front=front, back=back)
                out, io, sm, damage = filter_call(ctx, s, idx, o, plan_only=True, **kw)
                assert damage == "" and (out == 0xC3).all() and (io == 0xC3).all(), (tag, "the plan wrote something", damage)
                assert int(sm["stream_bytes"]) == len(want_out) and int(sm["error"]) == 0, (tag, sm)
                out, io, sm, damage = filter_call(ctx, s, idx, o, need=len(want_out), **kw)
                print(tag, "stream_bytes", int(sm["stream_bytes"]), "kept", int(sm["nal_count"]), damage)
                assert damage == "", (tag, damage)
                for f, v in want_s.items():
                    assert int(sm[f]) == v, (tag, f, int(sm[f]), v)
                assert list(sm["reserved"]) == [0, 0, 0], tag
                assert np.array_equal(out, want_out) if len(want_out) else (out == 0xC3).all(), (tag, "output bytes")
                kept = len(want_io)
                assert np.array_equal(io[: kept * 32].view(NAL_ENTRY), want_io), (tag, "output index")
                assert (io[kept * 32:] == 0xC3).all(), (tag, "output index behind the kept NALs")
                note("hbs_filter_annexb", "rule" if rule is not None else "mask", **o)
                k += 1
    finally:
        ctx.close()
    for p in ("rule", "mask"):
        covered("hbs_filter_annexb", p, "stream", K.OFFS16)
        covered("hbs_filter_annexb", p, "out", K.OFFS16)
        covered("hbs_filter_annexb", p, "index", K.OFFS8)
        covered("hbs_filter_annexb", p, "index_out", K.OFFS8)
    covered("hbs_filter_annexb", "mask", "keep", range(16))
    RAN.add("filter")


# ---- header parse -------------------------------------------------------------------------------------------------------------

def parse_streams():
    """name -> (stream bytes, the NALs): a rich synthetic sequence, the ten_nal fixture, and a stream of more NALs than one
    workgroup takes"""
    from tests.hevc_synth import annexb, stream_4k30
    from tests.test_sim_parse_logic import sequence
    from tests import _orc
    out = {}
    nals = sequence(11) + sequence(12)
    out["rich"] = np.frombuffer(annexb(nals), dtype=np.uint8).copy()
    out["ten_nal"] = np.fromfile(os.path.join(HERE, "golden", "ten_nal.hevc"), dtype=np.uint8)
    big, count = stream_4k30(7, n_pictures=280, slices_per_picture=8, idr_every=40, payload_bytes=(40, 120), rich=True)
    assert count > 2048
    out["above-a-workgroup"] = np.frombuffer(big, dtype=np.uint8).copy()
    res = {}
    for name, s in out.items():
        idx, arena, why = _orc.oracle().index_extract(s)
        res[name] = (s, idx, arena, [bytes(s[int(a):int(b)]) for a, b in zip(idx["start"], idx["end"])])
    return res


@pytest.fixture(scope="module")
def parse_cases():
    from tests._parsecmp import oracle_pass
    out = {}
    for name, (s, idx, arena, nals) in parse_streams().items():
        out[name] = (s, idx, arena, oracle_pass(nals))
    return out


def under_study(ptrs, sets, rng):
    """[(offsets of every pointer)]: each pointer through its whole set in turn, the others drawn from theirs"""
    out = []
    for p in ptrs:
        for off in sets[p]:
            o = {q: int(rng.choice(sets[q])) for q in ptrs}
            o[p] = off
            out.append(o)
    return out


def compare_compact(cp, cc, cs, exp, tag):
    """the compact parse against the oracle's parser: the record and, for a slice, the sixteen members against the struct the
    oracle filled; a parameter set's struct whole"""
    from hevcbitstream_amd.api import COMPACT_FIELDS
    from tests import _orc
    where = {name: i for name, i, cnt in _orc.flat_fields("hevc_slice_header_t")}
    cols = np.array([where[f] for f in COMPACT_FIELDS])
    assert len(cp) == len(exp), tag
    for k, e in enumerate(exp):
        assert int(cp["rc"][k]) == e["rc"], (tag, k)
        assert [0, int(cp["nal_unit_type"][k]), int(cp["nal_layer_id"][k]), int(cp["nal_temporal_id_plus1"][k])] == list(e["nal"]), (tag, k)
        if e.get("kind") == "sh" and e["rc"] >= 0:
            got = np.array([cc[f][k] for f in COMPACT_FIELDS])
            assert np.array_equal(got, e["struct"][cols]), (tag, k, got, e["struct"][cols])
            assert int(cp["slice_data_size"][k]) == e["slice_data"][0], (tag, k)
        elif e.get("kind") in ("vps", "sps", "pps"):
            size = _orc.layout()[_orc.STRUCT_TYPES[e["kind"]]]["size"]
            off = int(cp["struct_off"][k])
            assert np.array_equal(cs[off: off + size].view(np.int32), e["struct"]), (tag, k, e["kind"])


def parse_inputs(name, case, o):
    s, idx, arena, exp = case
    n = len(idx)
    cr = G(len(arena), o["rbsp"], 0x00).put(arena).hostile(b"\x00\x00\x01", b"\x00\x00\x03\xff")
    ci = G(n * 32, o["index"]).put(idx)
    return n, cr, ci


def which_cases(k):
    return ("rich", "ten_nal", "above-a-workgroup") if k % 9 == 0 else ("rich", "ten_nal")


def test_parse_headers_at_every_alignment(parse_cases):
    from hevcbitstream_amd.api import PARSED
    from tests._parsecmp import compare
    rng = np.random.default_rng(5500)
    sets = dict(rbsp=K.OFFS16, index=K.OFFS16, parsed=K.OFFS16, structs=K.OFFS16, summary=K.OFFS16)
    ctx = new_ctx()
    try:
        for k, o in enumerate(under_study(list(sets), sets, rng)):
            for name in which_cases(k):
                n, cr, ci = parse_inputs(name, parse_cases[name], o)
                cp = G(n * 32, o["parsed"], prefill=0xC3)
                cm = G(64, o["summary"], prefill=0xEE)
                ctx.parse_headers_async(cr.view, ci.view, n, cp.view, None, cm.view)
                need = int(ctx.read_summary(cm.view)["reserved"][0])
                st = G(need, o["structs"], prefill=0xC3)
                ctx.parse_headers_async(cr.view, ci.view, n, cp.view, st.view, cm.view)
                sm = ctx.read_summary(cm.view)
                tag = ("hbs_parse_headers", name, "offsets", o)
                damage = damages(rbsp=cr, index=ci, parsed=cp, structs=st, summary=cm)
                print(tag, "struct bytes", need, "error", int(sm["error"]), damage)
                assert damage == "" and int(sm["error"]) == 0, (tag, damage, sm)
                s, idx, arena, exp = parse_cases[name]
                try:
                    compare(cp.get().view(PARSED), st.get(), arena, idx, exp)
                except AssertionError as e:
                    raise AssertionError("%r: %s" % (tag, e))
                note("hbs_parse_headers", name, **o)
    finally:
        ctx.close()
    for p in sets:
        covered("hbs_parse_headers", "rich", p, sets[p])
    RAN.add("parse")


def test_parse_headers_compact_at_every_alignment(parse_cases):
    from hevcbitstream_amd.api import COMPACT, PARSED
    rng = np.random.default_rng(5501)
    sets = dict(rbsp=K.OFFS16, index=K.OFFS16, parsed=K.OFFS16, compact=K.OFFS16, structs=K.OFFS16, summary=K.OFFS16)
    ctx = new_ctx()
    try:
        for k, o in enumerate(under_study(list(sets), sets, rng)):
            for name in which_cases(k):
                n, cr, ci = parse_inputs(name, parse_cases[name], o)
                cp = G(n * 32, o["parsed"], prefill=0xC3)
                cc = G(n * 64, o["compact"], prefill=0xC3)
                cm = G(64, o["summary"], prefill=0xEE)
                ctx.parse_compact_async(cr.view, ci.view, n, cp.view, cc.view, None, cm.view)
                need = int(ctx.read_summary(cm.view)["reserved"][0])
                st = G(need, o["structs"], prefill=0xC3)
                ctx.parse_compact_async(cr.view, ci.view, n, cp.view, cc.view, st.view, cm.view)
                sm = ctx.read_summary(cm.view)
                tag = ("hbs_parse_headers_compact", name, "offsets", o)
                damage = damages(rbsp=cr, index=ci, parsed=cp, compact=cc, structs=st, summary=cm)
                print(tag, "struct bytes", need, "error", int(sm["error"]), damage)
                assert damage == "" and int(sm["error"]) == 0, (tag, damage, sm)
                compare_compact(cp.get().view(PARSED), cc.get().view(COMPACT), st.get(), parse_cases[name][3], tag)
                note("hbs_parse_headers_compact", name, **o)
    finally:
        ctx.close()
    for p in sets:
        covered("hbs_parse_headers_compact", "rich", p, sets[p])
    RAN.add("compact")


def test_index_parse_at_every_alignment(parse_cases):
    from hevcbitstream_amd.api import PARSED
    from tests._parsecmp import compare
    rng = np.random.default_rng(5502)
    sets = dict(stream=K.OFFS16, index=K.OFFS8, parsed=K.OFFS16, structs=K.OFFS16, payload_off=K.OFFS8, scan_summary=K.OFFS16, parse_summary=K.OFFS16)
    ctx = new_ctx()
    try:
        for k, o in enumerate(under_study(list(sets), sets, rng)):
            for name in which_cases(k):
                s, idx, arena, exp = parse_cases[name]
                n = len(idx)
                cap = n + 1 + k % 2
                cs = G(len(s), o["stream"], HOSTILE_FILL).put(s).hostile(rot(K.STREAM_FRONTS, k), rot(K.STREAM_BACKS, k))
                ci = G(cap * 32, o["index"], prefill=0xC3)
                cp = G(n * 32, o["parsed"], prefill=0xC3)
                cy = G(n * 8, o["payload_off"], prefill=0xC3)
                m1, m2 = G(64, o["scan_summary"], prefill=0xEE), G(64, o["parse_summary"], prefill=0xEE)
                assert ctx.index_parse_async(cs.view, ci.view, cap, cp.view, None, m1.view, m2.view) == n        # the plan: the struct arena's size
                st = G(int(ctx.read_summary(m2.view)["reserved"][0]), o["structs"], prefill=0xC3)
                ci.view.fill_(0xC3)
                got = ctx.index_parse_async(cs.view, ci.view, cap, cp.view, st.view, m1.view, m2.view, payload_off=cy.view)
                s1, s2 = ctx.read_summary(m1.view), ctx.read_summary(m2.view)
                tag = ("hbs_index_parse", name, "offsets", o)
                damage = damages(stream=cs, index=ci, parsed=cp, structs=st, payload_off=cy, scan_summary=m1, parse_summary=m2)
                print(tag, "nals", got, "errors", int(s1["error"]), int(s2["error"]), damage)
                assert damage == "" and got == n and int(s1["error"]) == 0 and int(s2["error"]) == 0, (tag, damage, s1, s2)
                entries = ci.get().view(NAL_ENTRY)
                for f in FIELDS:
                    assert np.array_equal(entries[f][:n], idx[f]), (tag, f)
                assert not entries[n:].view(np.uint8).any(), (tag, "index behind the NALs found")
                try:
                    compare(cp.get().view(PARSED), st.get(), arena, idx, exp)
                except AssertionError as e:
                    raise AssertionError("%r: %s" % (tag, e))
                note("hbs_index_parse", name, **o)
    finally:
        ctx.close()
    for p in sets:
        covered("hbs_index_parse", "rich", p, sets[p])
    RAN.add("index-parse")


# ---- access units -------------------------------------------------------------------------------------------------------------

def au_records(ctx, parse_cases):
    """name -> (index, parsed, compact, structs) as host records: the rich sequence and ten_nal through the compact parse on
    ordinary buffers (which the tests above pin on the oracle), and fabricated records of more NALs than a workgroup's 2048"""
    import torch
    from tests.test_gpu_au import fabricate
    from hevcbitstream_amd.api import COMPACT, PARSED
    out = {}
    for name in ("rich", "ten_nal"):
        s, idx, arena, exp = parse_cases[name]
        d_arena = torch.from_numpy(np.concatenate([arena, np.zeros(16, np.uint8)])).cuda()
        d_idx = torch.from_numpy(idx.view(np.uint8).copy()).cuda()
        cp, cc, cs = ctx.parse_headers_compact(d_arena, d_idx, len(idx))
        out[name] = (idx, cp.view(PARSED), cc.view(COMPACT), cs.cpu().numpy())
    off = int(ctx.lib.hbs_au_sps_poc_offset())
    out["above-a-workgroup"] = fabricate(np.random.default_rng(5600), 5000, 0.6, 0.3, off=off)
    return out


def test_access_units_and_au_keep_at_every_alignment(parse_cases):
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(5601)
    sets = dict(index=K.OFFS16, parsed=K.OFFS16, compact=K.OFFS16, au=K.OFFS16, structs=K.OFFS4, nal_au=K.OFFS4, carry_out=K.OFFS4, summary=K.OFFS16)
    keep_sets = dict(nal_au=K.OFFS4, parsed=K.OFFS8, keep=tuple(range(16)))
    ctx = new_ctx()
    try:
        recs = au_records(ctx, parse_cases)
        off = int(ctx.lib.hbs_au_sps_poc_offset())
        wants = {name: R.access_units(r[0], r[1], r[2], r[3], off) for name, r in recs.items()}
        for k, o in enumerate(under_study(list(sets), sets, rng)):
            for name in (("rich", "ten_nal", "above-a-workgroup") if k % 5 == 0 else ("rich", "ten_nal")):
                index, parsed, compact, structs = recs[name]
                want_au, want_nal_au, want_carry, want_s = wants[name]
                n, aus = len(parsed), len(want_au)
                ci, cp, cc = G(n * 32, o["index"]).put(index), G(n * 32, o["parsed"]).put(parsed), G(n * 64, o["compact"]).put(compact)
                st = G(len(structs), o["structs"]).put(structs)
                ca = G(aus * 64, o["au"], prefill=0xC3)
                cn = G(n * 4, o["nal_au"], prefill=0xC3)
                cy = G(16, o["carry_out"], prefill=0xC3)
                cm = G(64, o["summary"], prefill=0xEE)
                tag = ("hbs_access_units", name, "offsets", o)
                assert ctx.access_units_async(ci.view, cp.view, cc.view, st.view, n, None, 0, None, None, cm.view) == 0, tag
                plan = ctx.read_summary(cm.view).copy()
                assert int(plan["nal_count"]) == aus and int(plan["error"]) == 0, (tag, plan)
                assert (ca.get() == 0xC3).all() and (cn.get() == 0xC3).all() and (cy.get() == 0xC3).all(), (tag, "the plan wrote an output")
                assert ctx.access_units_async(ci.view, cp.view, cc.view, st.view, n, ca.view, aus, cn.view, cy.view, cm.view) == 0, tag
                sm = ctx.read_summary(cm.view).copy()
                damage = damages(index=ci, parsed=cp, compact=cc, structs=st, au=ca, nal_au=cn, carry_out=cy, summary=cm)
                print(tag, "aus", int(sm["nal_count"]), "error", int(sm["error"]), damage)
                assert damage == "" and int(sm["error"]) == 0, (tag, damage, sm)
                assert (int(sm["nal_count"]), int(sm["nal_found"]), int(sm["reserved"][0]), int(sm["reserved"][1]), int(sm["stream_bytes"])) == \
                    (want_s["nal_count"], want_s["nal_found"], want_s["pictures"], want_s["cvs_starts"], want_s["stream_bytes"]), (tag, sm, want_s)
                assert int(sm["rbsp_bytes"]) == 0 and int(sm["stop_reason"]) == 0 and int(sm["reserved"][2]) == 0, (tag, sm)
                got = ca.get().view(hbs.ACCESS_UNIT)
                for f in want_au.dtype.names:
                    assert np.array_equal(got[f], want_au[f]), (tag, f)
                assert np.array_equal(cn.get().view(np.uint32), want_nal_au), (tag, "nal_au")
                assert cy.get().view(hbs.AU_CARRY).tolist() == want_carry.tolist(), (tag, "carry")
                note("hbs_access_units", name, **o)
        for k, o in enumerate(under_study(list(keep_sets), keep_sets, rng)):
            for name in (("rich", "above-a-workgroup") if k % 4 == 0 else ("rich",)):
                index, parsed, compact, structs = recs[name]
                want_au, want_nal_au, _, _ = wants[name]
                n, aus = len(parsed), len(want_au)
                first, count, sets_flag = (aus // 3, max(aus // 3, 1), bool(k % 2))
                cn = G(n * 4, o["nal_au"]).put(want_nal_au)
                cp = G(n * 32, o["parsed"]).put(parsed)
                ck = G(n, o["keep"], prefill=0xC3)
                ctx.au_keep_async(cn.view, cp.view, n, first, count, ck.view, sets_flag)
                got = ck.get()
                tag = ("hbs_au_keep", name, "aus", (first, count), "param sets", sets_flag, "offsets", o)
                damage = damages(nal_au=cn, parsed=cp, keep=ck)
                print(tag, "kept", int(got.sum()), damage)
                assert damage == "", (tag, damage)
                assert np.array_equal(got, R.au_keep(want_nal_au, parsed, first, count, sets_flag)), tag
                note("hbs_au_keep", name, **o)
    finally:
        ctx.close()
    for p in sets:
        covered("hbs_access_units", "rich", p, sets[p])
    for p in keep_sets:
        covered("hbs_au_keep", "rich", p, keep_sets[p])
    assert 8 in TABLE[("hbs_au_keep", "rich", "parsed")]
    RAN.add("au")


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_the_nearest_misalignment_is_refused_and_nothing_is_written(orc, parse_cases):
    """for every pointer with a host check: + 8 on a 16-byte pointer, + 4 on an 8-byte one, + 2 and + 1 on a 4-byte one give
    HBS_E_ARG, and every output, the summary included, still holds its prefill"""
    from tests.test_gpu_au import fabricate
    rng = np.random.default_rng(5700)
    ctx = new_ctx()
    refused = []

    def untouched(tag, **bufs):
        import torch
        torch.cuda.synchronize()
        for name, (c, byte) in bufs.items():
            assert c.damage() == "" and (c.get() == byte).all(), (tag, name, "written by a refused call", c.damage())
        refused.append(tag)

    try:
        s = stream_of(rng, 1, 20000, 0)
        idx, arena, _ = orc.index_extract(s)
        n = len(idx)
        # hbs_index_extract
        for ptr, bump in (("stream", 8), ("rbsp", 8), ("index", 4)):
            o = dict(stream=16, index=8, rbsp=48, summary=32)
            o[ptr] += bump
            cs, ci = G(len(s), o["stream"]).put(s), G((n + 2) * 32, o["index"], prefill=0xC3)
            cr, cm = G(len(s) + 16, o["rbsp"], prefill=0xC3), G(64, o["summary"], prefill=0xEE)
            failed_with(E_ARG, ctx.index_extract_async, cs.view, ci.view, n + 2, cr.view, cm.view)
            untouched(("hbs_index_extract", ptr, bump), index=(ci, 0xC3), rbsp=(cr, 0xC3), summary=(cm, 0xEE))
        # hbs_filter_annexb
        for ptr, bump in (("stream", 8), ("out", 8), ("index", 4), ("index_out", 4)):
            o = dict(stream=16, index=8, out=48, index_out=24, summary=32)
            o[ptr] += bump
            cs, ci = G(len(s), o["stream"]).put(s), G(n * 32, o["index"]).put(idx)
            co, cx, cm = G(len(s), o["out"], prefill=0xC3), G(n * 32, o["index_out"], prefill=0xC3), G(64, o["summary"], prefill=0xEE)
            failed_with(E_ARG, ctx.filter_annexb_async, cs.view, len(s), ci.view, n, co.view, cx.view, cm.view, rule=ctx.nal_filter())
            untouched(("hbs_filter_annexb", ptr, bump), out=(co, 0xC3), index_out=(cx, 0xC3), summary=(cm, 0xEE))
        # hbs_parse_headers / hbs_parse_headers_compact / hbs_index_parse: the struct arena (and the scan's pointers)
        ps, pidx, parena, _ = parse_cases["rich"]
        pn = len(pidx)
        cr, ci = G(len(parena), 16).put(parena), G(pn * 32, 32).put(pidx)
        for entry in ("hbs_parse_headers", "hbs_parse_headers_compact"):
            cp, cc, st, cm = G(pn * 32, 48, prefill=0xC3), G(pn * 64, 80, prefill=0xC3), G(1 << 20, 16 + 8, prefill=0xC3), G(64, 32, prefill=0xEE)
            if entry == "hbs_parse_headers":
                failed_with(E_ARG, ctx.parse_headers_async, cr.view, ci.view, pn, cp.view, st.view, cm.view)
            else:
                failed_with(E_ARG, ctx.parse_compact_async, cr.view, ci.view, pn, cp.view, cc.view, st.view, cm.view)
            untouched((entry, "structs", 8), parsed=(cp, 0xC3), compact=(cc, 0xC3), structs=(st, 0xC3), summary=(cm, 0xEE))
        for ptr, bump in (("stream", 8), ("index", 4), ("structs", 8)):
            o = dict(stream=16, index=8, structs=48)
            o[ptr] += bump
            cs, ci2 = G(len(ps), o["stream"]).put(ps), G((pn + 2) * 32, o["index"], prefill=0xC3)
            cp, st = G(pn * 32, 48, prefill=0xC3), G(1 << 20, o["structs"], prefill=0xC3)
            m1, m2 = G(64, 32, prefill=0xEE), G(64, 80, prefill=0xEE)
            failed_with(E_ARG, ctx.index_parse_async, cs.view, ci2.view, pn + 2, cp.view, st.view, m1.view, m2.view)
            untouched(("hbs_index_parse", ptr, bump), index=(ci2, 0xC3), parsed=(cp, 0xC3), structs=(st, 0xC3), scan_summary=(m1, 0xEE), parse_summary=(m2, 0xEE))
        # hbs_access_units / hbs_au_keep
        index, parsed, compact, structs = fabricate(rng, 300, 0.6, 0.3, off=int(ctx.lib.hbs_au_sps_poc_offset()))
        m = len(parsed)
        for ptr, bump in (("index", 8), ("parsed", 8), ("compact", 8), ("au", 8), ("nal_au", 2), ("nal_au", 1), ("carry_out", 2), ("carry_out", 1),
                          ("structs", 2), ("structs", 1)):
            o = dict(index=16, parsed=32, compact=48, au=80, nal_au=4, carry_out=12, structs=60)
            o[ptr] += bump
            ci, cp, cc = G(m * 32, o["index"]).put(index), G(m * 32, o["parsed"]).put(parsed), G(m * 64, o["compact"]).put(compact)
            st = G(len(structs), o["structs"]).put(structs)
            ca, cn, cy, cm = G(m * 64, o["au"], prefill=0xC3), G(m * 4, o["nal_au"], prefill=0xC3), G(16, o["carry_out"], prefill=0xC3), G(64, 16, prefill=0xEE)
            assert ctx.access_units_async(ci.view, cp.view, cc.view, st.view, m, ca.view, m, cn.view, cy.view, cm.view) == E_ARG, (ptr, bump)
            untouched(("hbs_access_units", ptr, bump), au=(ca, 0xC3), nal_au=(cn, 0xC3), carry_out=(cy, 0xC3), summary=(cm, 0xEE))
        for ptr, bump in (("nal_au", 2), ("nal_au", 1), ("parsed", 4)):
            o = dict(nal_au=4, parsed=8)
            o[ptr] += bump
            cn, cp, ck = G(m * 4, o["nal_au"]).put(np.zeros(m, np.uint32)), G(m * 32, o["parsed"]).put(parsed), G(m, 5, prefill=0xC3)
            failed_with(E_ARG, ctx.au_keep_async, cn.view, cp.view, m, 0, 1, ck.view)
            untouched(("hbs_au_keep", ptr, bump), keep=(ck, 0xC3))
    finally:
        ctx.close()
    print("refused with HBS_E_ARG, outputs untouched:", refused)
    assert len(refused) == 3 + 4 + 2 + 3 + 10 + 3
    RAN.add("refusals")


# ---- the table ----------------------------------------------------------------------------------------------------------------

def expected_rows():
    rows = []
    for config, (kernel, ahead, arena, tile) in SCAN_CONFIGS.items():
        rows += [("hbs_index_extract", config, p) for p in ("stream", "index", "summary") + (("rbsp",) if arena else ())]
    for path in list(EMIT_PATHS) + ["groups"]:
        rows += [("hbs_emit_annexb", path, p) for p in ("rbsp", "out", "index_in", "index_out", "summary")]
    for p in ("rule", "mask"):
        rows += [("hbs_filter_annexb", p, q) for q in ("stream", "out", "index", "index_out", "summary")]
    rows.append(("hbs_filter_annexb", "mask", "keep"))
    for name in ("rich", "ten_nal", "above-a-workgroup"):
        rows += [("hbs_parse_headers", name, p) for p in ("rbsp", "index", "parsed", "structs", "summary")]
        rows += [("hbs_parse_headers_compact", name, p) for p in ("rbsp", "index", "parsed", "compact", "structs", "summary")]
        rows += [("hbs_index_parse", name, p) for p in ("stream", "index", "parsed", "structs", "payload_off", "scan_summary", "parse_summary")]
        rows += [("hbs_access_units", name, p) for p in ("index", "parsed", "compact", "au", "structs", "nal_au", "carry_out", "summary")]
    for name in ("rich", "above-a-workgroup"):
        rows += [("hbs_au_keep", name, p) for p in ("nal_au", "parsed", "keep")]
    return rows


def test_zz_table_of_cases():
    """entry point x kernel or path x pointer x offsets exercised, printed once per run.  A whole run of this module must have
    filled every row (the per-test assertions above have checked each row's offsets against the pointer's accepted set)."""
    print("\n%-26s %-18s %-14s %s" % ("entry point", "kernel / path", "pointer", "offsets from a 4096-byte boundary"))
    for (entry, path, ptr), offs in sorted(TABLE.items()):
        print("%-26s %-18s %-14s %s" % (entry, path, ptr, " ".join(str(x) for x in sorted(offs))))
    whole = {"filter", "parse", "compact", "index-parse", "au", "refusals", "emit-groups", "emit-by-address"}
    whole |= {p + c for c in SCAN_CONFIGS for p in ("scan-", "clear-", "hostile-")} | {p + c for c in EMIT_PATHS for p in ("emit-", "emit-hostile-")}
    whole |= {"hostile-tile-" + c for c in SCAN_CONFIGS if SCAN_CONFIGS[c][3]}
    if RAN >= whole:
        missing = [r for r in expected_rows() if r not in TABLE]
        assert not missing, ("combinations never exercised", missing)
    else:
        print("(a partial run: %d of %d groups of cases ran; the table is complete only for a whole run of the module)" % (len(RAN & whole), len(whole)))
