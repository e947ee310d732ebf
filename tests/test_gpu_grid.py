"""The persistent kernels with many tiles per workgroup.  Their grids are what the GPU holds (~512 workgroups), so a workgroup
only reaches its second tile on streams of tens of MiB, and every patterned stream of the other modules is smaller than that.
hbs_ctx_reserve_workgroups cuts the scan kernels' grids to a few workgroups, which then carry LDS, dense tiles, count-ahead
entries and look-back chains from tile to tile; the arena-tile emit kernel gets the same from one arena of several hundred MiB.
Every answer against the oracle, field for field and byte for byte."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._orc import NAL_ENTRY
from tests.test_gpu_index_parse import both_ways, same
from tests.hevc_synth import stream_4k30

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = 192 << 10
# the tile of each scan kernel: LDS image (2), event-sparse (4; 5 with an arena runs it) and its 24-row geometry (6)
TILE = {2: 64 << 10, 4: 192 << 10, 6: 96 << 10}
FIELDS = ("start", "end", "rbsp_off", "rbsp_len", "status")
SMALL_GRIDS = (1, 2, 5)
HBS_E_CAPACITY = -4


def _nals(rng, s, lo, hi, step_lo, step_hi):
    """start codes of 3 and 4 bytes with a header byte, every step_lo..step_hi bytes of s[lo:hi]"""
    at = lo
    while at + 8 < hi:
        sc = (0, 0, 1) if rng.randint(3) else (0, 0, 0, 1)
        s[at:at + len(sc)] = sc
        s[at + len(sc)] = 0x40
        at += int(rng.randint(step_lo, step_hi))


def _no_empty_nals(s):
    """a start code right behind a start code is an empty NAL, which ends the walk: put a byte between them"""
    while True:
        z = (s[:-5] == 0) & (s[1:-4] == 0) & (s[2:-3] == 1) & (s[3:-2] == 0) & (s[4:-1] == 0) & (s[5:] <= 1)
        at = np.nonzero(z)[0]
        if not len(at):
            return s
        s[at + 3] = 0x77


def _fuzz(rng, n):
    """the shape of test_fuzz_multi_tile: random bytes with start codes, EPBs, zero runs and errors sprinkled in"""
    s = rng.randint(0, 256, size=n).astype(np.uint8)
    for pat, cnt in ((b"\x00\x00\x01", n // 5000), (b"\x00\x00\x00\x01", n // 9000), (b"\x00\x00\x03", n // 700),
                     (b"\x00\x00\x00", n // 40000), (b"\x00\x00\x02", n // 200000 + 1), (b"\x00" * 70, 3)):
        for at in rng.randint(0, n - 80, size=cnt):
            s[at:at + len(pat)] = np.frombuffer(pat, dtype=np.uint8)
    return _no_empty_nals(s)


def _sparse(rng, n):
    """coded-video-like: NALs of 3-20 KB of plain bytes"""
    s = rng.randint(1, 256, size=n).astype(np.uint8)
    _nals(rng, s, 0, n, 3000, 20000)
    return s


def _tile_edges(rng):
    """the patterns of test_tile_edges at every tile border of the three geometries (multiples of 64 and 96 KiB) over 42
    tiles of 192 KiB: start codes and 00 00 | 03 split by the border, and zero runs longer than a tile across two borders"""
    n = 42 * T + 777
    s = rng.randint(4, 256, size=n).astype(np.uint8)
    s[0:4] = (0, 0, 1, 0x40)
    pats = [bytes([0, 0, 1]), bytes([0, 0, 0, 1]), bytes([0, 0, 3]), bytes([0, 0, 3, 0, 0, 3]), bytes([0, 0, 0]),
            bytes([0, 0, 2]), bytes([0, 0, 3, 9]), bytes([0] * 9)]
    split = [(bytes([0, 0, 1, 0x42]), 2), (bytes([0, 0, 3, 1]), 2), (bytes([0, 0, 0, 1, 0x40]), 1), (bytes([0, 0, 0, 1, 0x40]), 3),
             (bytes([0, 0, 3, 0]), 3), (bytes([0, 0, 1, 0x26]), 1)]
    edges = sorted(set(range(64 << 10, n, 64 << 10)) | set(range(96 << 10, n, 96 << 10)))
    for k, edge in enumerate(edges):
        p, before = split[k % len(split)]                 # p[:before] in front of the border, the rest behind it
        s[edge - before:edge - before + len(p)] = np.frombuffer(p, dtype=np.uint8)
        p = pats[rng.randint(len(pats))]
        at = edge + 8 + int(rng.randint(0, 40)) if rng.randint(2) else edge - 8 - len(p) - int(rng.randint(0, 40))
        s[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    s[10 * T - 100:11 * T + 100] = 0                       # a zero run longer than a tile over two borders of every geometry
    s[11 * T + 100:11 * T + 104] = (0, 0, 1, 0x40)
    s[30 * T + 5:31 * T + 70001] = 0                       # odd ends inside tiles
    return s


def _sparse_and_dense(rng):
    """40 tiles of sparse NALs; every 5th tile of 192 KiB is dense: 10 % zeros, tiny NALs or 00 00 03 padding"""
    n = 40 * T + 4321
    s = _sparse(rng, n)
    for k, t in enumerate(range(2, 40, 5)):
        a, b = t * T, (t + 1) * T
        if k % 3 == 0:
            s[a:b][rng.random_sample(T) < 0.10] = 0
        elif k % 3 == 1:
            _nals(rng, s, a, b, 20, 40)
        else:
            s[a + 7:b - 7] = np.tile(np.array([0, 0, 3], dtype=np.uint8), T // 3)[:T - 14]
    return _no_empty_nals(s)


def _small_nals(rng):
    """NALs of ~200 bytes over 64 tiles of 96 KiB: the 24-row geometry's case"""
    n = (6 << 20) + 999
    s = rng.randint(1, 256, size=n).astype(np.uint8)
    s[rng.random_sample(n) < 0.002] = 0
    p = 3
    while p < n - 8:
        if p & 2:
            s[p:p + 4] = (0, 0, 1, 0x42)
        else:
            s[p:p + 5] = (0, 0, 0, 1, 0x26)
        p += int(rng.randint(150, 251))
    return s


def _scan_streams():
    """name -> (stream, runs without an arena too, index_cap or None)"""
    rng = np.random.RandomState(2301)
    out = {}
    out["fuzz-12mib"] = (_fuzz(rng, (12 << 20) + 12345), True, None)
    out["tile-edges"] = (_tile_edges(rng), False, None)
    out["sparse-and-dense"] = (_sparse_and_dense(rng), True, None)
    out["nals-200"] = (_small_nals(rng), True, None)
    s = _sparse(rng, (8 << 20) + 17)
    s[int(0.8 * len(s)) + 333:][:6] = (0, 0, 1, 0, 0, 1)   # an empty NAL in a late tile: the walk stops there
    out["empty-nal-late"] = (s, False, None)
    s = _sparse(rng, (8 << 20) + 29)
    s[len(s) - 300_000:] = 0                               # the stream ends in a zero run over two tiles
    out["ends-in-zeros"] = (s, False, None)
    return out


def _oracle(orc, s):
    """(entries, arena, stop_reason, nal_found, rbsp_bytes) the call must report.  A walk the oracle stops at an empty NAL: the
    summary still counts every start code of the stream and every RBSP byte behind them (hbs_summary), which is the oracle's
    walk of the bytes behind the empty NAL's start code added on -- the empty NAL itself is one more NAL of no bytes."""
    idx, arena, why = orc.index_extract(s)
    found, kept = len(idx), len(arena)
    if why == 1:
        p = int(idx["end"][-1]) if len(idx) else 0
        assert bytes(s[p:p + 6]) == b"\x00\x00\x01\x00\x00\x01"
        rest, rest_arena, _ = orc.index_extract(s[p + 3:])
        found, kept = len(idx) + 1 + len(rest), len(arena) + len(rest_arena)
    return idx, arena, why, found, kept


@pytest.fixture(scope="module")
def streams(orc):
    """each stream, its device copy and the oracle's answer, once"""
    import torch
    out = {}
    for name, (s, no_arena, _) in _scan_streams().items():
        out[name] = (s, torch.from_numpy(s).cuda(), _oracle(orc, s), no_arena)
    return out


@pytest.fixture(scope="module")
def full_grids():
    """variant -> (workgroups, workgroups per CU) of the uncut grid"""
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    try:
        out = {}
        for v in (2, 4, 6):
            c.set_kernel(v)
            out[v] = c.grid()
        print("\nfull grids (workgroups, per CU):", out)
        return out
    finally:
        c.close()


@pytest.mark.parametrize("variant", [2, 4, 6], ids=["lds-image-kernel", "sparse-kernel", "sparse-kernel-24-rows"])
def test_reserve_workgroups_cuts_the_grid(variant):
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    try:
        c.set_kernel(variant)
        full, per_cu = c.grid()
        assert full >= 4 and per_cu >= 1
        for spare in (1, full - 3, full - 1, full, 10 ** 6):
            c.reserve_workgroups(spare)
            assert c.grid() == (max(full - spare, 1), per_cu), spare
        c.reserve_workgroups(0)
        assert c.grid() == (full, per_cu)
        with pytest.raises(hbs.HbsError):
            c.reserve_workgroups(-1)
        assert c.grid() == (full, per_cu)                  # a refused call changes nothing
        c.reserve_workgroups(full - 2)
        other = 4 if variant != 4 else 2
        c.set_kernel(other)
        c.set_kernel(variant)
        assert c.grid() == (2, per_cu)                     # the cut survives set_kernel
    finally:
        c.close()


def _check(got, want, ref, tag, cap=None):
    """got / ref: (entries, arena or None, summary) of the call and of the uncut grid's call; want: the oracle's"""
    g_idx, g_arena, s = got
    w_idx, w_arena, why, w_found, w_kept = want
    r_idx, r_arena, r = ref
    n = len(w_idx) if cap is None else cap
    assert int(s["error"]) == (0 if cap is None else HBS_E_CAPACITY), (tag, s)
    if cap is None:
        assert int(s["stop_reason"]) == why, tag
    assert int(s["nal_count"]) == n and len(g_idx) == n, (tag, int(s["nal_count"]), n)
    assert int(s["nal_found"]) == w_found, (tag, int(s["nal_found"]), w_found)
    if g_arena is not None:
        assert int(s["rbsp_bytes"]) == w_kept, (tag, int(s["rbsp_bytes"]), w_kept)
    for f in ("nal_count", "nal_found", "rbsp_bytes", "stop_reason"):
        assert int(s[f]) == int(r[f]), (tag, f, "against the uncut grid")
    for f in FIELDS:
        assert np.array_equal(g_idx[f], w_idx[f][:n]), (tag, f)
    if g_arena is not None:                               # the RBSP of the NALs delivered
        tot = int(w_idx["rbsp_off"][n - 1] + w_idx["rbsp_len"][n - 1]) if n else 0
        assert np.array_equal(g_arena[:tot], w_arena[:tot]), (tag, "arena")


def _runs(streams):
    """(stream name, want_rbsp, index_cap) of every call a configuration makes; the last is cut by its index capacity"""
    out = []
    for name, (s, d, want, no_arena) in streams.items():
        out.append((name, True, None))
        if no_arena:
            out.append((name, False, None))
    out.append(("nals-200", True, len(streams["nals-200"][2][0]) * 7 // 8))
    return out


def _call(c, streams, name, arena, cap):
    # (the default capacity, as test_gpu_scan's: the index needs room for every start code, those behind an empty NAL too)
    return c.index_extract(streams[name][1], index_cap=cap, want_rbsp=arena)


@pytest.mark.parametrize("variant", [0, 2, 4, 5, 6],
                         ids=["automatic", "lds-image-kernel", "sparse-kernel", "index-only-passes", "sparse-kernel-24-rows"])
def test_scan_parity_with_a_cut_grid(streams, full_grids, variant):
    """grids of 1, 2, 5 and full - 1 workgroups, tickets and device-exclusive first tiles, count-ahead off and on (kernels 4
    and 0): every call equals the oracle and the uncut grid's call; at 1-5 workgroups every workgroup takes >= 4 tiles"""
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    runs = _runs(streams)
    reach = {}
    try:
        c.set_kernel(variant)
        ref, picked = {}, {}
        for name, arena, cap in runs:                      # the uncut grid, defaults: against the oracle, and the reference below
            got = _call(c, streams, name, arena, cap)
            ref[name, arena, cap] = got
            picked[name, arena, cap] = c.last_kernel()
            _check(got, streams[name][2], got, (variant, "full", name, arena, cap), cap)
            if variant:
                assert picked[name, arena, cap] == (4 if variant == 5 and arena else variant)
        for grid in SMALL_GRIDS + ("full-1",):
            for exclusive in (0, 1):
                c.set_device_exclusive(exclusive)
                for ahead in ((0, 2) if variant in (0, 4) else (1,)):
                    c.set_count_ahead(ahead)
                    for name, arena, cap in runs:
                        kernel = picked[name, arena, cap]
                        tiled = 4 if kernel == 5 and arena else kernel
                        if grid == "full-1":
                            spare = 1
                        elif tiled in TILE:
                            spare = full_grids[tiled][0] - grid
                        else:                              # kernel 5 without an arena: its wave count goes down by 4 per slot
                            spare = full_grids[4][0] - grid
                        c.reserve_workgroups(spare)
                        if variant:                        # (grid() of kernel 5 pinned reports the LDS-image kernel's grid)
                            shown = 2 if variant == 5 else variant
                            assert c.grid()[0] == max(full_grids[shown][0] - spare, 1)
                        if tiled in TILE:
                            wgs = max(full_grids[tiled][0] - spare, 1)
                            if grid != "full-1":
                                per_wg = math.ceil(len(streams[name][0]) / TILE[tiled]) / wgs
                                assert per_wg >= 4, (variant, grid, name, per_wg)
                                reach[tiled, grid] = min(reach.get((tiled, grid), per_wg), per_wg)
                        tag = (variant, grid, exclusive, ahead, name, arena, cap)
                        _check(_call(c, streams, name, arena, cap), streams[name][2], ref[name, arena, cap], tag, cap)
                        assert c.last_kernel() == kernel, (tag, c.last_kernel())
        print("\nkernel %d: fewest tiles per workgroup (kernel, grid): %s" %
              (variant, {k: round(v, 1) for k, v in sorted(reach.items(), key=str)}))
    finally:
        c.close()


_K5_WORKER = r"""
import math, sys, numpy as np
sys.path.insert(0, %r)
import torch, hevcbitstream_amd as hbs
from tests import _orc
from tests.test_gpu_grid import _k5_stream
orc = _orc.oracle()
s = _k5_stream()
want, _, why = orc.index_extract(s)
d = torch.from_numpy(s).cuda()
ctx = hbs.Context(0)
ctx.set_kernel(5)
ctx.reserve_workgroups(10 ** 6)                        # launch_scan_index5 then keeps its floor of 64 wavefronts
for exclusive in (0, 1):
    ctx.set_device_exclusive(exclusive)
    got, arena, sm = ctx.index_extract(d, index_cap=len(want) + 16, want_rbsp=False)
    assert arena is None and int(sm["error"]) == 0 and int(sm["stop_reason"]) == why, (exclusive, sm)
    assert int(sm["nal_count"]) == len(got) == len(want) and int(sm["nal_found"]) == len(want), (exclusive, len(got), len(want))
    for f in ("start", "end", "rbsp_off", "rbsp_len", "status"):
        assert np.array_equal(got[f], want[f]), (exclusive, f)
    assert ctx.last_kernel() == 5
print("ok", math.ceil(len(s) / (64 * 1024)) / 64)        # tiles of 64 KiB over those 64 wavefronts (computed, not read back)
"""


def _k5_stream():
    """32 MiB: sparse NALs, fuzz, a stretch of padding, one of tiny NALs, one of 10 % zeros, and a zero run at the end"""
    rng = np.random.RandomState(2305)
    n = (32 << 20) + 4321
    s = _sparse(rng, n)
    s[(4 << 20):(8 << 20)] = _fuzz(rng, 4 << 20)
    s[(9 << 20) + 5:(12 << 20) + 3] = np.tile(np.array([0, 0, 3], dtype=np.uint8), (1 << 20) + 1)[:(3 << 20) - 2]
    _nals(rng, s, 14 << 20, 15 << 20, 20, 40)
    s[(17 << 20):(19 << 20)][rng.random_sample(2 << 20) < 0.10] = 0
    for m in range(64 << 10, n - 8, 64 << 10):         # start codes across the 64 KiB tile borders
        o = m + int(rng.randint(-4, 2))
        s[o:o + 5] = (0, 0, 0, 1, 0x42) if m % 3 else (0, 0, 1, 0, 0x40)
    s[n - 200_000:] = 0
    return _no_empty_nals(s)


def test_index_only_kernel_takes_many_tiles_per_wavefront():
    """kernel 5 with every workgroup slot reserved -- its launcher's floor of 64 wavefronts -- and tiles of 64 rows
    (HBS5_TILE_ROWS is read once: a process of its own): 513 tiles, 8 a wavefront by that floor"""
    env = dict(os.environ)
    env["HBS5_TILE_ROWS"] = "64"
    r = subprocess.run([sys.executable, "-c", _K5_WORKER % os.path.dirname(HERE)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().split()[-2] == "ok", (r.stdout[-2000:], r.stderr[-4000:])
    per_wave = float(r.stdout.strip().split()[-1])
    print("\nkernel 5: %.1f tiles per wavefront (computed from the 64-wavefront floor)" % per_wave)
    assert per_wave >= 4


def test_index_parse_and_host_ingest_on_one_workgroup(streams, orc):
    """hbs_index_parse and hbs_index_extract_host run the scan too: at a grid of 1 they give what they give at full grid"""
    import hevcbitstream_amd as hbs
    full, one = hbs.Context(0), hbs.Context(0)
    try:
        one.reserve_workgroups(10 ** 6)
        stream, count = stream_4k30(5, n_pictures=180, slices_per_picture=8, idr_every=30, payload_bytes=(3000, 9000), rich=True)
        assert len(stream) >= 40 * T
        a, b = both_ways(one, stream)
        same(a, b)
        assert len(a[1]) == count
        a_full, b_full = both_ways(full, stream)
        same(a_full, b)
        same(a, b_full)
        assert np.array_equal(a[4], a_full[4])
        s, _, want, _ = streams["fuzz-12mib"]
        w_idx, w_arena, why, _, _ = want
        got_idx, got_arena, sm = one.index_extract_host(s, window_bytes=1 << 20)
        assert int(sm["error"]) == 0 and int(sm["stop_reason"]) == why and len(got_idx) == len(w_idx), sm
        for f in FIELDS:
            assert np.array_equal(got_idx[f], w_idx[f]), f
        tot = int(w_idx["rbsp_off"][-1] + w_idx["rbsp_len"][-1])
        assert np.array_equal(got_arena[:tot], w_arena[:tot])
    finally:
        full.close()
        one.close()


# ---- the arena-tile emit kernel ---------------------------------------------------------------------------------------------

def fake_index(lens, gaps):
    """test_gpu_emit.fake_index without the loop: NALs back to back in the arena, gaps[k] bytes in front of NAL k"""
    lens = np.asarray(lens, dtype=np.int64)
    gaps = np.asarray(gaps, dtype=np.int64)
    idx = np.zeros(len(lens), dtype=NAL_ENTRY)
    idx["end"] = np.cumsum(lens + gaps)
    idx["start"] = idx["end"] - lens
    idx["rbsp_off"] = np.cumsum(lens) - lens
    idx["rbsp_len"] = lens
    return idx


def _emit_arena(cus):
    """an arena of >= 3 x (2 workgroups a CU) tiles of 192 KiB: runs of 300 NALs of 64-192 bytes (at most one run per tile, so
    no tile passes the kernel's 1024 NAL starts), NALs of ~10 KiB with empty ones among them, NALs of 30-90 KiB that are dense
    (10 % zeros, 00 00 03 padding, zeros), one NAL whose zero runs cover several tiles.  Every NAL begins with 40 and ends in
    80 but for one in 50 that ends in 00 00.  Returns (arena, lens, gaps, ends_in_zeros)."""
    rng = np.random.default_rng(2310)
    target = 3 * cus * 2 * T + 5 * T + 777
    lens, kinds = [], []
    total, block = 0, 0
    while total < target:
        k = block % 4
        if k == 0:
            ln = rng.integers(64, 193, size=300)
        elif k == 2:
            ln = rng.integers(30_000, 90_001, size=3)
        else:
            ln = rng.integers(9000, 11_501, size=15)
            ln[rng.integers(0, 15, size=2)] = 0
        if block == 400:
            ln = np.array([1_500_001])
            kinds.append(np.full(1, 5))
        else:
            kinds.append(np.full(len(ln), 1 + (block // 4) % 3 if k == 2 else 0))
        lens.append(ln)
        total += int(ln.sum())
        block += 1
    lens = np.concatenate(lens).astype(np.int64)
    kinds = np.concatenate(kinds)
    arena = rng.integers(1, 256, size=int(lens.sum()), dtype=np.uint8)
    off = np.cumsum(lens) - lens
    for o, ln, kind in zip(off[kinds > 0], lens[kinds > 0], kinds[kinds > 0]):
        body = arena[o + 1:o + ln - 1]
        if kind == 1:
            body[rng.random(len(body)) < 0.10] = 0
        elif kind == 2:
            body[:] = np.tile(np.array([0, 0, 3], dtype=np.uint8), len(body) // 3 + 1)[:len(body)]
        elif kind == 3:
            body[100:-100] = 0
        else:                                             # the long NAL: zeros over ~2.3 and ~1.3 tiles, odd ends
            body[100_003:100_003 + 450_001] = 0
            body[900_007:900_007 + 250_000] = 0
    full = lens > 0
    arena[off[full]] = 0x40
    arena[off[full] + lens[full] - 1] = 0x80
    zz = np.zeros(len(lens), dtype=bool)
    zz[::50] = True
    zz &= lens >= 3
    arena[off[zz] + lens[zz] - 1] = 0
    arena[off[zz] + lens[zz] - 2] = 0
    gaps = rng.integers(3, 9, size=len(lens))
    return arena, lens, gaps, zz


def test_emit_arena_tiles_with_many_tiles_per_workgroup(orc):
    """one arena of ~300 MiB through every emit path, gap modes 0 and 1, tickets and device-exclusive first tiles, dense tiles
    counted ahead or not: bytes against the oracle, output index against the kernel by NALs; then an arena without empty NALs
    and without NALs that end in 00 00, emitted by arena tiles and scanned again on one workgroup, gives itself back"""
    import torch
    import hevcbitstream_amd as hbs
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    arena, lens, gaps, zz = _emit_arena(cus)
    # (k3_tiles' grid comes from an occupancy query inside the library; 2 workgroups a CU -- 77 KiB of LDS each -- is assumed
    # here, not read back, so the reach below is computed from that assumption)
    assert len(arena) >= 3 * cus * 2 * T
    print("\nemit: %d MiB arena, %d NALs, %.1f tiles of 192 KiB per workgroup if 2 run a CU" %
          (len(arena) >> 20, len(lens), len(arena) / T / (2 * cus)))
    idx0 = fake_index(lens, gaps)
    idx1 = fake_index(lens, [4 if k % 4 == 0 else 3 for k in range(len(lens))])   # what gap_mode 1 writes
    want = {0: orc.emit_annexb(arena, idx0), 1: orc.emit_annexb(arena, idx1)}
    d_arena = torch.from_numpy(arena).cuda()
    c = hbs.Context(0)
    try:
        for gap_mode in (0, 1):
            by_nals = None
            for exclusive in (0, 1):
                c.set_device_exclusive(exclusive)
                for path, ahead in ((0, 1), (-1, 1), (1, 1), (2, 0), (2, 2)):
                    c.set_emit_path(path)
                    c.set_count_ahead(ahead)
                    got, got_idx = c.emit_annexb(d_arena, idx0, gap_mode)
                    tag = (gap_mode, exclusive, path, ahead)
                    assert len(got) == len(want[gap_mode]) and np.array_equal(got, want[gap_mode]), tag
                    if by_nals is None:
                        by_nals = got_idx
                    assert np.array_equal(got_idx, by_nals), (tag, "output index")
                    if path == 2:
                        assert c.lib.hbs_ctx_last_emit_by_tiles(c.h) == 1, tag
                    del got, got_idx
        c.set_device_exclusive(0)
        c.set_count_ahead(1)
        # the way back: no empty NAL (it ends the walk), no NAL that ends in 00 00 (the scan ends it at the zeros)
        clean = arena.copy()
        off = np.cumsum(lens) - lens
        clean[off[zz] + lens[zz] - 1] = 0x80
        keep = lens > 0
        idx_c = fake_index(lens[keep], gaps[keep])
        c.set_emit_path(2)
        out, out_idx = c.emit_annexb(torch.from_numpy(clean).cuda(), idx_c, 0)
        assert c.lib.hbs_ctx_last_emit_by_tiles(c.h) == 1
        assert np.array_equal(out, orc.emit_annexb(clean, idx_c))
        c.set_emit_path(-1)
        c.reserve_workgroups(10 ** 6)
        got_idx, got_arena, s = c.index_extract(torch.from_numpy(out).cuda(), index_cap=len(idx_c) + 16)
        assert int(s["error"]) == 0 and int(s["nal_count"]) == len(idx_c), s
        for f in ("start", "end"):
            assert np.array_equal(got_idx[f], out_idx[f]), f
        for f in ("rbsp_off", "rbsp_len"):
            assert np.array_equal(got_idx[f], idx_c[f]), f
        assert np.array_equal(got_arena, clean)
    finally:
        c.close()
