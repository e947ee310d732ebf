"""The layouts, plans and checkers of tests/_big.py on the CPU, at scale 65536 (the "4 GiB boundary" is 64 KiB): the references'
own bytes pass every checker, every corruption that a lost high word could cause fails it, the plan forms of the references give
the bytes the references gave before they were split (digests recorded under tests/golden/), and the full-scale layouts have the
properties tests/test_gpu_above_4gib.py relies on (from the tables alone)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from tests import _auins_ref as I
from tests import _big as G
from tests import _rtp_ref as R
from tests import _rtp_unpack_ref as U
from tests import _segments as S
from tests import _ts_ref as D
from tests import _tsmux_ref as T

SCALE = 65536
BD = (1 << 32) // SCALE
CAN = 0xC3
RTP_A = R.params(max_payload=1188, framing=2, seq=65000, ts_base=(1 << 32) - 200000)
RTP_A0 = dict(RTP_A, framing=0)
RTP_B = R.params(max_payload=8947, framing=0, seq=7)
TS_188 = T.params(packet_bytes=188, flags=T.PCR | T.PSI_AT_IRAP, cc_es=9, pcr_lead=1000)
TS_192 = T.params(packet_bytes=192, flags=0, cc_es=3)
INS = I.AUD | I.PARAM_SETS
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "big_ref_digests.json")


class Case:
    """one call on one layout: the source, the plan's segments and tables, the reference's bytes, and the checker bound to
    everything but the output and (for the table corruptions) the tables"""

    def __init__(self, name, src, want, tables, checker, packets=None, head=0):
        self.name, self.src, self.want, self.tables, self.checker = name, src, want, tables, checker
        self.segs, self.total = want[0], want[-1]["stream_bytes"]
        self.good = S.materialise(self.segs, self.total, src)
        self.packets, self.head = packets, head            # packet offsets and where the counter byte stands, for the packet corruptions

    def check(self, out, tables=None):
        import torch
        t = self.tables if tables is None else tables
        return self.checker(torch.from_numpy(out), *t, self.want[-1], torch.from_numpy(self.src), self.want)


@functools.lru_cache(maxsize=None)
def world():
    A, B = G.layout_a(SCALE), G.layout_b(SCALE)
    sa, sb = G.make_stream(A, "cpu").numpy(), G.make_stream(B, "cpu").numpy()
    cases = []
    pts = G.rtp_times(A)
    for prm in (RTP_A, RTP_A0):
        want = R.plan(A.total, A.hdr, A.index, A.nal_au, A.n_aus, pts, prm)
        c = Case("rtp_pack A framing %d" % prm["framing"], sa, want, (want[1], want[2]), G.check_pack, R.packet_offsets(want[1], want[2], prm),
                 prm["framing"] + 3)
        c.prm = prm
        cases.append(c)
        uw = G.unpack_plan(A, int(want[3]["nal_count"]), prm["ts_base"], pts)
        cases.append(Case("rtp_unpack A framing %d" % prm["framing"], sa, uw, uw[1:4], G.check_unpack))
    want = R.plan(B.total, B.hdr, B.index, B.nal_au, 6, None, RTP_B)
    c = Case("rtp_pack B", sb, want, (want[1], want[2]), G.check_pack, R.packet_offsets(want[1], want[2], RTP_B), 3)
    c.prm = RTP_B
    cases.append(c)
    uw = G.unpack_plan(B, int(want[3]["nal_count"]), 0, np.zeros(6, dtype=np.uint64))
    cases.append(Case("rtp_unpack B", sb, uw, uw[1:4], G.check_unpack))
    tp, td = G.times(A)
    for prm in (TS_188, TS_192):
        want = T.plan(A.total, A.au, tp, td, prm)
        Bp = prm["packet_bytes"]
        c = Case("ts_mux A %d" % Bp, sa, want, (want[1],), G.check_mux, np.arange(want[2]["nal_count"] + 1, dtype=np.uint64) * np.uint64(Bp),
                 (4 if Bp == 192 else 0) + 3)
        c.prm = prm
        cases.append(c)
        dw = G.demux_plan(A, tp, td, want[1], want[2]["reserved"][1])
        cases.append(Case("ts_demux A %d" % Bp, sa, dw, (dw[1],), G.check_demux))
    for first in (0, A.cross + 1):
        want = I.plan(A.total, A.index, A.parsed, A.au, A.nal_au, first, A.n_aus, INS)
        c = Case("au_insert A from AU %d" % first, sa, want, want[1:5], G.check_insert)
        c.first = first
        cases.append(c)
    return A, B, sa, sb, cases


def case(name):
    return next(c for c in world()[4] if c.name == name)


NAMES = ["rtp_pack A framing 2", "rtp_pack A framing 0", "rtp_unpack A framing 2", "rtp_unpack A framing 0", "rtp_pack B", "rtp_unpack B",
         "ts_mux A 188", "ts_mux A 192", "ts_demux A 188", "ts_demux A 192", "au_insert A from AU 0", "au_insert A from AU %d" % (G.layout_a(SCALE).cross + 1)]
PACKETS = [n for n in NAMES if n.startswith(("rtp_pack", "ts_mux"))]


def rejected(c, out, tables=None):
    with pytest.raises(AssertionError):
        c.check(out, tables)


def out_offset_of(segs, s):
    """the output byte that carries source byte s (the first, where it is copied twice)"""
    for seg in segs:
        if seg[0] == "copy" and seg[2] <= s < seg[2] + seg[3]:
            return seg[1] + s - seg[2]
        if seg[0] == "run" and seg[2]["src"] <= s < seg[2]["src"] + seg[2]["n"] * seg[2]["F"]:
            r = seg[2]
            i, within = divmod(s - r["src"], r["F"])
            return seg[1] + i * r["P"] + r["H"] + within
    raise AssertionError("source byte %d is nowhere in the output" % s)


# ---- the streams and the layouts ---------------------------------------------------------------------------------------------------

def test_the_cpu_stream_is_what_a_scan_finds(orc):
    A, B, sa, sb, _ = world()
    got, _, _ = orc.index_extract(sa)
    assert np.array_equal(got, A.index)
    assert np.count_nonzero(sa == 0) == int(A.gap.sum()) - len(A.index) + int((A.hdr[:, 0] == 0).sum())          # no zero byte but ours
    got, _, _ = orc.index_extract(sb)
    assert np.array_equal(got["start"], B.index["start"]) and np.array_equal(got["end"], B.index["end"])
    assert np.array_equal(R.nal_headers(sa, A.index), A.hdr) and np.array_equal(R.nal_headers(sb, B.index), B.hdr)


def test_the_scaled_layouts_cross_their_boundary():
    A, B, sa, sb, cases = world()
    assert A.boundary == BD and A.total > BD and int(A.index["start"][A.large]) > BD
    for c in cases:
        if not c.name.endswith("from AU %d" % (A.cross + 1)):
            assert c.total > BD, c.name
    assert G.giant_output(B, RTP_B["max_payload"], 0) > BD
    assert int(A.au["unit_begin"][A.cross + 1]) > BD
    assert T.AU_IRAP == I.A.IRAP


def test_layout_properties_at_full_scale():
    """from the tables alone: totals above 2^32, the source boundary among the small AUs, every NAL below 2^31, the outputs of
    every call of tests/test_gpu_above_4gib.py above 2^32, layout B's giant NAL alone above 2^32 of output"""
    A, B = G.layout_a(1), G.layout_b(1)
    two32 = 1 << 32
    assert A.boundary == two32 and A.total > two32 + (600 << 20) and int((A.index["end"] - A.index["start"]).max()) < 1 << 31
    assert 41 < A.cross < 100 and int(A.au["unit_begin"][A.cross]) < two32 < int(A.au["unit_end"][A.cross])
    assert two32 - (128 << 10) <= int(A.au["unit_end"][40]) <= two32 - (64 << 10)
    pts = G.rtp_times(A)
    want = R.plan(A.total, A.hdr, A.index, A.nal_au, A.n_aus, pts, RTP_A)
    assert want[3]["stream_bytes"] > two32 and S.tiles(want[0], want[3]["stream_bytes"]) and int(want[1][A.large]) > two32
    ts = (RTP_A["ts_base"] + pts) & np.uint64(R.M32)
    assert len(set((ts < 1 << 31).tolist())) == 2                                # the timestamps wrap
    assert G.unpack_plan(A, 1, 0, pts)[4]["stream_bytes"] > two32
    tp, td = G.times(A)
    for prm in (TS_188, TS_192):
        segs, au_packet, s = T.plan(A.total, A.au, tp, td, prm)
        assert s["stream_bytes"] > two32 and S.tiles(segs, s["stream_bytes"])
        assert (int(au_packet[41]) - int(au_packet[40])) * prm["packet_bytes"] > two32          # the big AU's packets alone
        dw = G.demux_plan(A, tp, td, au_packet, s["reserved"][1])
        assert dw[2]["stream_bytes"] > two32 and (dw[1]["out_off"] > two32).sum() > 40
    whole = I.plan(A.total, A.index, A.parsed, A.au, A.nal_au, 0, A.n_aus, INS)
    assert whole[5]["stream_bytes"] > A.total and whole[5]["reserved"][1] > 30
    part = I.plan(A.total, A.index, A.parsed, A.au, A.nal_au, A.cross + 1, A.n_aus, INS)
    assert int(A.au["unit_begin"][A.cross + 1]) > two32 and part[5]["reserved"][1] > 15
    assert any(seg[0] == "copy" and seg[2] < two32 < seg[1] for seg in whole[0])          # sets from below 2^32 to above it
    assert any(seg[0] == "copy" and seg[2] < two32 for seg in part[0])
    assert B.total > two32 and G.giant_output(B, RTP_B["max_payload"], RTP_B["framing"]) > two32
    bw = R.plan(B.total, B.hdr, B.index, B.nal_au, 6, None, RTP_B)
    assert int(bw[1][B.giant + 1]) - int(bw[1][B.giant]) == G.giant_output(B, RTP_B["max_payload"], 0)
    assert (12 + RTP_B["max_payload"]) % 16 == 15                                # the alignment of a full packet rotates


# ---- the references' bytes pass; the derived plans are what the independent loops give ------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_reference_bytes_pass(name):
    c = case(name)
    assert c.check(c.good.copy()) == c.total == len(c.good)


def test_pack_plans_materialise_to_the_reference():
    A, B, sa, sb, _ = world()
    pts = G.rtp_times(A)
    for prm in (RTP_A, RTP_A0):
        ref = R.pack(sa, A.index, A.nal_au, A.n_aus, pts, prm)
        c = case("rtp_pack A framing %d" % prm["framing"])
        assert np.array_equal(ref[0], c.good) and ref[3] == c.want[3]
    ref = T.mux(sa, A.au, *G.times(A), TS_188)
    assert np.array_equal(ref[0], case("ts_mux A 188").good)
    ref = I.au_insert(sa, A.index, A.parsed, A.au, A.nal_au, 0, A.n_aus, INS)
    assert np.array_equal(ref[0], case("au_insert A from AU 0").good)


def test_unpack_plan_is_the_receivers():
    A, B, sa, sb, _ = world()
    for pack_name, name, L in (("rtp_pack A framing 2", "rtp_unpack A framing 2", A), ("rtp_pack A framing 0", "rtp_unpack A framing 0", A),
                               ("rtp_pack B", "rtp_unpack B", B)):
        p, u = case(pack_name), case(name)
        off, size = G.packet_table(p.want[1], p.want[2], p.prm)
        ref = U.unpack(p.good, off, size, U.params(startcode_bytes=4), out_cap=1 << 40)
        assert ref["summary"] == u.want[4], (ref["summary"], u.want[4])
        assert np.array_equal(ref["out"], u.good) and np.array_equal(ref["index"], u.want[1])
        assert np.array_equal(ref["nal_au"], u.want[2]) and np.array_equal(ref["au_ts"], u.want[3])


def test_demux_plan_is_the_receivers():
    A = world()[0]
    for prm in (TS_188, TS_192):
        m, d = case("ts_mux A %d" % prm["packet_bytes"]), case("ts_demux A %d" % prm["packet_bytes"])
        out, pes, s = D.demux(m.good.tobytes(), prm["packet_bytes"], prm["pid"])
        assert s == d.want[2], (s, d.want[2])
        assert np.array_equal(out, d.good) and np.array_equal(pes, d.want[1])
    # with the foreign packets: the same bytes, the packet numbers moved
    m, d = case("ts_mux A 188"), case("ts_demux A 188")
    import torch
    big, moved = G.with_foreign_packets(torch.from_numpy(m.good))
    n = len(m.good) // 188
    assert big.numel() == (n + -(-n // 9)) * 188 and moved(0) == 1 and moved(8) == 9 and moved(9) == 11
    rows = big.numpy().reshape(-1, 188)
    assert (rows[::10, 1] == 0x1F).all() and (rows[::10, 2] == 0xFF).all() and np.array_equal(np.delete(rows, np.s_[::10], axis=0).reshape(-1), m.good)
    out, pes, s = D.demux(big.numpy().tobytes(), 188, TS_188["pid"])
    assert np.array_equal(out, d.good) and np.array_equal(pes["packet"], moved(d.want[1]["packet"].astype(np.int64))) and s == d.want[2]


def test_insert_rescan_needs_no_exception(orc):
    A, _, sa, _, _ = world()
    for first in (0, A.cross + 1):
        c = case("au_insert A from AU %d" % first)
        exc, junk, short = I.rescan_exceptions(sa, A.index, A.au, first, A.n_aus, c.good, c.want[1], c.want[2])
        assert exc is None and not junk and not short
        got, _, _ = orc.index_extract(c.good)
        assert np.array_equal(got, c.want[1])


def test_packet_table_is_the_loops():
    def loop(nal_off, nal_packet, prm):
        out = []
        for k in range(len(nal_off) - 1):
            for i in range(int(nal_packet[k + 1] - nal_packet[k])):
                out.append(int(nal_off[k]) + i * (prm["framing"] + 12 + prm["max_payload"]))
        return np.array(out + [int(nal_off[-1])], dtype=np.uint64)
    rng = np.random.default_rng(3)
    for n, mp, fr in ((0, 100, 0), (1, 4, 2), (60, 19, 2), (300, 100, 0), (40, 1188, 2)):
        prm = R.params(max_payload=mp, framing=fr)
        stream, index, nal_au, n_aus, pts = R.random_case(rng, n, max_nal=700)
        _, nal_off, nal_packet, s = R.pack(stream, index, nal_au, n_aus, pts, prm)
        want = loop(nal_off, nal_packet, prm)
        got = R.packet_offsets(nal_off, nal_packet, prm)
        assert got.dtype == want.dtype and np.array_equal(got, want) and len(got) == s["nal_count"] + 1
        off, size = G.packet_table(nal_off, nal_packet, prm)
        assert np.array_equal(off, want[:-1] + np.uint64(fr)) and np.array_equal(off + size, want[1:])


def run_behind_the_boundary(c):
    """the last strided run -> (its segment, the offset of its last packet, the offset of the packet behind it: the NAL's or the
    AU's last).  Both lie behind the boundary, but in layout B, whose giant NAL passes it by less than a packet at this scale:
    there the last packet begins below the boundary and ends behind it."""
    r = [seg for seg in c.segs if seg[0] == "run"][-1]
    inside, last = r[1] + (r[2]["n"] - 1) * r[2]["P"], r[1] + r[2]["n"] * r[2]["P"]
    assert (last > BD and inside > BD) or (c.name.endswith(" B") and c.total - last < r[2]["P"] + 3000 and c.total > BD)
    return r, inside, last


# ---- corruptions ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_one_payload_byte_flipped_behind_the_boundary(name):
    A, B, _, _, _ = world()
    c = case(name)
    L = B if name.endswith(" B") else A
    k = L.giant if L is B else L.large
    s = int(L.index["end"][k]) - (int(L.index["end"][k]) - max(int(L.index["start"][k]), L.boundary)) // 2
    assert s > L.boundary
    o = out_offset_of(c.segs, s)
    assert o > BD or "from AU" in name
    bad = c.good.copy()
    bad[o] ^= 0x10
    rejected(c, bad)


@pytest.mark.parametrize("name", NAMES)
def test_source_offsets_that_lost_their_high_word(name):
    """every output byte at or behind the boundary taken from source offset - boundary"""
    c = case(name)
    wrapped = c.src.copy()
    wrapped[BD:] = c.src[:len(c.src) - BD]
    bad = S.materialise(c.segs, c.total, wrapped)
    if c.total > BD:                                                 # (the range that begins above the boundary reads nothing below it)
        bad[:BD] = c.good[:BD]
    assert not np.array_equal(bad, c.good)
    rejected(c, bad)


@pytest.mark.parametrize("name", [n for n in NAMES if "from AU 0" in n or "from AU" not in n])
def test_output_offsets_that_lost_their_high_word(name):
    """the bytes due behind the boundary written at offset - boundary, over the output's beginning"""
    c = case(name)
    bad = np.full(c.total, CAN, dtype=np.uint8)
    bad[:BD] = c.good[:BD]
    bad[:c.total - BD] = c.good[BD:]
    rejected(c, bad)


@pytest.mark.parametrize("name", PACKETS)
def test_one_counter_off_by_one_behind_the_boundary(name):
    """a sequence number or a continuity counter, in a packet of a strided run and in one that is given by itself"""
    c = case(name)
    r, inside, last = run_behind_the_boundary(c)
    assert inside in c.packets and last in c.packets
    for o in (inside, last):
        bad = c.good.copy()
        low = bad[o + c.head] & 15
        bad[o + c.head] = (bad[o + c.head] & 0xF0) | ((low + 1) & 15)
        rejected(c, bad)


@pytest.mark.parametrize("name", [n for n in PACKETS if n.startswith("rtp_pack")])
def test_one_fu_header_with_s_or_e_wrong(name):
    c = case(name)
    fr = c.prm["framing"]
    r, inside, last = run_behind_the_boundary(c)
    first = r[1] - r[2]["P"]
    for o, flip in ((first, 0x80), (inside, 0x80), (inside, 0x40), (last, 0x40)):
        bad = c.good.copy()
        assert bad[o + fr + 12] >> 1 & 63 == 49
        bad[o + fr + 14] ^= flip
        rejected(c, bad)
    assert c.good[first + fr + 14] & 0xC0 == 0x80 and c.good[inside + fr + 14] & 0xC0 == 0 and c.good[last + fr + 14] & 0xC0 == 0x40


@pytest.mark.parametrize("name", NAMES)
def test_one_table_entry_without_its_high_bit(name):
    c = case(name)
    done = 0
    for which, table in enumerate(c.tables):
        for field in (table.dtype.names or (None,)):
            col = table[field] if field else table
            if field not in (None, "start", "end", "out_off", "unit_begin", "unit_end", "packet"):
                continue
            bit = BD
            hit = np.flatnonzero(col.astype(np.uint64) & np.uint64(bit))
            if not len(hit):
                top = int(col.max())
                if top == 0:
                    continue
                bit = 1 << (top.bit_length() - 1)                      # (packet numbers: the highest bit there is)
                hit = np.flatnonzero(col.astype(np.uint64) & np.uint64(bit))
            tables = [t.copy() for t in c.tables]
            t = tables[which][field] if field else tables[which]
            t[hit[len(hit) // 2]] = int(col[hit[len(hit) // 2]]) & ~bit
            rejected(c, c.good, tables)
            done += 1
    assert done >= 1


def test_a_plan_that_skips_a_region_is_refused():
    import torch
    c = case("ts_mux A 188")
    segs = [seg for seg in c.segs if not (seg[0] == "run" and seg[1] > BD)]
    with pytest.raises(AssertionError):
        G.check_segments(torch.from_numpy(c.good), torch.from_numpy(c.src), segs, c.total)


# ---- the references before and after they were split into plan and bytes ---------------------------------------------------------

def plain(x):
    """dicts, lists and numpy scalars as plain Python, so that their repr is the same everywhere"""
    if isinstance(x, dict):
        return sorted((k, plain(v)) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return None if x is None else int(x)


def digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(plain(p)).encode())
    return h.hexdigest()


def reference_digests(R, T, I):
    """the outputs of the three references (the modules given) on the seeds tests/test_rtp_abi.py, tests/test_tsmux_abi.py and
    tests/test_auins_abi.py use, as digests"""
    out = {}
    for seed in (5, 9, 11, 13):
        rng = np.random.default_rng(seed)
        for it in range(6):
            prm = R.params(max_payload=int(rng.choice([4, 5, 19, 100, 1188])), framing=int(rng.choice([0, 2])), flags=int(rng.integers(0, 2)),
                           seq=int(rng.integers(0, 65536)), ts_base=int(rng.integers(0, 1 << 32)), ts_step=3003)
            stream, index, nal_au, n_aus, pts = R.random_case(rng, int(rng.integers(0, 200)), max_nal=int(rng.choice([40, 900, 5000])),
                                                              aus=it % 3 != 2, times=it % 2 == 0)
            got = R.pack(stream, index, nal_au, n_aus, pts, prm)
            out["rtp %d %d" % (seed, it)] = digest(stream, *got)
            if len(index) > 3:
                index["end"][2] = index["start"][2] + 1
                out["rtp %d %d bad" % (seed, it)] = digest(*R.pack(stream, index, nal_au, n_aus, pts, prm))
    for seed in (188, 192, 204, 77, 31):
        rng = np.random.default_rng(seed)
        for it in range(6):
            prm = T.params(packet_bytes=seed if seed in T.SIZES else int(rng.choice(T.SIZES)), flags=int(rng.integers(0, 8)), cc_es=int(rng.integers(0, 16)),
                           cc_pat=int(rng.integers(0, 16)), cc_pmt=int(rng.integers(0, 16)), pcr_lead=int(rng.integers(0, 5000)))
            stream, au, pts, dts = T.random_case(rng, int(rng.integers(0, 80)), prm, max_es=int(rng.choice([30, 900, 9000])))
            got = T.mux(stream, au, pts if it % 4 != 3 else None, dts if it % 4 < 2 else None, prm)
            out["ts %d %d" % (seed, it)] = digest(stream, *got)
            out["ts %d %d cap" % (seed, it)] = digest(*T.mux(stream, au, pts, None, prm, out_cap=1000))
    for seed in (3, 5, 6, 8, 9, 10, 12):
        rng = np.random.default_rng(seed)
        for it in range(8):
            n_aus = int(rng.choice([1, 2, 5, 17, 40]))
            c = I.random_case(rng, n_aus, irap_every=int(rng.choice([0, 1, 3, 6])), sets_at_start=bool(rng.random() < 0.8),
                              last_without_picture=bool(rng.random() < 0.3), lead_junk=int(rng.integers(1, 9)) if it % 5 == 1 else 0)
            first = int(rng.integers(0, n_aus)) if it % 3 == 0 else 0
            count = int(rng.integers(1, n_aus + 2)) if it % 3 == 0 else n_aus
            got = I.au_insert(c[0], c[1], c[2], c[4], c[5], first, count, int(rng.integers(0, 8)))
            out["auins %d %d" % (seed, it)] = digest(*c, *got)
            out["auins %d %d cap" % (seed, it)] = digest(*I.au_insert(c[0], c[1], c[2], c[4], c[5], first, count, 3, out_cap=10, index_cap=2))
    return out


def test_the_split_references_give_what_they_gave():
    """tests/golden/big_ref_digests.json holds reference_digests() of the three references as they were before pack(), mux() and
    au_insert() became plan plus materialise and build() became the bytes plus tables()"""
    with open(GOLDEN) as f:
        recorded = json.load(f)
    now = reference_digests(R, T, I)
    assert sorted(now) == sorted(recorded)
    differ = [k for k in now if now[k] != recorded[k]]
    assert not differ, differ
