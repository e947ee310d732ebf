"""Streams of more than 2^32 bytes for the transport and AU-insert calls, without a host copy of them: layouts (lists of the nal()
dicts of tests/_auins_ref.py with explicit sizes, and the host tables that follow from the sizes alone), the stream of a layout
as a torch tensor on either device, the expectations of hbs_rtp_unpack and hbs_ts_demux derived from a layout, and checkers that
hold a call's whole output against a plan (the segments of tests/_segments.py).  A checker counts the bytes it compared and
demands that they are all of the output.  `scale` divides the large sizes and the 2^32 boundary, so that the same layouts and
checkers run on the CPU at scale 65536 (tests/test_big_checks.py).  No fixtures; no loop per byte or per packet."""
import numpy as np

from tests import _auins_ref as I
from tests import _rtp_ref as R
from tests import _segments as S
from tests import _ts_ref as D
from tests import _tsmux_ref as T

FIELDS = ("nal_count", "nal_found", "rbsp_bytes", "stream_bytes", "stop_reason", "error")


# ---- layouts ------------------------------------------------------------------------------------------------------------------

class Layout:
    """nals (nal() dicts with sizes), boundary (2^32 / scale), and the tables: total, index, parsed, compact, au, nal_au"""

    def __init__(self, nals, boundary, scale, tables=None):
        self.nals, self.boundary, self.scale = nals, boundary, scale
        self.total, self.index, self.parsed, self.compact, self.au, self.nal_au = tables if tables is not None else I.tables(nals)
        self.hdr = np.array([I.header_bytes(d) for d in nals], dtype=np.uint8).reshape(len(nals), 2)
        self.gap = np.array([I.gap_bytes(d, k) for k, d in enumerate(nals)], dtype=np.int64)

    @property
    def n_aus(self):
        return len(self.au)


def _gaps(rng):
    return dict(sc=int(rng.choice([3, 4])), zeros=int(rng.integers(0, 4)) if rng.random() < 0.3 else 0)


def small_aus(rng, count, lo, hi, first_au, irap_every, sets_in_first=False, p_aud=0.3, max_slices=3):
    """the NALs of `count` access units of random_aus' kinds (existing AUDs on some, prefix SEI on some, IRAP pictures, 3- and
    4-byte start codes, zeros between units), every NAL of lo .. hi bytes but the 3-byte AUDs; no junk, one layer, rc >= 0"""
    out = []
    for a in range(first_au, first_au + count):
        irap = a % irap_every == 0
        if rng.random() < p_aud:
            out.append(I.nal(35, size=3, **_gaps(rng)))
        if sets_in_first and a == first_au:
            out += [I.nal(t, size=int(rng.integers(4, 60)), rc=1, **_gaps(rng)) for t in (32, 33, 34)]
        if rng.random() < 0.3:
            out.append(I.nal(39, size=int(rng.integers(max(lo, 3), hi + 1)), **_gaps(rng)))
        tid1 = 1 if irap else int(rng.integers(1, 4))
        for sl in range(int(rng.integers(1, max_slices + 1))):
            out.append(I.nal(19 if irap else (1 if tid1 == 1 else 0), tid1=tid1, first=1 if sl == 0 else 0, stype=2 if irap else int(rng.integers(0, 3)),
                             lsb=(a * 2) % 256, size=int(rng.integers(lo, hi + 1)), **_gaps(rng)))
    return out


def _bytes_of(nals, first):
    return sum(I.gap_bytes(d, first + k) + d["size"] for k, d in enumerate(nals))


def layout_a(scale=1, seed=1):
    """Access units around the boundary B = 2^32 / scale: 40 small AUs (AU 0 with VPS, SPS, PPS), one AU of four slices of about
    B / 4 bytes that ends 64 .. 128 KiB (at scale 1) below B, 60 AUs of one small slice among which B falls (every seventh an
    IRAP picture, the sets in force for them in AU 0), one AU of one slice of about 600 MiB / scale, 40 small AUs above B."""
    rng = np.random.default_rng(seed)
    B = (1 << 32) // scale
    hi = max(24, min(20000, B // 160))
    tiny = max(40, 3072 // min(scale, 64))
    part1 = small_aus(rng, 40, 3, hi, 0, 6, sets_in_first=True)
    mid = small_aus(rng, 60, tiny - 8, tiny + 8, 41, 7, p_aud=0.2, max_slices=1)
    margin = int(_bytes_of(mid, 1) * rng.uniform(0.4, 0.65))
    big = [I.nal(1, first=1 if sl == 0 else 0, stype=1, lsb=80, sc=4 if sl == 0 else 3) for sl in range(4)]
    room = B - margin - _bytes_of(part1, 0) - _bytes_of([dict(d, size=0) for d in big], 1)
    cut = np.sort(rng.integers(room // 4 - room // 64, room // 4 + room // 64, size=3) * np.arange(1, 4))
    for d, size in zip(big, np.diff(np.concatenate([[0], cut, [room]]))):
        d["size"] = int(size)
    large = [I.nal(1, first=1, stype=0, lsb=90, size=600 * (1 << 20) // scale + int(rng.integers(0, 977)), sc=3)]
    tail = small_aus(rng, 40, 3, hi, 102, 5)
    L = Layout(part1 + big + mid + large + tail, B, scale)
    L.big = list(range(len(part1), len(part1) + 4))           # the four large slices
    L.large = len(part1) + 4 + len(mid)                       # the slice behind the boundary
    L.margin = margin
    a_big = int(L.nal_au[L.big[0]])
    # what the layout promises
    assert L.n_aus == 40 + 1 + 60 + 1 + 40 and a_big == 40 and (L.nal_au[L.big] == a_big).all(), (L.n_aus, a_big)
    assert int(L.au["unit_end"][a_big]) == B - margin and int(L.au["nal_count"][a_big]) == 4
    if scale == 1:
        assert 64 << 10 <= margin <= 128 << 10
    a_cross = int(np.searchsorted(L.au["unit_end"], B, side="right"))
    assert 41 < a_cross < 100 and int(L.au["unit_begin"][a_cross]) < B, a_cross          # B falls among the 60 small AUs
    L.cross = a_cross
    irap = (L.au["flags"] & I.A.IRAP) != 0
    assert irap[a_cross + 1:101].sum() >= 2 and irap[102:].sum() >= 3                    # IRAP AUs behind B whose sets lie in front of the big AU
    assert int(L.nal_au[L.large]) == 101 and int(L.au["unit_begin"][101]) > B and int(L.au["nal_count"][101]) == 1
    sizes = (L.index["end"] - L.index["start"]).astype(np.int64)
    assert sizes.max() < (1 << 31) // scale + 1 and L.total > B + 600 * (1 << 20) // scale
    assert not ((L.parsed["nal_unit_type"][L.large:] >= 32) & (L.parsed["nal_unit_type"][L.large:] <= 34)).any()
    return L


def layout_b(scale=1, seed=2):
    """one NAL of 2^32 / scale + 40 MiB / scale bytes between a few small ones: for the RTP calls alone (rbsp_len cannot say its
    size), so the index is made by hand and has start and end only"""
    rng = np.random.default_rng(seed)
    B = (1 << 32) // scale
    nals = [I.nal(t, size=int(rng.integers(3, 90)), **_gaps(rng)) for t in (32, 33, 34, 39)]
    nals.append(I.nal(19, first=1, stype=2, size=B + 40 * (1 << 20) // scale + int(rng.integers(0, 500)), sc=4))
    nals += [I.nal(1, first=1, size=int(rng.integers(3, 2000)), **_gaps(rng)) for _ in range(5)]
    n = len(nals)
    index = np.zeros(n, dtype=I.NAL_ENTRY)
    at = 0
    for k, d in enumerate(nals):
        at += I.gap_bytes(d, k)
        index["start"][k], index["end"][k] = at, at + d["size"]
        at += d["size"]
    nal_au = np.array([0] * 5 + list(range(1, 6)), dtype=np.uint32)
    L = Layout(nals, B, scale, tables=(at, index, None, None, np.zeros(6, dtype=I.ACCESS_UNIT), nal_au))
    L.giant = 4
    assert int(index["end"][4] - index["start"][4]) > B and int(index["start"][4]) < B // 2
    return L


def giant_output(L, max_payload, framing):
    """the bytes hbs_rtp_pack writes for layout B's giant NAL"""
    size = int(L.index["end"][L.giant] - L.index["start"][L.giant])
    count = R.nal_packets(size, max_payload)
    return count * (framing + 15) + size - 2


# ---- streams --------------------------------------------------------------------------------------------------------------------

def make_stream(L, device, seed=5):
    """the layout's bytes as a torch uint8 tensor on `device`: random bytes of 1 .. 255, then the zeros and the 01 of every start
    code and the two header bytes of every NAL scattered in by index"""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    d = torch.randint(1, 256, (L.total,), dtype=torch.uint8, device=device, generator=g)
    start = L.index["start"].astype(np.int64)
    before = np.concatenate([[0], np.cumsum(L.gap)[:-1]])
    zeros = np.repeat(start - L.gap - before, L.gap) + np.arange(int(L.gap.sum()))          # every byte of every gap
    d[torch.from_numpy(zeros).to(device)] = 0
    d[torch.from_numpy(start - 1).to(device)] = 1
    d[torch.from_numpy(start).to(device)] = torch.from_numpy(L.hdr[:, 0].copy()).to(device)
    d[torch.from_numpy(start + 1).to(device)] = torch.from_numpy(L.hdr[:, 1].copy()).to(device)
    return d


def times(L):
    """pts and dts per AU for hbs_ts_mux: a third of the AUs without a time, a third with a PTS only, a third with both"""
    m = L.n_aus
    form = np.arange(m) % 3
    form[40] = 2                                                    # the big AU has both, and so a PCR where PCRs are asked for
    pts = np.where(form == 0, T.NO_TIME, (900000 + 3003 * np.arange(m) + 6006).astype(np.uint64) % np.uint64(1 << 33)).astype(np.uint64)
    dts = np.where(form == 2, (900000 + 3003 * np.arange(m)).astype(np.uint64), np.uint64(T.NO_TIME)).astype(np.uint64)
    return pts, dts


def rtp_times(L):
    """one pts per AU for hbs_rtp_pack"""
    return (np.arange(L.n_aus, dtype=np.uint64) * np.uint64(3003) + np.uint64(1000)).astype(np.uint64)


# ---- expectations that follow from a layout ----------------------------------------------------------------------------------------

def packet_table(nal_off, nal_packet, prm):
    """pkt_off and pkt_size of every packet hbs_rtp_pack wrote, by np.repeat arithmetic (no length field inside)"""
    off = R.packet_offsets(nal_off, nal_packet, prm)
    fr = np.uint64(prm["framing"])
    return (off[:-1] + fr).astype(np.uint64), (np.diff(off) - fr).astype(np.uint64)


def unpack_plan(L, n_packets, ts_base, pts, sc=4):
    """what hbs_rtp_unpack makes of hbs_rtp_pack's packets of a layout: the NALs behind start codes
    -> (segments, index, nal_au, au_ts, summary)"""
    n = len(L.index)
    start, size = L.index["start"].astype(np.int64), (L.index["end"] - L.index["start"]).astype(np.int64)
    at = np.concatenate([[0], np.cumsum(size + sc)])
    segs = []
    for k in range(n):
        segs += [("lit", int(at[k]), bytes(sc - 1) + b"\x01"), ("copy", int(at[k]) + sc, int(start[k]), int(size[k]))]
    index = np.zeros(n, dtype=I.NAL_ENTRY)
    index["start"], index["end"] = at[:-1] + sc, at[1:]
    index["status"][-1] = I.ST_UNTERMINATED
    nal_au = (L.nal_au - L.nal_au[0]).astype(np.uint32)
    m = int(nal_au[-1]) + 1
    au_ts = ((np.uint64(ts_base) + pts[:m]) & np.uint64(R.M32)).astype(np.uint64)
    s = dict(nal_count=n, nal_found=n_packets, rbsp_bytes=int(size.sum()), stream_bytes=int(at[-1]), stop_reason=-1, error=0, reserved=[0, m, 0])
    return segs, index, nal_au, au_ts, s


def demux_plan(L, pts, dts, au_packet, es_packets):
    """what hbs_ts_demux makes of hbs_ts_mux's packets of a layout: the AUs back to back, one PES each
    -> (segments, pes, summary)"""
    m = L.n_aus
    b, size = L.au["unit_begin"].astype(np.int64), (L.au["unit_end"] - L.au["unit_begin"]).astype(np.int64)
    at = np.concatenate([[0], np.cumsum(size)])
    segs = [("copy", int(at[a]), int(b[a]), int(size[a])) for a in range(m) if size[a]]
    pes = np.zeros(m, dtype=D.TS_PES)
    has_pts = pts != np.uint64(T.NO_TIME)
    has_dts = has_pts & (dts != np.uint64(T.NO_TIME)) & (dts != pts)
    pes["out_off"], pes["packet"] = at[:-1], au_packet[:-1]
    pes["pts"] = np.where(has_pts, pts, np.uint64(D.NO_TIME))
    pes["dts"] = np.where(has_dts, dts, pes["pts"])
    irap = (L.au["flags"] & T.AU_IRAP) != 0
    pes["flags"] = D.F_ALIGN | np.where(has_pts, D.F_PTS, 0) | np.where(has_dts, D.F_DTS, 0) | np.where(irap, D.F_RAI, 0)
    s = dict(nal_count=m, nal_found=es_packets, rbsp_bytes=0, stream_bytes=int(at[-1]), stop_reason=0, error=0, reserved=[0, 0, 0])
    return segs, pes, s


# ---- checkers ---------------------------------------------------------------------------------------------------------------------

def _t(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def check_segments(out, src, segs, total, chunk=1 << 28):
    """every byte of `out` (a torch uint8 tensor of exactly `total` bytes) against the segments over `src` (a tensor on the same
    device) -> the bytes compared, which are all of them.  Verbatim ranges and the payload columns of strided runs are compared
    on the device, the header columns of a run against its vectorised headers, literals on the host after one indexed fetch."""
    import torch
    assert out.numel() == total, (out.numel(), total)
    assert S.tiles(segs, total), "the plan's segments do not tile the output"
    done = 0
    lits = [(seg[1], seg[2]) for seg in segs if seg[0] == "lit"]
    if lits:
        sizes = np.array([len(b) for _, b in lits], dtype=np.int64)
        before = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        where = np.repeat(np.array([o for o, _ in lits], dtype=np.int64) - before, sizes) + np.arange(int(sizes.sum()))
        got = out[_t(where, out.device)].cpu().numpy()
        want = np.frombuffer(b"".join(b for _, b in lits), dtype=np.uint8)
        bad = np.flatnonzero(got != want)
        if len(bad):
            k = int(np.searchsorted(before, bad[0], side="right")) - 1
            raise AssertionError("literal at output byte %d differs: %s, wanted %s" % (lits[k][0], got[before[k]:before[k] + sizes[k]].tobytes().hex(),
                                                                                       lits[k][1].hex()))
        done += int(sizes.sum())
    for seg in segs:
        o = seg[1]
        if seg[0] == "copy":
            _, _, s, n = seg
            assert s >= 0 and s + n <= src.numel(), seg
            if not torch.equal(out[o:o + n], src[s:s + n]):
                at = int(torch.nonzero(out[o:o + n] != src[s:s + n])[0])
                raise AssertionError("output byte %d is not source byte %d (a verbatim range of %d bytes from output byte %d)" % (o + at, s + at, n, o))
            done += n
        elif seg[0] == "run":
            r = seg[2]
            n, P, H, F = r["n"], r["P"], r["H"], r["F"]
            assert r["src"] >= 0 and r["src"] + n * F <= src.numel(), (seg[1], n, F)
            step = max(1, chunk // P)
            tail = _t(np.frombuffer(r["tail"], dtype=np.uint8), out.device) if r["tail"] else None
            for lo in range(0, n, step):
                hi = min(n, lo + step)
                rows = out[o + lo * P:o + hi * P].view(hi - lo, P)
                heads = _t(r["heads"](lo, hi), out.device)
                if not torch.equal(rows[:, :H], heads):
                    at = int(torch.nonzero((rows[:, :H] != heads).any(dim=1))[0])
                    raise AssertionError("the header of packet %d of the run at output byte %d differs: %s, wanted %s" % (
                        lo + at, o, bytes(rows[at, :H].cpu().tolist()).hex(), bytes(heads[at].cpu().tolist()).hex()))
                pay = src[r["src"] + lo * F:r["src"] + hi * F].view(hi - lo, F)
                if not torch.equal(rows[:, H:H + F], pay):
                    at = int(torch.nonzero((rows[:, H:H + F] != pay).any(dim=1))[0])
                    raise AssertionError("the payload of packet %d of the run at output byte %d is not source bytes %d .." % (
                        lo + at, o, r["src"] + (lo + at) * F))
                if tail is not None:
                    assert bool((rows[:, H + F:] == tail).all()), "the bytes behind packets %d .. of the run at output byte %d" % (lo, o)
            done += n * P
    assert done == total, "compared %d bytes of %d" % (done, total)
    return done


def summary_equal(s, want):
    for k in FIELDS:
        assert int(s[k]) == want[k], (k, s, want)
    assert [int(x) for x in s["reserved"]] == want["reserved"], (s, want)


def table_equal(name, got, want):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        j = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s differs at entry %d: %s, wanted %s" % (name, j, got[j], want[j]))


def check_pack(out, nal_off, nal_packet, summary, src, want):
    """hbs_rtp_pack's outputs against R.plan()'s"""
    segs, w_off, w_pkt, w_s = want
    summary_equal(summary, w_s)
    table_equal("d_nal_off", nal_off, w_off)
    table_equal("d_nal_packet", nal_packet, w_pkt)
    return check_segments(out, src, segs, w_s["stream_bytes"])


def check_unpack(out, index, nal_au, au_ts, summary, src, want):
    """hbs_rtp_unpack's outputs against unpack_plan()'s"""
    segs, w_index, w_au, w_ts, w_s = want
    summary_equal(summary, w_s)
    table_equal("d_index_out", index, w_index)
    table_equal("d_nal_au_out", nal_au, w_au)
    table_equal("d_au_ts_out", au_ts, w_ts)
    return check_segments(out, src, segs, w_s["stream_bytes"])


def check_mux(out, au_packet, summary, src, want):
    """hbs_ts_mux's outputs against T.plan()'s"""
    segs, w_packet, w_s = want
    summary_equal(summary, w_s)
    table_equal("d_au_packet", au_packet, w_packet)
    return check_segments(out, src, segs, w_s["stream_bytes"])


def check_demux(out, pes, summary, src, want, packet=None):
    """hbs_ts_demux's outputs against demux_plan()'s; packet: the packet numbers to expect where foreign packets were put in"""
    segs, w_pes, w_s = want
    if packet is not None:
        w_pes = w_pes.copy()
        w_pes["packet"] = packet
    summary_equal(summary, w_s)
    table_equal("d_pes", pes, w_pes)
    return check_segments(out, src, segs, w_s["stream_bytes"])


def check_insert(out, index_out, nal_src, nal_au_out, au_out, summary, src, want):
    """hbs_au_insert's outputs against I.plan()'s"""
    segs, w_index, w_src, w_nau, w_au, w_s = want
    summary_equal(summary, w_s)
    table_equal("d_index_out", index_out, w_index)
    table_equal("d_nal_src", nal_src, w_src)
    table_equal("d_nal_au_out", nal_au_out, w_nau)
    table_equal("d_au_out", au_out, w_au)
    return check_segments(out, src, segs, w_s["stream_bytes"])


def with_foreign_packets(ts, every=9):
    """a 188-byte transport stream (torch tensor) with a packet of PID 0x1FFF in front of every `every`-th packet, by one indexed
    copy into a larger tensor, the index made on the tensor's device -> (the stream, old packet number -> new packet number)"""
    import torch
    n = ts.numel() // 188

    def moved(p):
        return p + p // every + 1
    total = n + -(-n // every)
    null = np.full(188, 0xFF, dtype=np.uint8)
    null[:4] = (0x47, 0x1F, 0xFF, 0x10)
    big = _t(null, ts.device).repeat(total)
    big.view(total, 188).index_copy_(0, moved(torch.arange(n, dtype=torch.int64, device=ts.device)), ts.view(n, 188))
    return big, moved
