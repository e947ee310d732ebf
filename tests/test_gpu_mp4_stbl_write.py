"""hbs_mp4_stbl_write on the GPU against tests/_mp4_stbl_write_ref.py, byte for byte: every case plans first, then runs into a
d_out of exactly T bytes with canaries behind it and behind d_tables; the plan's summary is the run's; output bytes, record and
every summary field are the reference's.  The round trips: tables -> boxes -> hbs_mp4_stbl_samples -> tables on the device, and
Annex-B -> a whole .mp4 -> Annex-B."""
import struct

import numpy as np
import pytest

from tests import _mp4_stbl_ref as S
from tests import _mp4_stbl_write_ref as Wr
from tests.test_mp4_read_ref import NALS

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 1024
W = Wr.W
CASES = Wr.valid_cases()
ERRORS = Wr.error_cases()
_want = {}


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


def want_of(c):
    """the reference's (blob, record, summary) of a case, computed once"""
    if c["name"] not in _want:
        _want[c["name"]] = Wr.call(c)
    return _want[c["name"]]


def dev(values, dtype=np.uint64):
    import torch
    a = np.array([int(v) & ((1 << 64) - 1) for v in values], dtype=dtype).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).cuda() if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")


def canary(n):
    import torch
    return torch.full((n + PAD,), CAN, dtype=torch.uint8, device="cuda")


def upload(c):
    t = c["t"]
    return dict(sample_off=dev(t["off"]), sample_size=dev(t["size"]), dts=None if t["dts"] is None else dev(t["dts"]),
                pts=None if t["pts"] is None else dev(t["pts"]), sample_flags=None if t["flags"] is None else dev(t["flags"], np.uint32))


def params_of(c):
    import hevcbitstream_amd as hbs
    p = c["params"]
    return hbs.mp4_stbl_write_params(flags=S.CO64 if p.get("co64") else 0, max_chunk_samples=p.get("max_chunk_samples", 0),
                                     sample_duration=p["sample_duration"], base_time=p.get("base_time", 0), data_offset=p.get("data_offset", 0))


def launch(ctx, c, d, out=None, out_cap=0, tables=None, fill=0x5A):
    import torch
    from hevcbitstream_amd.api import SUMMARY
    summary = torch.full((SUMMARY.itemsize,), fill, dtype=torch.uint8, device="cuda")
    rc = ctx.mp4_stbl_write_async(d["sample_off"], d["sample_size"], len(c["t"]["size"]), params_of(c), summary, dts=d["dts"], pts=d["pts"],
                                  sample_flags=d["sample_flags"], out=out, out_cap=out_cap, tables=tables)
    assert rc == 0, rc
    return ctx.read_summary(summary)


def summary_matches(s, want):
    got = dict(error=int(s["error"]), nal_count=int(s["nal_count"]), nal_found=int(s["nal_found"]), rbsp_bytes=int(s["rbsp_bytes"]),
               stream_bytes=int(s["stream_bytes"]), stop_reason=int(s["stop_reason"]), reserved=[int(x) for x in s["reserved"]])
    assert got == want


def untouched(*tensors):
    for t in tensors:
        assert (t.cpu().numpy() == CAN).all(), "stored where nothing may be"


def run(ctx, c):
    """plan, then a run into exactly T bytes; everything against the reference"""
    blob, rec, want = want_of(c)
    assert want["error"] == 0, want
    d = upload(c)
    T = len(blob)
    tab = canary(128)
    s = launch(ctx, c, d, tables=tab)
    summary_matches(s, want)
    got = tab.cpu().numpy()
    assert got[:128].tobytes() == rec.tobytes() and (got[128:] == CAN).all()
    out, tab = canary(T), canary(128)
    s2 = launch(ctx, c, d, out=out, out_cap=T, tables=tab)
    summary_matches(s2, want)
    assert s2.tobytes() == s.tobytes(), "the plan's summary is the run's"
    got = out.cpu().numpy()
    bad = np.flatnonzero(got[:T] != np.frombuffer(blob, dtype=np.uint8))
    assert not len(bad), "%s: byte %d of %d differs (%d do)" % (c["name"], bad[0], T, len(bad))
    assert (got[T:] == CAN).all(), "stored behind d_out"
    got = tab.cpu().numpy()
    assert got[:128].tobytes() == rec.tobytes() and (got[128:] == CAN).all()
    return out, rec


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_boxes_record_and_summary(ctx, i):
    run(ctx, CASES[i])


@pytest.mark.parametrize("i", range(len(ERRORS)), ids=["%s at %d" % (c["name"], p) for c, p in ERRORS])
def test_every_sample_error_at_its_lowest_sample_and_nothing_written(ctx, i):
    c, p = ERRORS[i]
    want = want_of(dict(c, name="%s at %d" % (c["name"], p)))[2]
    assert want == Wr.summary(Wr.E_ARG, len(c["t"]["size"]), bad_sample=p + 1)
    d = upload(c)
    tab = canary(128)
    summary_matches(launch(ctx, c, d, tables=tab), want)
    out = canary(1 << 16)
    summary_matches(launch(ctx, c, d, out=out, out_cap=1 << 16, tables=tab), want)
    untouched(out, tab)


def test_the_same_offsets_without_co64_are_an_error_at_the_chunk_s_first_sample(ctx):
    c = next(x for x in CASES if x["name"] == "co64 above 4 GiB")
    c = dict(c, name="no co64", params=dict(c["params"], co64=False))
    want = want_of(c)[2]
    assert want == Wr.summary(Wr.E_ARG, len(c["t"]["size"]), bad_sample=1)
    out, tab = canary(4096), canary(128)
    summary_matches(launch(ctx, c, upload(c), out=out, out_cap=4096, tables=tab), want)
    untouched(out, tab)
    # a chunk that begins below 4 GiB may run past it; the next chunk may not begin there
    c = next(x for x in CASES if x["name"] == "a chunk that crosses 4 GiB")
    c = dict(c, name="cut behind 4 GiB", params=dict(c["params"], max_chunk_samples=W))
    want = want_of(c)[2]
    assert want == Wr.summary(Wr.E_ARG, len(c["t"]["size"]), bad_sample=W + 1)
    summary_matches(launch(ctx, c, upload(c), out=out, out_cap=4096, tables=tab), want)
    untouched(out, tab)


def test_capacity(ctx):
    c = CASES[5]
    blob, rec, want = want_of(c)
    T = len(blob)
    d = upload(c)
    for cap in (0, T - 4):
        out, tab = canary(T), canary(128)
        summary_matches(launch(ctx, c, d, out=out, out_cap=cap, tables=tab), dict(want, error=Wr.E_CAPACITY))
        untouched(out, tab)
    out = canary(T + 64)
    summary_matches(launch(ctx, c, d, out=out, out_cap=T + 64), want)          # more room than bytes, no d_tables
    got = out.cpu().numpy()
    assert got[:T].tobytes() == blob and (got[T:] == CAN).all()


def test_argument_refusals(ctx):
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import SUMMARY
    c = CASES[2]
    d = upload(c)
    n = len(c["t"]["size"])
    summary = torch.full((SUMMARY.itemsize + 16,), 0x11, dtype=torch.uint8, device="cuda")
    out, tab = canary(1 << 14), canary(128 + 16)
    E = S.E_ARG

    def rc(prm=None, n=n, summ=summary[:SUMMARY.itemsize], **kw):
        a = dict(d, out=out, out_cap=1 << 14, tables=tab[:128])
        a.update(kw)
        return ctx.mp4_stbl_write_async(a.pop("sample_off"), a.pop("sample_size"), n, params_of(c) if prm is None else prm, summ, **a)
    assert rc() == 0 and rc(out=None, out_cap=0, tables=None) == 0
    for field, value in (("flags", 2), ("flags", 1 << 31), ("reserved0", 1), ("base_time", 1 << 62), ("data_offset", 1 << 62)):
        p = params_of(c)
        p[field] = value
        assert rc(prm=p) == E, field
    p = params_of(c)
    p["base_time"], p["data_offset"] = (1 << 62) - 1, 0
    assert rc(prm=p) == 0
    assert rc(n=1 << 32) == E
    assert rc(out_cap=(1 << 46) + 1) == E and rc(out=None, out_cap=(1 << 46) + 1) == 0
    assert rc(sample_off=None) == E and rc(sample_size=None) == E and rc(summ=None) == E
    assert ctx.mp4_stbl_write_async(d["sample_off"], d["sample_size"], n, None, summary[:SUMMARY.itemsize]) == E
    assert ctx.mp4_stbl_write_async(None, None, 0, params_of(c), summary[:SUMMARY.itemsize]) == 0          # no samples: no tables needed
    for name, step in (("sample_off", 4), ("sample_size", 4), ("dts", 4), ("pts", 4), ("sample_flags", 2)):
        if d[name] is not None:
            assert rc(**{name: d[name][step:]}) == E, name
    assert rc(out=out[8:]) == E and rc(tables=tab[8:136]) == E and rc(summ=summary[8:8 + SUMMARY.itemsize]) == E
    for name in ("dts", "pts", "sample_flags", "tables"):
        assert rc(**{name: None}) == 0, name                                                                # each is optional
    torch.cuda.synchronize()
    assert hbs.mp4_stbl_write_bytes(n) >= int(want_of(c)[2]["stream_bytes"])


# ---- round trips ---------------------------------------------------------------------------------------------------------------

def test_round_trip_on_the_device_tables_boxes_tables(ctx):
    c = next(x for x in CASES if x["name"] == "random %d" % (2 * W + 1))
    t, p = c["t"], c["params"]
    d = upload(c)
    n = len(t["size"])
    out, rec, s = ctx.mp4_stbl_write(d["sample_off"], d["sample_size"], n, params_of(c), dts=d["dts"], pts=d["pts"], sample_flags=d["sample_flags"])
    blob, want_rec, want = want_of(c)
    assert out.cpu().numpy().tobytes() == blob and rec.tobytes() == want_rec.tobytes()
    summary_matches(s, want)
    rec["file_bytes"] = 1 << 40
    off, size, dts, pts, flags, s2 = ctx.mp4_stbl_samples(out, rec)
    assert off.tolist() == t["off"] and size.tolist() == t["size"] and int(s2["nal_found"]) == want["nal_found"]
    assert dts.tolist() == [x - t["dts"][0] for x in t["dts"]] and pts.tolist() == [x - t["dts"][0] for x in t["pts"]]
    assert (flags != 0).tolist() == [bool(f & S.NON_SYNC) for f in t["flags"]]


@pytest.mark.parametrize("moov_first", (True, False))
def test_round_trip_annexb_mp4_file_annexb(ctx, moov_first):
    import torch
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(31)
    n_aus = 2 * W + 37
    counts = rng.integers(1, 4, size=n_aus)
    n = int(counts.sum())
    lens = rng.integers(2, 300, size=n)
    stream = bytearray()
    for k in range(n):
        stream += b"\x00\x00\x00\x01" + bytes(rng.integers(4, 256, size=int(lens[k]), dtype=np.uint8))
    stream = np.frombuffer(bytes(stream), dtype=np.uint8)
    d_stream = torch.from_numpy(stream.copy()).cuda()
    idx, _, s = ctx.index_extract(d_stream, index_cap=n + 16, want_rbsp=False)
    assert len(idx) == n
    nal_au = np.repeat(np.arange(n_aus, dtype=np.uint32), counts)
    lp, _, so, s = ctx.annexb_to_lenpref(d_stream, idx, nal_au=nal_au, n_aus=n_aus, length_size=4)
    body = lp.cpu().numpy().tobytes()
    so = np.asarray(so, dtype=np.uint64)
    sizes = (so[1:] - so[:-1]).tolist()
    track = S.random_track(rng, n_aus)
    dts = np.concatenate([[0], np.cumsum(track["deltas"][:-1])]).astype(np.int64) + 1000
    pts = dts + np.array(track["cts"], dtype=np.int64)
    flags = np.full(n_aus, 0x01010000, dtype=np.uint32)
    flags[track["sync"]] = 0x02000000
    d = dict(sample_off=dev(so[:n_aus]), sample_size=dev(sizes), dts=dev(dts), pts=dev(pts), sample_flags=dev(flags, np.uint32))
    prm = hbs.mp4_stbl_write_params(sample_duration=track["deltas"][-1], max_chunk_samples=50)
    _, _, plan = ctx.mp4_stbl_write(d["sample_off"], d["sample_size"], n_aus, prm, dts=d["dts"], pts=d["pts"], sample_flags=d["sample_flags"])
    T, D = int(plan["stream_bytes"]), int(plan["reserved"][1])
    assert D == sum(track["deltas"]) and int(plan["nal_found"]) == -(-n_aus // 50)
    prefix = hbs.mp4_moov(NALS, D, T, track_id=4)
    assert prefix == Wr.moov_prefix(NALS, D, T, track_id=4)
    prm["data_offset"] = len(prefix) + T + 8 if moov_first else int.from_bytes(prefix[:4], "big") + 8
    boxes, rec, s = ctx.mp4_stbl_write(d["sample_off"], d["sample_size"], n_aus, prm, dts=d["dts"], pts=d["pts"], sample_flags=d["sample_flags"])
    assert int(s["stream_bytes"]) == T
    data = Wr.assemble(prefix, boxes.cpu().numpy().tobytes(), body, moov_first)
    assert data[int(prm["data_offset"][0]) - 8:][:8] == struct.pack(">I", 8 + len(body)) + b"mdat"
    # the file read back by what reads files
    found = hbs.mp4_stbl_find(data, track_id=4)
    assert found.tobytes() == S.find(data).tobytes()
    base = len(prefix) if moov_first else len(data) - T
    for name in S.BOXES:
        assert found[name][0].tolist() == [int(rec[name][0][0]) + base, int(rec[name][0][1])], name
    trk, sets = hbs.mp4_track_read(data)
    assert int(trk["length_size"]) == 4 and int(trk["track_id"]) == 4 and sets == [bytes(x) for x in NALS]
    d_file = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    off, size, dts2, pts2, fl2, s = ctx.mp4_stbl_samples(d_file, found)
    want = S.read(data, found)
    for got, w in zip((off, size, dts2, pts2, fl2), want[:5]):
        assert np.array_equal(got, w)
    assert size.tolist() == sizes and np.array_equal(dts2.astype(np.int64), dts - 1000) and np.array_equal(pts2.astype(np.int64), pts - 1000)
    assert np.flatnonzero(fl2 == 0).tolist() == track["sync"]
    back, _, _ = ctx.lenpref_to_annexb(d_file, off, size, length_size=4, startcode_bytes=4)
    assert np.array_equal(back.cpu().numpy(), stream)


# ---- a HIP graph ---------------------------------------------------------------------------------------------------------------

def test_one_replay_from_a_graph_on_other_contents(ctx):
    """captured on a side stream after one warm-up call, replayed on other contents of the same buffers: other sizes, chunks,
    times and sync samples; every host argument is the same"""
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import SUMMARY
    n = 2 * W + 50
    members = []
    for seed in (90, 91):
        rng = np.random.default_rng(seed)
        sizes = [int(x) for x in rng.integers(0, 60, size=n)]
        lens = [seed - 60, n - 2 * (seed - 60), seed - 60]
        t = Wr.tables_of(sizes, lens, [int(x) for x in rng.integers(0, 3, size=n)], [int(x) for x in rng.integers(-2, 3, size=n)],
                         list(range(seed % 3, n, 3)), dts0=10)
        members.append(Wr.case("graph %d" % seed, t, sample_duration=7, max_chunk_samples=40, data_offset=48, co64=True))
    wants = [want_of(c) for c in members]
    assert len(wants[0][0]) != len(wants[1][0])
    cap = hbs.mp4_stbl_write_bytes(n, True, True, S.CO64)
    d = upload(members[0])
    out, tab = canary(cap), canary(128)
    summary = torch.full((SUMMARY.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")

    def go():
        return ctx.mp4_stbl_write_async(d["sample_off"], d["sample_size"], n, params_of(members[0]), summary, dts=d["dts"], pts=d["pts"],
                                        sample_flags=d["sample_flags"], out=out, out_cap=cap, tables=tab)

    def check(want):
        blob, rec, s = want
        summary_matches(ctx.read_summary(summary), s)
        got = out.cpu().numpy()
        assert got[:len(blob)].tobytes() == blob and (got[len(blob):] == CAN).all()
        assert tab.cpu().numpy()[:128].tobytes() == rec.tobytes()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert go() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            go()
    check(wants[0])
    held = ctx.device_bytes()
    for which in (1, 0):
        fresh = upload(members[which])
        for name in d:
            d[name].copy_(fresh[name])
        out.fill_(CAN)
        tab.fill_(CAN)
        summary.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        check(wants[which])
    assert ctx.device_bytes() == held
