"""hbs_annexb_to_lenpref / hbs_lenpref_to_annexb on the device against the plain-loop reference (tests/_lenpref_ref.py): output
bytes, output index, sample tables and every summary field; outputs of exactly the planned capacity with canaries behind them."""
import numpy as np
import pytest

from tests import _filter_ref as F
from tests import _lenpref_ref as R

pytestmark = pytest.mark.gpu
CAN = 0xC3
PAD = 4096
TILE = 65536


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def canary(n):
    import torch
    return torch.full((n + PAD,), CAN, dtype=torch.uint8, device="cuda")


def summary_matches(sm, want):
    for k, v in want.items():
        if k == "reserved0":
            assert int(sm["reserved"][0]) == v, (k, int(sm["reserved"][0]), v)
        else:
            assert int(sm[k]) == v, (k, int(sm[k]), v)
    assert list(sm["reserved"][1:]) == [0, 0] and ("reserved0" in want or int(sm["reserved"][0]) == 0)


def random_aus(rng, n):
    """a valid AU numbering of n NALs"""
    if n == 0:
        return np.zeros(0, np.uint32), 0
    au = np.cumsum(np.concatenate([[0], rng.random(n - 1) < rng.random()])).astype(np.uint32)
    return au, int(au[-1]) + 1


def forward(ctx, s, idx, keep=None, L=4, nal_au=None, n_aus=0, out_cap=None, want_error=0):
    """plan, then run into an output of exactly out_cap bytes (default: the planned size); everything against the reference.
    Returns the output bytes."""
    import torch
    n = len(idx)
    want_out, want_io, want_so, want_s = R.to_lenpref_ref(s, idx, keep, L, nal_au, n_aus, out_cap)
    assert want_s["error"] == want_error
    if want_error == R.E_ARG:          # the header leaves the sizes open for HBS_E_ARG
        want_s = {k: v for k, v in want_s.items() if k not in ("nal_count", "rbsp_bytes", "stream_bytes")}
    d_s, d_i = dev(s), dev(idx)
    d_k = dev(np.asarray(keep, dtype=np.uint8)) if keep is not None else None
    d_a = dev(np.asarray(nal_au, dtype=np.uint32)) if nal_au is not None else None
    summ = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    kw = dict(keep=d_k, length_size=L, nal_au=d_a, n_aus=n_aus)
    assert ctx.annexb_to_lenpref_async(d_s, len(s), d_i, n, None, None, summ, **kw) == 0
    plan = ctx.read_summary(summ)
    if want_error != R.E_CAPACITY:
        summary_matches(plan, want_s)
    cap = int(plan["stream_bytes"]) if out_cap is None else out_cap
    out, io, so = canary(cap), canary(n * 32), canary((n_aus + 1) * 8)
    summ.fill_(0xEE)
    assert ctx.annexb_to_lenpref_async(d_s, len(s), d_i, n, out, io, summ, sample_off=so if nal_au is not None else None, out_cap=cap, **kw) == 0
    sm = ctx.read_summary(summ)
    summary_matches(sm, want_s)
    o, i, t = out.cpu().numpy(), io.cpu().numpy(), so.cpu().numpy()
    if want_error:
        assert (o == CAN).all() and (i == CAN).all() and (t == CAN).all()          # nothing written
        return None
    assert np.array_equal(o[:cap], want_out) and (o[cap:] == CAN).all()
    k = len(want_io) * 32
    assert np.array_equal(i[:k].view(F.NAL_ENTRY), want_io) and (i[k:] == CAN).all()
    if nal_au is not None:
        assert np.array_equal(t[:(n_aus + 1) * 8].view(np.uint64), want_so) and (t[(n_aus + 1) * 8:] == CAN).all()
    else:
        assert (t == CAN).all()
    return o[:cap]


def reverse(ctx, data, off, size, L=4, sc=4, nal_cap=None, out_cap=None, want_error=0):
    import torch
    n = len(off)
    want_out, want_so, want_s = R.to_annexb_ref(data, off, size, L, sc, nal_cap, out_cap)
    assert want_s["error"] == want_error
    d_d, d_o, d_z = dev(data), dev(np.asarray(off, dtype=np.uint64)), dev(np.asarray(size, dtype=np.uint64))
    summ = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    kw = dict(length_size=L, startcode_bytes=sc)
    assert ctx.lenpref_to_annexb_async(d_d, len(data), d_o, d_z, n, None, None, summ, nal_cap=(1 << 64) - 1, **kw) == 0
    plan = ctx.read_summary(summ)
    if want_error != R.E_CAPACITY:
        summary_matches(plan, want_s)
    cap = int(plan["stream_bytes"]) if out_cap is None else out_cap
    ncap = int(plan["nal_count"]) if nal_cap is None else nal_cap
    out, so = canary(cap), canary((n + 1) * 8)
    summ.fill_(0xEE)
    assert ctx.lenpref_to_annexb_async(d_d, len(data), d_o, d_z, n, out, so, summ, nal_cap=ncap, out_cap=cap, **kw) == 0
    sm = ctx.read_summary(summ)
    summary_matches(sm, want_s)
    o, t = out.cpu().numpy(), so.cpu().numpy()
    if want_error:
        assert (o == CAN).all() and (t == CAN).all()
        return None
    assert np.array_equal(o[:cap], want_out) and (o[cap:] == CAN).all()
    assert np.array_equal(t[:(n + 1) * 8].view(np.uint64), want_so) and (t[(n + 1) * 8:] == CAN).all()
    return o[:cap]


def both_ways(ctx, s, idx, keep, L, sc, rng):
    """forward with a random AU numbering, then its samples back"""
    au, n_aus = random_aus(rng, len(idx))
    out = forward(ctx, s, idx, keep, L, au, n_aus)
    so = R.to_lenpref_ref(s, idx, keep, L, au, n_aus)[2].astype(np.int64)
    back = reverse(ctx, out, so[:-1], np.diff(so), L, sc)
    pay = [s[int(e["start"]):int(e["end"])] for e in idx[np.asarray(keep, bool)]] if keep is not None else [s[int(e["start"]):int(e["end"])] for e in idx]
    want = np.concatenate([np.concatenate([np.frombuffer(R.SC[sc], np.uint8), p]) for p in pay]) if pay else np.zeros(0, np.uint8)
    assert np.array_equal(back, want)


def made_stream(rng, lens, junk=0):
    """`junk` non-zero bytes, then for each length a 3- or 4-byte start code and that many non-zero payload bytes; its index"""
    lens = np.asarray(lens, dtype=np.int64)
    sc = np.where(rng.random(len(lens)) < 0.3, 4, 3)
    pos = junk + np.concatenate([[0], np.cumsum(lens + sc)[:-1]])
    s = rng.integers(1, 256, size=junk + int((lens + sc).sum()), dtype=np.uint8)
    s[pos] = 0
    s[pos + 1] = 0
    s[pos + 2] = np.where(sc == 4, 0, 1)
    s[pos[sc == 4] + 3] = 1
    idx = np.zeros(len(lens), dtype=F.NAL_ENTRY)
    idx["start"], idx["end"], idx["rbsp_len"] = pos + sc, pos + sc + lens, lens
    idx["status"] = rng.integers(0, 8, size=len(lens))
    return s, idx


def test_random_streams_masks_and_length_sizes(ctx, orc):
    rng = np.random.default_rng(2025)
    for it in range(40):
        size = int(rng.choice([1, 7, 100, 5000, 70000, 300000, 3 << 20]))
        mean = int(rng.choice([3, 20, 200, 3000, 100000]))
        if mean < 100:
            size = min(size, 200000)
        s = F.random_stream(rng, size, mean)
        idx, _, _ = orc.index_extract(s)
        keep = rng.random(len(idx)) < rng.random()
        longest = int((idx["end"] - idx["start"])[keep].max()) if keep.any() else 0
        L = int(rng.choice([x for x in (1, 2, 4) if longest < (1 << (8 * x))]))
        both_ways(ctx, s, idx, keep, L, int(rng.choice([3, 4])), rng)
        forward(ctx, s, idx, None, 4)                                        # keep-all without a mask, no sample table


@pytest.mark.parametrize("L", [1, 2, 4])
def test_tile_and_chunk_boundaries_inside_prefixes(ctx, L):
    """record offsets sweep 65536 - 8 .. 65536 + 8 (and the same around 16-byte chunk boundaries all along): every byte of a
    length field, and the first and last payload byte, falls on a tile boundary and on a chunk boundary"""
    rng = np.random.default_rng(40 + L)
    big = 250 if L == 1 else 3000
    for target in range(TILE - 8, TILE + 9):
        lens, at = [], 0
        while target - at > big + L:
            n = int(rng.integers(big // 2, big + 1)); lens.append(n); at += L + n
        rest = target - at - L              # the record that ends at `target`
        if rest < 0:
            lens[-1] += rest; rest = None
        else:
            lens.append(rest)
        lens += [int(x) for x in rng.integers(0, 40, size=6)] + [big] * 3
        s, idx = made_stream(rng, lens, junk=int(rng.integers(0, 16)))
        out = forward(ctx, s, idx, None, L)
        offs = np.concatenate([[0], np.cumsum(np.array(lens) + L)])
        assert target in offs
        back = reverse(ctx, out, [0], [len(out)], L, 3 + (target & 1))
        assert len(back) == len(out) + (3 + (target & 1) - L) * len(lens)


@pytest.mark.parametrize("sc", [3, 4])
def test_tile_boundaries_inside_start_codes(ctx, sc):
    rng = np.random.default_rng(50 + sc)
    L = 2
    for target in range(TILE - 8, TILE + 9):           # the output offset a start code begins at
        lens, at = [], 0
        while target - at > 3000 + sc:
            n = int(rng.integers(1500, 3001)); lens.append(n); at += sc + n
        lens.append(target - at - sc) if target - at - sc >= 0 else lens.__setitem__(-1, lens[-1] + target - at - sc)
        lens += [int(x) for x in rng.integers(0, 40, size=6)] + [3000] * 3
        data = np.concatenate([np.concatenate([np.frombuffer(int(n).to_bytes(L, "big"), np.uint8), rng.integers(0, 256, size=int(n), dtype=np.uint8)])
                               for n in lens])
        junk = int(rng.integers(0, 16))
        data = np.concatenate([rng.integers(0, 256, size=junk, dtype=np.uint8), data])
        assert target in np.concatenate([[0], np.cumsum(np.array(lens) + sc)])
        reverse(ctx, data, [junk], [len(data) - junk], L, sc)


def test_dense_pieces(ctx):
    rng = np.random.default_rng(17)
    # 600 KB of payloads of 0-3 bytes, L = 1: up to 16 pieces in a chunk, far more than 2048 in a tile
    lens = rng.integers(0, 4, size=240000)
    s, idx = made_stream(rng, lens)
    assert len(s) > 600000
    out = forward(ctx, s, idx, None, 1)
    assert len(out) / TILE * 2048 < len(lens)
    reverse(ctx, out, [0], [len(out)], 1, 3)
    both_ways(ctx, s, idx, rng.random(len(idx)) < 0.5, 1, 4, rng)
    # payloads of 1-61 bytes, every other NAL
    lens = rng.integers(1, 62, size=18000)
    s, idx = made_stream(rng, lens)
    keep = (np.arange(len(idx)) % 2) == 0
    both_ways(ctx, s, idx, keep, 1, 3, rng)
    both_ways(ctx, s, idx, ~keep, 2, 4, rng)


def test_every_misalignment(ctx):
    rng = np.random.default_rng(19)
    lens = [int(x) for x in rng.integers(20, 6000, size=66)]
    for junk in range(16):
        s, idx = made_stream(np.random.default_rng(77), lens, junk=junk)     # the same stream behind 0..15 bytes
        assert len(s) > 190000
        out = forward(ctx, s, idx, None, 4)
        # the way back with the records behind `junk` bytes, 3-byte codes: source minus output offset takes every value mod 16
        data = np.concatenate([rng.integers(0, 256, size=junk, dtype=np.uint8), out])
        reverse(ctx, data, [junk], [len(out)], 4, 3)


def test_round_trip_of_a_gop_with_the_au_chain(ctx):
    """index + parse -> access units -> hbs_au_keep of one GOP with its parameter sets -> records with the sample table -> back"""
    import torch
    from tests.hevc_synth import Synth, annexb
    from tests.test_gpu_au import parse_stream
    g = Synth(3, rich=False)
    rng = np.random.RandomState(4)
    nals = []
    for pic in range(48):
        if pic % 16 == 0:
            nals += [g.vps(), g.sps_nal(3840, 2160, ctb_log2=6), g.pps_nal(force={"tiles": 0})]
        tid = 1 if pic % 4 == 0 else 2 if pic % 4 == 2 else 3           # hierarchical: three temporal sub-layers
        for sl in range(4):
            pay = rng.randint(0, 256, size=int(rng.randint(2000, 6000))).astype(np.uint8).tobytes()
            nt = 19 if pic % 16 == 0 else 1
            nals.append(g.slice_nal(nt, first=(sl == 0), payload=pay, address=sl * 510, tid=tid))
    s = np.frombuffer(annexb(nals), dtype=np.uint8).copy()
    d, n, index, parsed, cc, structs = parse_stream(ctx, s.tobytes(), len(nals))
    assert n == len(nals)
    idx = index[: n * 32].cpu().numpy().view(F.NAL_ENTRY).copy()
    au, nal_au, _, _ = ctx.access_units(index, parsed, cc, structs, n)
    assert len(au) == 48
    d_au = torch.from_numpy(nal_au.view(np.int32).copy()).cuda()
    keep = ctx.au_keep(d_au, parsed, n, 16, 16, param_sets=True)         # the second GOP, with the parameter sets in force
    k = keep.cpu().numpy().astype(bool)
    assert 16 * 4 <= k.sum() < n
    out, io, so, sm = ctx.annexb_to_lenpref(d, idx, keep=keep, length_size=4, nal_au=d_au, n_aus=len(au))
    want_out, want_io, want_so, want_s = R.to_lenpref_ref(s, idx, k, 4, nal_au, len(au))
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(io, want_io) and np.array_equal(so, want_so)
    summary_matches(sm, want_s)
    kk = np.nonzero(k)[0]
    first_rec = {}                       # AU -> its first kept record
    for j, q in enumerate(kk):
        first_rec.setdefault(int(nal_au[q]), j)
    for a in range(len(au)):             # each sample begins at its AU's first kept record; an AU with nothing kept is empty
        if a in first_rec:
            assert int(so[a]) == int(io["start"][first_rec[a]]) - 4 and so[a + 1] > so[a]
        else:
            assert so[a] == so[a + 1]
    # back, samples in table order: L equals the start code's size, so the sample offsets stay what they were
    size = np.diff(so.astype(np.int64)).astype(np.uint64)
    back, so2, bs = ctx.lenpref_to_annexb(out, so[:-1].copy(), size)
    b = back.cpu().numpy()
    assert np.array_equal(so2, so) and int(bs["nal_count"]) == len(kk) and int(bs["nal_found"]) == len(au)
    got, _, _ = ctx.index_extract(back)
    pay = [s[int(e["start"]):int(e["end"])] for e in idx[k]]
    assert len(got) == len(pay) and all(np.array_equal(b[int(e["start"]):int(e["end"])], p) for e, p in zip(got, pay))
    for a, j in first_rec.items():       # d_sample_off_out marks the AUs: each begins at the start code of its first NAL
        assert int(so2[a]) == int(got["start"][j]) - 4
    # shuffled, with gaps: the samples laid out in another order in a larger buffer come out in table order
    order = np.random.default_rng(3).permutation(len(au))
    buf = np.full(len(want_out) + 64 * len(au) + 64, 0xA7, dtype=np.uint8)
    off = np.zeros(len(au), dtype=np.uint64)
    at = 13
    for a in order:
        off[a] = at
        buf[at: at + int(size[a])] = want_out[int(so[a]): int(so[a + 1])]
        at += int(size[a]) + int(a % 5) * 11 + 1
    assert np.array_equal(reverse(ctx, buf[:at + 7], off, size, 4, 4), b)
    pick = order[:20]                    # some of them, in shuffled order, 3-byte start codes
    reverse(ctx, buf[:at + 7], off[pick], size[pick], 4, 3)


def test_errors_capacity_plan_and_empty(ctx, orc):
    import torch
    rng = np.random.default_rng(9)
    idx = []
    while len(idx) <= 10:
        s = F.random_stream(rng, 150000, 900)
        idx, _, _ = orc.index_extract(s)
    keep = rng.random(len(idx)) < 0.6
    au, n_aus = random_aus(rng, len(idx))
    want = R.to_lenpref_ref(s, idx, keep, 4, au, n_aus)
    out = forward(ctx, s, idx, keep, 4, au, n_aus)
    forward(ctx, s, idx, keep, 4, au, n_aus, out_cap=len(out) - 1, want_error=R.E_CAPACITY)      # right sizes, no byte written
    # an inconsistent index
    for bad in (5, -1, 7):
        a = idx.copy()
        if bad == 5:
            a["start"][5] = a["end"][5] + 1
        elif bad == -1:
            a["end"][-1] = len(s) + 1
        else:
            a["start"][7] = a["end"][6] - 1
        assert not F.consistent(a, len(s))
        forward(ctx, s, a, None, 4, au, n_aus, out_cap=2 * len(s), want_error=R.E_ARG)
    # a bad AU table
    for k, v in ((0, 1), (len(idx) // 2, int(au[len(idx) // 2 - 1]) + 2), (len(idx) - 1, int(au[-1]) + 1)):
        b = au.copy(); b[k] = v
        forward(ctx, s, idx, keep, 4, b, n_aus, out_cap=2 * len(s), want_error=R.E_ARG)
    forward(ctx, s, idx, keep, 4, au, n_aus + 1, out_cap=2 * len(s), want_error=R.E_ARG)
    forward(ctx, s, idx[:0], None, 4, au[:0], 1, out_cap=64, want_error=R.E_ARG)
    # a length overflow: only a kept NAL has to fit
    lens = [100, 255, 256, 3]
    s2, i2 = made_stream(rng, lens)
    forward(ctx, s2, i2, None, 1, out_cap=1000, want_error=R.E_ARG)
    forward(ctx, s2, i2, [1, 1, 0, 1], 1)
    lens = [65535, 65536, 7]
    s2, i2 = made_stream(rng, lens)
    forward(ctx, s2, i2, None, 2, out_cap=200000, want_error=R.E_ARG)
    forward(ctx, s2, i2, [1, 0, 1], 2)
    forward(ctx, s2, i2, None, 4)
    # empty input, nothing kept, an empty kept NAL
    forward(ctx, s, idx[:0], None, 4, au[:0], 0)
    forward(ctx, s[:0], idx[:0], None, 2)
    forward(ctx, s, idx, np.zeros(len(idx), bool), 4, au, n_aus)
    e = idx[:3].copy(); e["end"][1] = e["start"][1]
    forward(ctx, s, e, None, 2, np.array([0, 1, 2], np.uint32), 3)
    # the reverse: malformed chains (reserved[0] names the lowest bad sample), nal_cap and out_cap one short, empty
    so = want[2].astype(np.int64)
    off, size = so[:-1].copy(), np.diff(so)
    full = [a for a in range(n_aus) if size[a] > 8]
    back = reverse(ctx, out, off, size, 4, 3)
    recs = int(want[3]["nal_count"])
    for a, (doff, dsize) in ((full[3], (0, -1)), (full[1], (0, 2)), (full[2], (1, 0))):
        o2, z2 = off.copy(), size.copy(); o2[a] += doff; z2[a] += dsize
        if a == full[2]:
            z2[full[4]] -= 3               # two bad samples: the lowest is reported
        reverse(ctx, out, o2, z2, 4, 3, want_error=R.E_ARG)
    z2 = size.copy(); z2[-1] += 1
    reverse(ctx, out, off, z2, 4, 3, want_error=R.E_ARG)             # leaves the buffer
    o2 = off.astype(np.uint64).copy(); o2[2] = (1 << 64) - 2
    reverse(ctx, out, o2, size, 4, 3, want_error=R.E_ARG)            # the sum wraps
    reverse(ctx, out, off, size, 4, 3, nal_cap=recs - 1, want_error=R.E_CAPACITY)
    reverse(ctx, out, off, size, 4, 3, out_cap=len(back) - 1, want_error=R.E_CAPACITY)
    reverse(ctx, out, off[:0], size[:0], 4, 3)
    reverse(ctx, out[:0], [0, 0], [0, 0], 1, 4)
    reverse(ctx, np.zeros(7, np.uint8), [0, 2], [4, 5], 1, 3)         # zero-length records only: bare start codes
    reverse(ctx, out, off, size, 4, 3, nal_cap=(1 << 64) - 1)        # "no limit": out_cap bounds the piece table
    reverse(ctx, out, off, size, 4, 3, nal_cap=(1 << 64) - 1, out_cap=len(back) - 1, want_error=R.E_CAPACITY)
    # refused at once: bad length_size / startcode_bytes, misaligned pointers; nothing is written
    d_s, d_i, summ = dev(s), dev(idx), torch.full((80,), CAN, dtype=torch.uint8, device="cuda")
    outb = canary(len(out) + 16)
    for L in (0, 3, 5, 8, -1):
        assert ctx.annexb_to_lenpref_async(d_s, len(s), d_i, len(idx), outb, None, summ, length_size=L) == -3
        assert ctx.lenpref_to_annexb_async(d_s, len(s), dev(off), dev(size), n_aus, outb, None, summ, length_size=L, nal_cap=recs) == -3
    for sc in (0, 2, 5):
        assert ctx.lenpref_to_annexb_async(d_s, len(s), dev(off), dev(size), n_aus, outb, None, summ, startcode_bytes=sc, nal_cap=recs) == -3
    d_off, d_size = dev(off), dev(size)
    assert ctx.lenpref_to_annexb_async(d_s, len(s), d_off, d_size, n_aus, outb, None, summ, nal_cap=recs, out_cap=(1 << 46) + 1) == -3
    assert ctx.annexb_to_lenpref_async(d_s[1:], len(s) - 1, d_i, len(idx), outb, None, summ) == -3
    assert ctx.annexb_to_lenpref_async(d_s, len(s), d_i[4:], len(idx) - 1, outb, None, summ) == -3
    assert ctx.annexb_to_lenpref_async(d_s, len(s), d_i, len(idx), outb[8:], None, summ) == -3
    assert ctx.annexb_to_lenpref_async(d_s, len(s), d_i, len(idx), outb, None, summ[8:]) == -3
    assert ctx.annexb_to_lenpref_async(d_s, len(s), d_i, len(idx), outb, None, summ, nal_au=dev(au)[2:], n_aus=n_aus) == -3
    assert ctx.annexb_to_lenpref_async(d_s, len(s), d_i, len(idx), outb, None, summ, nal_au=dev(au), n_aus=n_aus, sample_off=outb[4:]) == -3
    assert ctx.lenpref_to_annexb_async(d_s[8:], len(s) - 8, d_off, d_size, n_aus, outb, None, summ, nal_cap=recs) == -3
    assert ctx.lenpref_to_annexb_async(d_s, len(s), d_off[4:], d_size, n_aus - 1, outb, None, summ, nal_cap=recs) == -3
    assert ctx.lenpref_to_annexb_async(d_s, len(s), d_off, d_size, n_aus, outb, outb[4:], summ, nal_cap=recs) == -3
    assert ctx.lenpref_to_annexb_async(d_s, len(s), d_off, d_size, n_aus, outb[1:], None, summ, nal_cap=recs) == -3
    torch.cuda.synchronize()
    assert (outb.cpu().numpy() == CAN).all() and (summ.cpu().numpy() == CAN).all()


def test_every_accepted_alignment_on_carved_buffers(ctx):
    from tests import _carve as K
    rng = np.random.default_rng(61)
    lens = [int(x) for x in rng.integers(0, 900, size=60)]
    s, idx = made_stream(rng, lens, junk=5)
    keep = (rng.random(len(idx)) < 0.7).astype(np.uint8)
    au, n_aus = random_aus(rng, len(idx))
    want_out, want_io, want_so, want_s = R.to_lenpref_ref(s, idx, keep, 2, au, n_aus)
    nk = len(want_io)
    for it in range(len(K.OFFS1)):
        o16, o8, o4, o1 = K.OFFS16[it % len(K.OFFS16)], K.OFFS8[it % len(K.OFFS8)], K.OFFS4[it % len(K.OFFS4)], K.OFFS1[it]
        bufs = dict(s=K.carve(len(s), o16), i=K.carve(idx.nbytes, o8), k=K.carve(len(keep), o1), a=K.carve(au.nbytes, o4),
                    out=K.carve(len(want_out), K.OFFS16[(it + 3) % len(K.OFFS16)]), io=K.carve(len(idx) * 32, K.OFFS8[(it + 5) % len(K.OFFS8)]),
                    so=K.carve((n_aus + 1) * 8, K.OFFS8[(it + 7) % len(K.OFFS8)]), sm=K.carve(64, K.OFFS16[(it + 1) % len(K.OFFS16)]))
        for name, data in (("s", s), ("i", idx), ("k", keep), ("a", au)):
            bufs[name][1].put(data)
        v = {k: b[0] for k, b in bufs.items()}
        assert ctx.annexb_to_lenpref_async(v["s"], len(s), v["i"], len(idx), v["out"], v["io"], v["sm"], keep=v["k"], length_size=2,
                                           nal_au=v["a"], n_aus=n_aus, sample_off=v["so"], out_cap=len(want_out)) == 0
        summary_matches(ctx.read_summary(v["sm"]), want_s)
        assert np.array_equal(bufs["out"][1].get(), want_out)
        assert np.array_equal(bufs["io"][1].get()[:nk * 32].view(F.NAL_ENTRY), want_io)
        assert np.array_equal(bufs["so"][1].get().view(np.uint64), want_so)
        for name, b in bufs.items():
            assert b[1].intact(), (name, b[1].damage())
        # the way back: the records behind o16 junk-free bytes of another carved buffer, the tables at 8-byte offsets
        off, size = want_so[:-1].copy(), np.diff(want_so.astype(np.int64)).astype(np.uint64)
        back_want, so_want, bs_want = R.to_annexb_ref(want_out, off, size, 2, 3)
        rb = dict(d=K.carve(len(want_out), o16), off=K.carve(off.nbytes, o8), size=K.carve(size.nbytes, K.OFFS8[(it + 2) % len(K.OFFS8)]),
                  out=K.carve(len(back_want), K.OFFS16[(it + 4) % len(K.OFFS16)]), so=K.carve((n_aus + 1) * 8, K.OFFS8[(it + 6) % len(K.OFFS8)]),
                  sm=K.carve(64, K.OFFS16[(it + 2) % len(K.OFFS16)]))
        for name, data in (("d", want_out), ("off", off), ("size", size)):
            rb[name][1].put(data)
        v = {k: b[0] for k, b in rb.items()}
        assert ctx.lenpref_to_annexb_async(v["d"], len(want_out), v["off"], v["size"], n_aus, v["out"], v["so"], v["sm"], length_size=2,
                                           startcode_bytes=3, nal_cap=nk, out_cap=len(back_want)) == 0
        summary_matches(ctx.read_summary(v["sm"]), bs_want)
        assert np.array_equal(rb["out"][1].get(), back_want) and np.array_equal(rb["so"][1].get().view(np.uint64), so_want)
        for name, b in rb.items():
            assert b[1].intact(), (name, b[1].damage())


def test_stream_above_4gib(ctx):
    """a few NALs near 1 GiB among small ones, L = 4: offsets above 4 GiB, payloads spread over many tiles.  Compared by the
    sample table and output index arithmetic, a device re-scan of the way back, and slices of the outputs against the stream"""
    import torch
    rng = np.random.default_rng(23)
    sizes = []
    for k in range(4):
        sizes += [int(rng.integers(100, 20000)) for _ in range(int(rng.integers(200, 600)))]
        sizes.append((1 << 30) + int(rng.integers(-5000, 5000)))
    sizes += [int(rng.integers(100, 20000)) for _ in range(300)]
    lens = np.array(sizes, dtype=np.int64)
    sc = np.where(rng.random(len(lens)) < 0.3, 4, 3)
    total = int((lens + sc).sum())
    assert total > (4 << 30)
    d = torch.randint(1, 256, (total,), dtype=torch.uint8, device="cuda")          # no zero bytes: no start code but ours
    pos = np.concatenate([[0], np.cumsum(lens + sc)[:-1]])
    st = torch.from_numpy(pos).cuda()
    four = torch.from_numpy(sc == 4).cuda()
    d[st] = 0
    d[st + 1] = 0
    d[st + 2] = torch.where(four, 0, 1).to(torch.uint8)
    d[(st + 3)[four]] = 1
    idx, _, s0 = ctx.index_extract(d, index_cap=len(lens) + 16, want_rbsp=False)
    assert len(idx) == len(lens) and np.array_equal(idx["start"].astype(np.int64), pos + sc)
    au = (np.arange(len(lens)) // 7).astype(np.uint32)
    n_aus = int(au[-1]) + 1
    out, io, so, sm = ctx.annexb_to_lenpref(d, idx, length_size=4, nal_au=au, n_aus=n_aus)
    rec = np.concatenate([[0], np.cumsum(lens + 4)])
    assert int(sm["stream_bytes"]) == int(rec[-1]) == out.numel() and int(sm["nal_count"]) == len(lens) and int(rec[-1]) > (1 << 32)
    assert np.array_equal(io["start"].astype(np.int64), rec[:-1] + 4) and np.array_equal(io["end"].astype(np.int64), rec[1:])
    firsts = np.concatenate([np.flatnonzero(np.diff(au, prepend=-1)), [len(lens)]])
    assert np.array_equal(so.astype(np.int64), rec[firsts])

    def slices(o, ooff, skip):
        for j in range(len(lens)):
            a, b = int(ooff[j]) + skip, int(ooff[j]) + skip + int(lens[j])
            w = min(4096, b - a)
            x, y = int(idx["start"][j]), int(idx["end"][j])
            assert torch.equal(o[a:a + w], d[x:x + w]) and torch.equal(o[b - w:b], d[y - w:y])
        for _ in range(100):
            j = int(rng.integers(0, len(lens)))
            f = int(rng.integers(0, lens[j]))
            w = min(int(rng.integers(1, 1 << 20)), int(lens[j]) - f)
            assert torch.equal(o[int(ooff[j]) + skip + f: int(ooff[j]) + skip + f + w], d[int(idx["start"][j]) + f: int(idx["start"][j]) + f + w])
    slices(out, rec, 4)
    hdr = out[torch.from_numpy(rec[:-1, None] + np.arange(4)[None, :]).cuda()].cpu().numpy().astype(np.int64)
    assert np.array_equal((hdr[:, 0] << 24) | (hdr[:, 1] << 16) | (hdr[:, 2] << 8) | hdr[:, 3], lens)
    back, so2, bs = ctx.lenpref_to_annexb(out, so[:-1], np.diff(so.astype(np.int64)).astype(np.uint64), length_size=4, startcode_bytes=3)
    rec3 = np.concatenate([[0], np.cumsum(lens + 3)])
    assert int(bs["stream_bytes"]) == int(rec3[-1]) == back.numel() and int(bs["nal_count"]) == len(lens)
    assert np.array_equal(so2.astype(np.int64), rec3[firsts])
    del out
    torch.cuda.empty_cache()
    got, _, gs = ctx.index_extract(back, index_cap=len(lens) + 16, want_rbsp=False)
    assert np.array_equal(got["start"].astype(np.int64), rec3[:-1] + 3) and np.array_equal(got["end"].astype(np.int64), rec3[1:])
    slices(back, rec3, 3)


def test_two_contexts_at_the_same_time(orc):
    import torch
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(29)
    jobs = []
    for k in range(2):
        s = F.random_stream(rng, 4 << 20, 3000)
        idx, _, _ = orc.index_extract(s)
        keep = rng.random(len(idx)) < 0.5
        au, n_aus = random_aus(rng, len(idx))
        fw = R.to_lenpref_ref(s, idx, keep, 4, au, n_aus)
        so = fw[2].astype(np.int64)
        bw = R.to_annexb_ref(fw[0], so[:-1], np.diff(so), 4, 4)
        jobs.append((s, idx, keep, au, n_aus, fw, bw))
    streams = [torch.cuda.Stream() for _ in jobs]
    ctxs, bufs = [], []
    for (s, idx, keep, au, n_aus, fw, bw), st in zip(jobs, streams):
        with torch.cuda.stream(st):
            c = hbs.Context(0)
            so = fw[2].astype(np.int64)
            b = dict(s=dev(s), i=dev(idx), k=dev(keep.astype(np.uint8)), a=dev(au), out=canary(len(fw[0])), io=canary(len(idx) * 32),
                     so=canary((n_aus + 1) * 8), sm=torch.zeros(64, dtype=torch.uint8, device="cuda"), size=dev(np.diff(so).astype(np.uint64)),
                     back=canary(len(bw[0])), so2=canary((n_aus + 1) * 8), sm2=torch.zeros(64, dtype=torch.uint8, device="cuda"))
            ctxs.append(c)
            bufs.append(b)
    for r in range(3):
        for (s, idx, keep, au, n_aus, fw, bw), st, c, b in zip(jobs, streams, ctxs, bufs):
            with torch.cuda.stream(st):
                assert c.annexb_to_lenpref_async(b["s"], len(s), b["i"], len(idx), b["out"], b["io"], b["sm"], keep=b["k"], nal_au=b["a"],
                                                 n_aus=n_aus, sample_off=b["so"], out_cap=len(fw[0])) == 0
                # the forward call's own sample table, on the device, is the way back's
                assert c.lenpref_to_annexb_async(b["out"], len(fw[0]), b["so"], b["size"], n_aus, b["back"], b["so2"], b["sm2"],
                                                 nal_cap=len(fw[1]), out_cap=len(bw[0])) == 0
    torch.cuda.synchronize()
    for (s, idx, keep, au, n_aus, fw, bw), c, b in zip(jobs, ctxs, bufs):
        o, k2 = b["out"].cpu().numpy(), b["back"].cpu().numpy()
        assert np.array_equal(o[: len(fw[0])], fw[0]) and (o[len(fw[0]):] == CAN).all()
        assert np.array_equal(b["io"][: len(fw[1]) * 32].cpu().numpy().view(F.NAL_ENTRY), fw[1])
        assert np.array_equal(b["so"][: (n_aus + 1) * 8].cpu().numpy().view(np.uint64), fw[2])
        assert np.array_equal(k2[: len(bw[0])], bw[0]) and (k2[len(bw[0]):] == CAN).all()
        assert np.array_equal(b["so2"][: (n_aus + 1) * 8].cpu().numpy().view(np.uint64), bw[1])
        summary_matches(c.read_summary(b["sm"]), fw[3])
        summary_matches(c.read_summary(b["sm2"]), bw[2])
        c.close()


def test_timing_covers_both_calls(ctx):
    rng = np.random.default_rng(31)
    s, idx = made_stream(rng, [int(x) for x in rng.integers(100, 5000, size=400)])
    ctx.enable_timing(True)
    try:
        out = forward(ctx, s, idx, None, 4)
        assert ctx.kernel_ms() > 0 and ctx.kernel_ms_back(1) > 0
        reverse(ctx, out, [0], [len(out)], 4, 4)
        assert ctx.kernel_ms() > 0 and ctx.kernel_ms_back(1) > 0
    finally:
        ctx.enable_timing(False)
