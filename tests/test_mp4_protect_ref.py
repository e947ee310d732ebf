"""tests/_mp4_protect_ref.py against protected fragments written out by hand, against its own independent walker and the reader of
tests/_mp4_read_ref.py; the library's two host functions (hbs_mp4_protect_bytes_host, hbs_mp4_init_protect_host) against it.
No GPU."""
import struct

import numpy as np
import pytest

from tests import _mp4_protect_ref as P
from tests import _mp4_read_ref as RR
from tests import _mp4_ref as R

VPS = bytes([0x40, 0x01, 0x0C, 0x01, 0xFF, 0xFF, 0x01, 0x60])
SPS = bytes([0x42, 0x01, 0x01, 0x01, 0x60, 0x00, 0x00, 0x03, 0x00, 0x90, 0x00, 0x00, 0x03, 0x00, 0x00, 0x03, 0x00, 0x78, 0xA0, 0x03, 0xC0])
PPS = bytes([0x44, 0x01, 0xC1, 0x72, 0xB4, 0x62, 0x40])


def table(per_sample):
    """[[(clear, protect)]] a sample -> (sub_first, sub)"""
    first = np.cumsum([0] + [len(e) for e in per_sample]).astype(np.uint64)
    sub = np.array([x for e in per_sample for x in e], dtype=P.SUBSAMPLE).reshape(-1)
    return first, sub


def one_input(per_sample, seed, dt=1000, seq=7, track=3):
    """one fragment of hbs_mp4_fragment's form whose sample sizes are the entries' sums -> (bytes, FRAG table of one, iv)"""
    rng = np.random.default_rng(seed)
    sizes = [sum(a + b for a, b in e) for e in per_sample]
    samples = [(100 + i, 0x02000000 if i == 0 else 0x01010000, 5 * i, rng.integers(0, 256, z, dtype=np.uint8).tobytes()) for i, z in enumerate(sizes)]
    b = R.one_fragment(seq, track, dt, samples)
    frag = np.array([(0, len(b), 40, dt, len(sizes), seq, 1, 0)], dtype=R.FRAG)
    return b, frag, rng.integers(1, 256, 16 * len(sizes), dtype=np.uint8)


def test_iv_size_8_two_samples_by_hand():
    per = [[(5, 20)], [(3, 0), (0, 7)]]
    b, frag, iv = one_input(per, 1)
    iv[8:16] = 0
    iv[24:32] = 0
    assert len(b) == 88 + 32 + 8 + 35
    want = (struct.pack(">I4s", 213, b"moof") + b[8:24] + struct.pack(">I4s", 189, b"traf") + b[32:68]
            + struct.pack(">I4sIII", 52, b"trun", 0x01000F01, 2, 221) + b[88:120]
            + struct.pack(">I4sIBI", 19, b"saiz", 0, 0, 2) + bytes([16, 22])
            + struct.pack(">I4sIII", 20, b"saio", 0, 1, 175)
            + struct.pack(">I4sII", 54, b"senc", 2, 2)
            + bytes(iv[0:8]) + struct.pack(">HHI", 1, 5, 20) + bytes(iv[16:24]) + struct.pack(">HHIHI", 2, 3, 0, 0, 7)
            + b[120:])
    assert len(want) == len(b) + 53 + 11 * 2 + 6 * 3 and want[213:221] == struct.pack(">I4s", 43, b"mdat")
    first, sub = table(per)
    out, so, ss, fr, s = P.protect(b, frag, first, sub, iv, 8)
    assert out.tobytes() == want
    assert so.tolist() == [221, 246] and ss.tolist() == [25, 10]
    assert fr.tolist() == [(0, len(want), 40, 1000, 2, 7, 1, 0)]
    assert s == P.summary(0, 1, 2, 3, len(want))


def test_iv_size_16_and_a_sample_of_no_entries_by_hand():
    per = [[], [(2, 9)]]
    b, frag, iv = one_input(per, 2)
    want = (struct.pack(">I4s", 141 + 35 * 2 + 6, b"moof") + b[8:24] + struct.pack(">I4s", 217 - 24, b"traf") + b[32:68]
            + struct.pack(">I4sIII", 52, b"trun", 0x01000F01, 2, 225) + b[88:120]
            + struct.pack(">I4sIBI", 19, b"saiz", 0, 0, 2) + bytes([18, 24])
            + struct.pack(">I4sIII", 20, b"saio", 0, 1, 175)
            + struct.pack(">I4sII", 16 + 18 + 24, b"senc", 2, 2)
            + bytes(iv[0:16]) + struct.pack(">H", 0) + bytes(iv[16:32]) + struct.pack(">HHI", 1, 2, 9)
            + b[120:])
    first, sub = table(per)
    out, so, ss, fr, s = P.protect(b, frag, first, sub, iv, 16)
    assert out.tobytes() == want and so.tolist() == [225, 225] and ss.tolist() == [0, 11] and s == P.summary(0, 1, 2, 1, len(b) + 53 + 38 + 6)


def test_iv_size_0_and_a_split_clear_run_by_hand():
    per = [[(65535, 0), (10, 30)]]
    b, frag, _ = one_input(per, 3)
    want = (struct.pack(">I4s", 141 + 19 + 12, b"moof") + b[8:24] + struct.pack(">I4s", 148, b"traf") + b[32:68]
            + struct.pack(">I4sIII", 36, b"trun", 0x01000F01, 1, 180) + b[88:104]
            + struct.pack(">I4sIBI", 18, b"saiz", 0, 0, 1) + bytes([14])
            + struct.pack(">I4sIII", 20, b"saio", 0, 1, 158)
            + struct.pack(">I4sII", 16 + 2 + 12, b"senc", 2, 1)
            + struct.pack(">HHIHI", 2, 65535, 0, 10, 30)
            + b[104:])
    first, sub = table(per)
    out, so, ss, fr, s = P.protect(b, frag, first, sub, None, 0)
    assert out.tobytes() == want and so.tolist() == [180] and ss.tolist() == [65575]
    assert s == P.summary(0, 1, 1, 2, len(b) + 53 + 3 + 12)


def random_input(rng, n_frags, V, max_entries=None, gaps=True):
    """fragments of 1..40 samples somewhere in a buffer -> (data, FRAG table, sub_first, sub, iv, per-sample entries)"""
    cap = P.max_entries(V) if max_entries is None else max_entries
    buf, frags, per, au = bytearray(), [], [], 500
    for r in range(n_frags):
        S = int(rng.integers(1, 41))
        mine = [[(int(rng.integers(0, 70)), int(rng.integers(0, 300))) for _ in range(int(rng.integers(0, min(cap, 6) + 1)))] for _ in range(S)]
        if rng.integers(4) == 0:
            mine[int(rng.integers(S))] = [(int(rng.integers(0, 9)), int(rng.integers(0, 9)))] * cap
        b, f, _ = one_input(mine, int(rng.integers(1 << 30)), dt=int(rng.integers(0, 1 << 40)), seq=r + 9)
        if gaps:
            buf += rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        f["out_off"], f["first_au"] = len(buf), au
        au += S
        buf += b
        frags.append(f[0])
        per += mine
    first, sub = table(per)
    iv = rng.integers(0, 256, 16 * len(per), dtype=np.uint8)
    if V == 8:
        iv.reshape(-1, 16)[:, 8:] = 0
    return np.frombuffer(bytes(buf), dtype=np.uint8), np.array(frags, dtype=R.FRAG), first, sub, iv, per


@pytest.mark.parametrize("V", (0, 8, 16))
def test_walker_and_reader_on_the_reference_output(V):
    rng = np.random.default_rng(70 + V)
    data, frags, first, sub, iv, per = random_input(rng, 9, V)
    out, so, ss, fr, s = P.protect(data, frags, first, sub, iv, V)
    assert s["error"] == 0 and s["stream_bytes"] == len(out) == int(frags["out_bytes"].sum()) + 53 * 9 + (V + 3) * len(per) + 6 * len(sub)
    # the walker, which knows only saio's offset and saiz's sizes, returns exactly the tables that went in
    got = P.walk_protected(out, V)
    assert [(g["off"], g["bytes"]) for g in got] == [(int(f["out_off"]), int(f["out_bytes"])) for f in fr]
    flat = [x for g in got for x in g["samples"]]
    assert [e for _, e in flat] == per
    assert all(iv_ == bytes(iv[16 * i:16 * i + V]) for i, (iv_, _) in enumerate(flat))
    # the reader of hbs_mp4_samples' reference: the stated sample offsets, and the times and flags of the input
    prm = RR.read_params()
    o2, z2, d2, p2, f2, fr2, s2 = RR.samples(out, [(int(f["out_off"]), int(f["out_bytes"])) for f in fr], prm)
    o1, z1, d1, p1, f1, fr1, s1 = RR.samples(data, [(int(f["out_off"]), int(f["out_bytes"])) for f in frags], prm)
    assert s2["error"] == 0 and np.array_equal(o2, so) and np.array_equal(z2, ss) and np.array_equal(z1, ss)
    assert np.array_equal(d1, d2) and np.array_equal(p1, p2) and np.array_equal(f1, f2)
    for a, b in zip(fr1, fr2):
        assert a.tolist()[3:] == b.tolist()[3:]
    # every mdat whole
    for f_in, f_out, S in zip(frags, fr, frags["samples"].tolist()):
        a, b = int(f_in["out_off"]) + 88 + 16 * S, int(f_in["out_off"] + f_in["out_bytes"])
        assert out[int(f_out["out_off"] + f_out["out_bytes"]) - (b - a): int(f_out["out_off"] + f_out["out_bytes"])].tobytes() == data[a:b].tobytes()


def test_each_rule_in_the_reference():
    rng = np.random.default_rng(5)
    data, frags, first, sub, iv, per = random_input(rng, 6, 8)
    N = len(per)
    ok = P.protect(data, frags, first, sub, iv, 8)[4]
    assert ok["error"] == 0

    def err(**kw):
        a = dict(data=data, frags=frags, sub_first=first, sub=sub, iv=iv, V=8)
        a.update(kw)
        out, _, _, _, s = P.protect(**a)
        assert out is None and s["error"] == P.E_ARG
        return s["reserved"]

    # fragment rule: one patched word each, the lowest named, a fragment error hides a sample error
    off3, S3 = int(frags["out_off"][3]), int(frags["samples"][3])
    bad_first = first.copy()
    bad_first[1] = 99999
    for at in (76, 80, 84, 88 + 16 * S3, 4, 28, 36, 52, 72, 0, 24, 68):
        d = data.copy()
        d[off3 + at + 3] ^= 1
        assert err(data=d) == [0, 4, 0] and err(data=d, sub_first=bad_first) == [0, 4, 0]
    for at in (20, 44, 60):                                  # sequence, track id, decode time: not constrained
        d = data.copy()
        d[off3 + at] ^= 0x55
        assert P.protect(d, frags, first, sub, iv, 8)[4]["error"] == 0
    f = frags.copy()
    f["out_bytes"][5] += 1                                   # leaves the buffer (and its mdat size is another)
    assert err(frags=f) == [0, 6, 0]
    f = frags.copy()
    f["first_au"][2] += 1
    assert err(frags=f) == [0, 3, 0]
    assert err(sub_first=np.concatenate([first, first[-1:]])) == [0, 6, 0]          # one sample more than the fragments have
    # sample rule
    assert err(sub_first=bad_first)[0] == 1
    j = N - 1
    bad_iv = iv.copy()
    bad_iv[16 * j + 15] = 1
    assert err(iv=bad_iv) == [j + 1, 0, 0]
    j = next(i for i in range(3, N) if first[i + 1] > first[i])          # a sample that has entries
    s2 = sub.copy()
    e = int(first[j])
    s2["protect"][e] += 1
    assert err(sub=s2) == [j + 1, 0, 0]
    s2 = sub.copy()
    s2["clear"][e], s2["protect"][e] = 65536, int(s2["clear"][e]) + int(s2["protect"][e]) - 65536 & 0xFFFFFFFF
    assert err(sub=s2) == [j + 1, 0, 0]
    # capacity
    out, _, _, _, s = P.protect(data, frags, first, sub, iv, 8, out_cap=ok["stream_bytes"] - 1)
    assert out is None and s == dict(ok, error=P.E_CAPACITY)


def test_entry_cap_is_the_saiz_byte():
    for V in (0, 8, 16):
        cap = P.max_entries(V)
        assert V + 2 + 6 * cap <= 255 < V + 2 + 6 * (cap + 1)
    assert [P.max_entries(V) for V in (0, 8, 16)] == [42, 40, 39]
    for V, cap in ((0, 42), (8, 40), (16, 39)):
        for n, good in ((cap, True), (cap + 1, False)):
            per = [[(1, 1)] * n]
            b, frag, iv = one_input(per, 9)
            iv[8:] = 0
            first, sub = table(per)
            s = P.protect(b, frag, first, sub, iv, V)[4]
            assert (s["error"] == 0) == good and (good or s["reserved"] == [1, 0, 0])


def test_size_formula_against_the_library():
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(11)
    for _ in range(200):
        S, E, V = int(rng.integers(0, 1 << 28)), int(rng.integers(0, 1 << 33)), int(rng.choice([0, 8, 16]))
        assert hbs.mp4_protect_bytes(S, E, V) == P.growth(S, E, V) == 53 + (V + 3) * S + 6 * E == P.moof_size(S, E, V) - (88 + 16 * S)
    assert hbs.mp4_protect_bytes(0, 0, 0) == 53


# ---- the init segment -------------------------------------------------------------------------------------------------------------

def pssh_box(system, payload, version=0):
    return R.full(b"pssh", version, 0, system, struct.pack(">I", len(payload)), payload)


CASES = (dict(scheme=P.CENC, iv_size=8), dict(scheme=P.CENC, iv_size=16),
         dict(scheme=P.CBCS, iv_size=0, constant_iv=bytes(range(200, 216)), crypt_byte_block=1, skip_byte_block=9),
         dict(scheme=P.CBCS, iv_size=0, constant_iv=bytes(range(8))), dict(scheme=P.CBCS, iv_size=16, crypt_byte_block=5, skip_byte_block=5))


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("flags", (0, 1), ids=("hvc1", "hev1"))
def test_init_protect_against_the_reference(case, flags):
    import hevcbitstream_amd as hbs
    kw = CASES[case]
    init = hbs.mp4_init([VPS, SPS, PPS], track_id=5, width=640, height=360, flags=flags)
    assert init == R.init_segment([VPS, SPS, PPS], track_id=5, width=640, height=360, flags=flags)
    kid = bytes(range(16, 32))
    t = P.tenc_record(kid=kid, **kw)
    for boxes in ((), (pssh_box(bytes(range(16)), b"abc"),), (pssh_box(bytes(16), b""), pssh_box(bytes(range(16)), bytes(300), version=1))):
        want = P.init_protect(init, t, boxes)
        assert isinstance(want, bytes) and len(want) > len(init) + sum(len(x) for x in boxes)
        assert hbs.mp4_init_protect(init, kid, pssh=boxes, **kw) == want
        assert hbs.mp4_init_protect(init, kid, pssh=boxes, track_id=5, tenc=t) == want
    # what a reader sees: boxes that tile, encv with the old entry's bytes, the sinf's fields
    top = R.walk(want, 0, len(want))
    assert [k for k, _, _ in top] == [b"ftyp", b"moov"]
    tr = R.tree(want, top[1][1], top[1][2])
    assert len(tr[b"pssh"]) == 2 and [k for k, _, _ in R.walk(want, top[1][1], top[1][2])][-2:] == [b"pssh", b"pssh"]
    p, e = R.only(tr, b"stsd")
    (kind, sp, se), = R.walk(want, p + 8, e)
    assert kind == b"encv"
    kids = R.walk(want, sp + 78, se)
    assert [k for k, _, _ in kids] == [b"hvcC", b"sinf"]
    sinf = want[kids[1][1]:kids[1][2]]
    fourcc = b"hev1" if flags else b"hvc1"
    assert sinf[:12] == struct.pack(">I4s", 12, b"frma") + fourcc
    assert sinf[12:32] == struct.pack(">I4sI", 20, b"schm", 0) + struct.pack(">II", kw["scheme"], 0x00010000)
    assert sinf[36:40] == b"schi" and sinf[44:48] == b"tenc" and P.u32(sinf, 32) == len(sinf) - 32 and P.u32(sinf, 40) == len(sinf) - 40
    pattern = bool(kw.get("crypt_byte_block", 0) or kw.get("skip_byte_block", 0))
    assert sinf[48:56] == bytes([1 if pattern else 0, 0, 0, 0, 0, kw.get("crypt_byte_block", 0) << 4 | kw.get("skip_byte_block", 0), 1, kw["iv_size"]])
    assert sinf[56:72] == kid
    civ = kw.get("constant_iv", b"")
    assert sinf[72:] == (bytes([len(civ)]) + civ if kw["iv_size"] == 0 else b"")
    # the sample entry but for its size and name, and everything else, are the old bytes
    i0 = init.index(fourcc) - 4
    w0 = want.index(b"encv") - 4
    assert i0 == w0 and want[w0 + 8:kids[0][2]] == init[i0 + 8:i0 + P.u32(init, i0)]


def test_init_protect_refusals():
    import hevcbitstream_amd as hbs
    init = hbs.mp4_init([VPS, SPS, PPS])
    kid = bytes(16)
    good = P.tenc_record(kid=kid)
    assert hbs.mp4_init_protect(init, kid, tenc=good) == P.init_protect(init, good)

    def refused(seg=init, t=good, pssh=(), track_id=0):
        assert P.init_protect(seg, t, pssh, track_id) == P.E_ARG
        with pytest.raises(hbs.HbsError):
            hbs.mp4_init_protect(seg, kid, tenc=t, pssh=pssh, track_id=track_id)

    for cut in list(range(0, 40)) + list(range(len(init) - 40, len(init))):          # (every length: the sanitizer test)
        refused(seg=init[:cut])
    refused(track_id=2)
    moov = init.index(b"moov") - 4
    refused(seg=init[:moov] + struct.pack(">I", 0) + init[moov + 4:])                          # "to the end"
    refused(seg=init[:moov] + struct.pack(">I4sQ", 1, b"moov", len(init) - moov + 8) + init[moov + 8:])      # a 64-bit size
    stsd = init.index(b"stsd") - 4
    refused(seg=init[:stsd] + struct.pack(">I", P.u32(init, stsd) + 1) + init[stsd + 4:])        # a child that leaves its parent
    renamed = init.replace(b"hvc1", b"avc1")
    refused(seg=renamed)
    for kw in (dict(scheme=0x63656E73), dict(scheme=0), dict(iv_size=4), dict(iv_size=0), dict(iv_size=0, constant_iv=bytes(4)),
               dict(iv_size=8, constant_iv=bytes(8)), dict(crypt_byte_block=1, skip_byte_block=9), dict(scheme=P.CBCS, crypt_byte_block=16),
               dict(scheme=P.CBCS, skip_byte_block=16)):
        refused(t=P.tenc_record(kid=kid, **kw))
    r = good.copy()
    r["reserved"][0][5] = 1
    refused(t=r)
    box = pssh_box(bytes(16), b"xy")
    for bad in (box[:-1], box + b"\0", box.replace(b"pssh", b"psst"), box[:7]):
        refused(pssh=(bad,))
        refused(pssh=(box, bad))
    # protecting twice: the entry is no 'hvc1' any more
    refused(seg=hbs.mp4_init_protect(init, kid, tenc=good))
