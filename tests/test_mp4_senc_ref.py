"""tests/_mp4_senc_ref.py: on the output of the writer's reference (tests/_mp4_protect_ref.py) it returns the tables that went in
and agrees with that module's independent walker; hand-written fragments of other packagers' forms; every error class with the
lowest offender named; and the library's host function hbs_mp4_init_unprotect_host against the reference walk.  No GPU."""
import struct

import numpy as np
import pytest

from tests import _mp4_protect_ref as P
from tests import _mp4_read_ref as RR
from tests import _mp4_ref as R
from tests import _mp4_senc_ref as S
from tests.test_mp4_protect_ref import CASES, PPS, SPS, VPS, pssh_box, random_input

IV = bytes(range(1, 17))


def per_sample(first, sub, iv, V):
    return [(bytes(iv[16 * s:16 * s + V]) + bytes(16 - V) if V else bytes(16),
             [(int(c), int(p)) for c, p in sub[int(first[s]):int(first[s + 1])]]) for s in range(len(first) - 1)]


# ---- the writer's output ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", (0, 8, 16))
def test_the_tables_that_went_into_protect_come_back(V):
    rng = np.random.default_rng(300 + V)
    data, frags, first, sub, iv, per = random_input(rng, 9, V)
    out, so, ss, fr, s = P.protect(data, frags, first, sub, iv, V)
    assert s["error"] == 0
    got_first, got_sub, got_iv, gs = S.senc_samples(out, fr, ss, V)
    assert np.array_equal(got_first, first) and np.array_equal(got_sub, sub)
    assert np.array_equal(got_iv, iv if V else np.zeros(16 * len(per), np.uint8))
    assert gs == S.summary(0, len(sub), len(per), int(sub["protect"].sum()), len(out), senc_read=len(fr))
    # plan only and a sub_cap one short
    assert S.senc_samples(out, fr, None, V, sub_cap=len(sub))[3] == gs
    assert S.senc_samples(out, fr, None, V, sub_cap=len(sub) - 1)[3] == dict(gs, error=S.E_CAPACITY)
    # the independent walker of the writer's module sees the same samples
    walked = [x for g in P.walk_protected(out, V) for x in g["samples"]]
    mine = per_sample(got_first, got_sub, got_iv, V)
    assert [(bytes(i) + bytes(16 - V) if V else bytes(16), [tuple(map(int, e)) for e in ent]) for i, ent in walked] == mine


# ---- other packagers' forms ----------------------------------------------------------------------------------------------------------

def foreign(V=8):
    """-> (bytes, FRAG table, sizes, the samples [(iv16, entries)] in order, fragments with a senc): hand-written fragments"""
    iv = lambda k: bytes((k + j) % 251 + 1 for j in range(V)) + bytes(16 - V)          # noqa: E731
    a = [(iv(1), [(5, 20)]), (iv(2), [(3, 0), (0, 7)]), (iv(3), [])]
    b = [(iv(4), [(9, 1)] * 3)]
    c = [(iv(5), [(1, 2)]), (iv(6), [(65535, 0), (4, 4)])]
    d = [(iv(7), [(7, 70)]), (iv(8), [(8, 80)])]
    e = [(iv(9), [(0, 11)]), (iv(10), []), (iv(11), [(0, 13)])]           # a senc without flag 2
    f = [(iv(12), [(2, 3)])]
    size = lambda x: [sum(p + q for p, q in ent) for _, ent in x]          # noqa: E731
    blobs = [
        # the senc in front of the trun, no saiz
        S.fragment([S.traf(1, size(a), front=(S.senc_box(V, a),))]),
        # a uuid and a free between the children, a saiz with aux_info_type
        S.fragment([S.traf(1, size(b), RR.box(b"uuid", bytes(20)), S.saiz_box(V, b, typed=True), RR.box(b"free", b"xy"), S.senc_box(V, b))]),
        # a 64-bit traf size, a saiz of a default size that is wrong for sample 1
        S.fragment([S.traf(1, size(c), S.saiz_box(V, c, default=V + 8), S.senc_box(V, c), large=True)]),
        # two trafs, the second chosen by track_id; the first has a senc of its own
        S.fragment([S.traf(2, [1], S.senc_box(V, [(iv(99), [(1, 0)])])), S.traf(1, size(d), S.saiz_box(V, d), S.senc_box(V, d))]),
        # a senc without flag 2
        S.fragment([S.traf(1, [11, 0, 13], S.senc_box(V, e, flags=0))]),
        # trailing bytes in the senc, a second senc that is not read
        S.fragment([S.traf(1, size(f), S.senc_box(V, f, trailing=b"\x00\x09abcdefg"), S.senc_box(V, [(iv(50), [(1, 1)])]))]),
    ]
    groups = [a, b, c, d, e, f]
    data, fr = S.frag_table(blobs, [len(g) for g in groups], gap=3)
    sizes = size(a) + size(b) + size(c) + size(d) + [11, 0, 13] + size(f)
    return data, fr, sizes, [x for g in groups for x in g], len(groups)


@pytest.mark.parametrize("V", (0, 8, 16))
def test_foreign_fragments(V):
    data, fr, sizes, want, read = foreign(V)
    first, sub, iv, s = S.senc_samples(data, fr, sizes, V, track_id=1)
    assert s["error"] == 0 and s["reserved"] == [0, 0, read]
    assert per_sample(first, sub, iv, V) == [(i if V else bytes(16), e) for i, e in want]
    assert s["nal_count"] == sum(len(e) for _, e in want) and s["rbsp_bytes"] == sum(q for _, e in want for _, q in e)
    # without sizes only the fragment without flag 2 offends
    assert S.senc_samples(data, fr, None, V, track_id=1)[3]["reserved"] == [0, 5, 0]
    # track_id 0 takes the first traf: fragment 3's has one sample, not two
    assert S.senc_samples(data, fr, sizes, V)[3]["reserved"] == [0, 4, 0]


def test_clear_if_absent():
    sizes = [0, 1, 65535, 65536, 200000]
    data, fr = S.frag_table([S.fragment([S.traf(1, sizes[:2])]), S.fragment([S.traf(1, sizes[2:], RR.box(b"saio", bytes(12)))])], [2, 3])
    first, sub, iv, s = S.senc_samples(data, fr, sizes, 8, flags=S.CLEAR_IF_ABSENT)
    assert first.tolist() == [0, 0, 1, 2, 4, 8] and not iv.any() and s["reserved"] == [0, 0, 0] and s["rbsp_bytes"] == 0
    assert [tuple(x) for x in sub.tolist()] == [(1, 0), (65535, 0), (65535, 0), (1, 0), (65535, 0), (65535, 0), (65535, 0), (200000 - 3 * 65535, 0)]
    assert S.senc_samples(data, fr, sizes, 8)[3]["reserved"] == [0, 1, 0]
    assert S.senc_samples(data, fr, None, 8, flags=S.CLEAR_IF_ABSENT)[3]["reserved"] == [0, 1, 0]
    sizes[3] = 1 << 32
    assert S.senc_samples(data, fr, sizes, 8, flags=S.CLEAR_IF_ABSENT)[3] == S.summary(S.E_ARG, 0, 5, 0, len(data), bad_sample=4)


# ---- errors -----------------------------------------------------------------------------------------------------------------------

def error_cases(V=8):
    """-> [(name, bytes, FRAG table, sizes, kwargs, reserved)]: three good fragments of two samples with one thing wrong in
    fragment 1 (and, where named, fragment 2), so that the lowest offender is never fragment 0"""
    iv = bytes(range(1, 17))
    smp = [(iv, [(5, 20)]), (iv, [(3, 0), (0, 7)])]
    sizes = [25, 10]
    good = S.fragment([S.traf(1, sizes, S.saiz_box(V, smp), S.senc_box(V, smp))])
    cases = []

    def case(name, middle, reserved, third=None, sizes3=None, no_sizes=False, **kw):
        data, fr = S.frag_table([good, middle, good if third is None else third], [2, 2, 2], gap=5)
        cases.append((name, data, fr, None if no_sizes else (sizes * 3 if sizes3 is None else sizes3), kw, reserved))

    t = lambda *extra, **kw: S.fragment([S.traf(1, sizes, *extra, **kw)])          # noqa: E731
    # sample 1 says two entries, and the box ends behind the first
    walk_bad = t(RR.full(b"senc", 0, 2, struct.pack(">I", 2) + iv[:V] + struct.pack(">HHI", 1, 5, 20) + iv[:V] + struct.pack(">HHI", 2, 3, 0)))
    case("not a moof", RR.box(b"moov", good[8:len(good) - 8]) + RR.box(b"mdat"), [0, 2, 0])
    case("a child breaks the box rule", S.fragment([S.traf(1, sizes, S.senc_box(V, smp)) + struct.pack(">I4s", 4, b"free")]), [0, 2, 0])
    case("no tfhd", S.fragment([RR.box(b"traf", RR.tfdt(0) + S.senc_box(V, smp))]), [0, 2, 0])
    case("no traf of the track", S.fragment([S.traf(9, sizes, S.senc_box(V, smp))]), [0, 2, 0], track_id=1)
    case("senc version 1", t(S.senc_box(V, smp, version=1)), [0, 2, 0])
    case("senc flags 4", t(S.senc_box(V, smp, flags=6)), [0, 2, 0])
    case("sample_count", t(S.senc_box(V, smp, count=3)), [0, 2, 0])
    case("a sample leaves the box", walk_bad, [0, 2, 0])
    case("no senc", t(), [0, 2, 0])
    case("no sizes for a senc without flag 2", t(S.senc_box(V, smp, flags=0)), [0, 2, 0], no_sizes=True)
    case("two classes: the lower fragment wins", walk_bad, [0, 2, 0], third=t(S.senc_box(V, smp, version=1)))
    case("a form error below a walk error", t(S.senc_box(V, smp, version=1)), [0, 2, 0], third=walk_bad)
    case("a fragment error wins over a sample error", t(S.senc_box(V, smp, flags=0)), [0, 3, 0], third=t(), sizes3=[25, 10, 1 << 32, 10, 25, 10])
    case("a sample error", t(S.senc_box(V, smp, flags=0)), [4, 0, 0], sizes3=[25, 10, 25, 1 << 33, 1 << 32, 10])
    # numbering
    data, fr = S.frag_table([good, good, good], [2, 2, 2])
    fr["first_au"][2] += 1
    cases.append(("numbering", data, fr.copy(), sizes * 3, {}, [0, 3, 0]))
    fr["first_au"][2] -= 1
    cases.append(("the last sum is not n_samples", data, fr.copy(), sizes * 3 + [1], dict(n_samples=7), [0, 3, 0]))
    fr["out_bytes"][1] = len(data)
    cases.append(("leaves the buffer", data, fr.copy(), sizes * 3, {}, [0, 2, 0]))
    fr["out_bytes"][1] = 40
    cases.append(("the moof is larger than out_bytes", data, fr.copy(), sizes * 3, {}, [0, 2, 0]))
    return cases


@pytest.mark.parametrize("i", range(len(error_cases())), ids=[c[0].replace(" ", "_") for c in error_cases()])
def test_every_error_class_names_the_lowest_offender(i):
    name, data, fr, sizes, kw, reserved = error_cases()[i]
    n = kw.get("n_samples", int(fr["samples"].sum()))
    first, sub, iv, s = S.senc_samples(data, fr, sizes, 8, **kw)
    assert first is None and sub is None and iv is None
    assert s == S.summary(S.E_ARG, 0, n, 0, len(data), bad_sample=reserved[0], bad_frag=reserved[1]), name


def test_empty_calls():
    assert S.senc_samples(b"", np.zeros(0, R.FRAG), None, 8)[3] == S.summary()
    fr = np.zeros(2, dtype=R.FRAG)
    fr["out_off"], fr["out_bytes"] = [0, 8], [8, 3]
    first, sub, iv, s = S.senc_samples(b"x" * 11, fr, None, 8)
    assert first.tolist() == [0] and len(sub) == 0 and s == S.summary(in_bytes=11)
    fr["out_bytes"][1] = 4
    assert S.senc_samples(b"x" * 11, fr, None, 8)[3]["reserved"] == [0, 2, 0]


# ---- the init segment -------------------------------------------------------------------------------------------------------------

def unprotect(seg, track_id=0):
    """the library's answer in the reference's form"""
    import hevcbitstream_amd as hbs
    try:
        out, tenc, fmt, pssh = hbs.mp4_init_unprotect(seg, track_id)
    except hbs.HbsError:
        return S.E_ARG
    raw = bytes(seg)
    return out, tenc, fmt, [(raw.index(x) if raw.count(x) == 1 else None, len(x)) for x in pssh]


def same(got, want):
    if want == S.E_ARG or got == S.E_ARG:
        return got == want
    return got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2] == want[2] and [z for _, z in got[3]] == [z for _, z in want[3]] \
        and all(a is None or a == b for (a, _), (b, _) in zip(got[3], want[3]))


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("flags", (0, 1), ids=("hvc1", "hev1"))
def test_init_round_trip(case, flags):
    kw = CASES[case]
    init = R.init_segment([VPS, SPS, PPS], track_id=5, width=640, height=360, flags=flags)
    kid = bytes(range(16, 32))
    t = P.tenc_record(kid=kid, **kw)
    for boxes in ((), (pssh_box(bytes(range(16)), b"abc"),), (pssh_box(bytes(16), b""), pssh_box(bytes(range(16)), bytes(300), version=1))):
        prot = P.init_protect(init, t, boxes)
        want = S.init_unprotect(prot)
        assert want != S.E_ARG and want[0] == init and want[1].tobytes() == t.tobytes() and want[2] == struct.unpack(">I", b"hev1" if flags else b"hvc1")[0]
        assert [prot[a:a + z] for a, z in want[3]] == list(boxes)
        for tid in (0, 5):
            assert same(unprotect(prot, tid), S.init_unprotect(prot, tid))
        assert unprotect(prot, 6) == S.E_ARG == S.init_unprotect(prot, 6)
        assert RR.init_read(want[0])[0]["entry"] == want[2]
    assert unprotect(init) == S.E_ARG == S.init_unprotect(init)


def test_init_truncated_at_every_length_and_every_size_byte_flipped():
    init = R.init_segment([VPS, SPS, PPS], track_id=5, width=640, height=360)
    t = P.tenc_record(kid=bytes(range(16)), scheme=P.CBCS, iv_size=0, constant_iv=bytes(range(8)), crypt_byte_block=1, skip_byte_block=9)
    prot = P.init_protect(init, t, (pssh_box(bytes(range(16)), b"abc"),))
    for n in range(len(prot)):
        assert same(unprotect(prot[:n]), S.init_unprotect(prot[:n])), n
    # every byte of every box's size field, found by walking the tree
    def size_fields(lo, hi, depth=0):
        for kind, at, pay, end in RR.boxes(prot, lo, hi):
            yield from range(at, at + 4)
            if kind in (b"moov", b"trak", b"mdia", b"minf", b"stbl", b"sinf", b"schi", b"mvex", b"dinf"):
                yield from size_fields(pay, end, depth + 1)
            elif kind == b"stsd":
                yield from size_fields(pay + 8, end, depth + 1)
            elif kind == b"encv":
                yield from size_fields(pay + 78, end, depth + 1)
    fields = sorted(set(size_fields(0, len(prot))))
    assert len(fields) >= 4 * 20
    answers = set()
    for at in fields:
        for bit in (0x01, 0x10, 0x80):
            x = bytearray(prot)
            x[at] ^= bit
            got, want = unprotect(bytes(x)), S.init_unprotect(bytes(x))
            assert same(got, want), (at, bit)
            answers.add(want == S.E_ARG)
    assert answers == {True, False}
