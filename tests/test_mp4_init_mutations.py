"""The five host calls that walk an MP4's moov to one track's sample entry -- hbs_mp4_init_read_host, hbs_mp4_track_read_host,
hbs_mp4_stbl_find_host, hbs_mp4_init_protect_host, hbs_mp4_init_unprotect_host -- through the built library, against their
Python references (tests/_mp4_read_ref.py, _mp4_stbl_ref.py, _mp4_protect_ref.py, _mp4_senc_ref.py) on mutated inputs: a
single-track init segment, a progressive file, a protected init segment and six two-track init segments, each truncated at
every length and with every header byte of every box of its tree altered.  Library and reference must agree on every input:
on whether it is accepted, and then on the return value and every byte and field that comes back.  No GPU."""
import functools
import struct

import pytest

from tests import _mp4_protect_ref as P
from tests import _mp4_read_ref as RR
from tests import _mp4_ref as R
from tests import _mp4_senc_ref as S
from tests import _mp4_stbl_ref as T
from tests.test_mp4_protect_ref import PPS, SPS, VPS, pssh_box
from tests.test_mp4_senc_ref import same, unprotect

REFUSED = "refused"
TENC = P.tenc_record(kid=bytes(range(16)), scheme=P.CBCS, iv_size=0, constant_iv=bytes(range(8)), crypt_byte_block=1, skip_byte_block=9)
PSSH = (pssh_box(bytes(range(16)), b"abc"),)


# ---- the base inputs --------------------------------------------------------------------------------------------------------------

def tree(b, lo=0, hi=None, path=()):
    """every box of the tree that the calls walk: [(path of types, box begin, payload begin, end)]"""
    out = []
    for kind, at, pay, end in RR.boxes(b, lo, len(b) if hi is None else hi):
        out.append((path + (kind,), at, pay, end))
        if kind in (b"moov", b"trak", b"mdia", b"minf", b"stbl", b"dinf", b"mvex", b"sinf", b"schi"):
            out += tree(b, pay, end, path + (kind,))
        elif kind == b"stsd":
            out += tree(b, pay + 8, end, path + (kind,))
        elif path[-1:] == (b"stsd",) and end - pay >= 78:         # a visual sample entry: its boxes lie behind 78 bytes
            out += tree(b, pay + 78, end, path + (kind,))
    return out


def box_of(b, *path):
    return next(x for x in tree(b) if x[0] == path)


@functools.lru_cache(maxsize=None)
def init_segment():
    seg = bytes(R.init_segment([VPS, SPS, PPS], track_id=5, width=640, height=360))
    assert len(seg) == 689
    return seg


@functools.lru_cache(maxsize=None)
def progressive():
    data, _ = T.progressive_file([bytes([i] * 5) for i in range(4)], [2, 2], [100] * 4, nals=[VPS, SPS, PPS], track_id=5)
    assert len(data) == 721
    return bytes(data)


@functools.lru_cache(maxsize=None)
def protected():
    prot = P.init_protect(init_segment(), TENC, PSSH)
    assert prot != P.E_ARG
    return bytes(prot)


@functools.lru_cache(maxsize=None)
def two_tracks(kind, front):
    """the init segment with a copy of its trak, as track 9, in front of the trak or behind it; the copy's sample entry renamed
    'mp4a' (kind "mp4a"), its minf renamed 'free' (kind "free"), or as it is (kind "same")"""
    seg = init_segment()
    _, moov_at, _, _ = box_of(seg, b"moov")
    _, trak_at, _, trak_end = box_of(seg, b"moov", b"trak")
    copy = bytearray(seg)
    _, _, tkhd, _ = box_of(seg, b"moov", b"trak", b"tkhd")
    assert copy[tkhd] == 0 and struct.unpack(">I", copy[tkhd + 12:tkhd + 16])[0] == 5
    copy[tkhd + 12:tkhd + 16] = struct.pack(">I", 9)
    if kind == "mp4a":
        _, at, _, _ = box_of(seg, b"moov", b"trak", b"mdia", b"minf", b"stbl", b"stsd", b"hvc1")
        copy[at + 4:at + 8] = b"mp4a"
    elif kind == "free":
        _, at, _, _ = box_of(seg, b"moov", b"trak", b"mdia", b"minf")
        copy[at + 4:at + 8] = b"free"
    copy = bytes(copy[trak_at:trak_end])
    where = trak_at if front else trak_end
    out = bytearray(seg[:where] + copy + seg[where:])
    out[moov_at:moov_at + 4] = struct.pack(">I", struct.unpack(">I", seg[moov_at:moov_at + 4])[0] + len(copy))
    return bytes(out)


BASES = {"init": init_segment, "progressive": progressive, "protected": protected}
for _kind in ("mp4a", "free", "same"):
    for _front in (True, False):
        BASES["%s-%s" % (_kind, "front" if _front else "behind")] = functools.partial(two_tracks, _kind, _front)
CASES = [(name, 0) for name in ("init", "progressive", "protected")] + [(name, tid) for name in BASES if "-" in name for tid in (0, 5, 9)]


@functools.lru_cache(maxsize=None)
def mutations(name):
    """the base input, then its truncation at every length, then every one of the 8 header bytes of every box of its tree
    XORed with 0x01, 0x10 and 0x80"""
    b = BASES[name]()
    out = [b] + [b[:n] for n in range(len(b))]
    for _, at, _, _ in tree(b):
        for i in range(at, at + 8):
            for bit in (0x01, 0x10, 0x80):
                out.append(b[:i] + bytes([b[i] ^ bit]) + b[i + 1:])
    return out


# ---- the five calls: (the library's answer, the reference's) in one form, REFUSED for what is refused --------------------------------

def track_answer(read, b, tid):
    import hevcbitstream_amd as hbs
    try:
        t, nals = read(b, tid)
    except hbs.HbsError:
        return REFUSED
    assert t["reserved"].tolist() == [0, 0]
    return {k: int(t[k]) for k in t.dtype.names if k != "reserved"}, nals


def track_want(read, b, tid):
    try:
        t, where = read(b, tid)
    except RR.Malformed:
        return REFUSED
    return t, [b[o:o + n] for o, n in where]


def call_init_read(b, tid):
    import hevcbitstream_amd as hbs
    return track_answer(hbs.mp4_init_read, b, tid), track_want(RR.init_read, b, tid)


def call_track_read(b, tid):
    import hevcbitstream_amd as hbs
    return track_answer(hbs.mp4_track_read, b, tid), track_want(T.track_read, b, tid)


def call_stbl_find(b, tid):
    import hevcbitstream_amd as hbs
    try:
        got = hbs.mp4_stbl_find(b, 16, tid).tobytes()
    except hbs.HbsError:
        got = REFUSED
    try:
        want = T.find(b, 16, tid).tobytes()
    except RR.Malformed:
        want = REFUSED
    return got, want


def call_init_protect(b, tid):
    import hevcbitstream_amd as hbs
    try:
        got = hbs.mp4_init_protect(b, None, tenc=TENC, pssh=PSSH, track_id=tid)
    except hbs.HbsError:
        got = REFUSED
    want = P.init_protect(b, TENC, PSSH, tid)
    return got, REFUSED if want == P.E_ARG else want


class Unprotected:
    """hbs_mp4_init_unprotect_host's answer -- the clear segment, the tenc, the format, the pssh list -- compared as
    tests/test_mp4_senc_ref.py compares it"""
    def __init__(self, x):
        self.x = x

    def __eq__(self, other):
        return isinstance(other, Unprotected) and same(self.x, other.x)


def call_init_unprotect(b, tid):
    got, want = unprotect(b, tid), S.init_unprotect(b, tid)
    return REFUSED if got == S.E_ARG else Unprotected(got), REFUSED if want == S.E_ARG else Unprotected(want)


CALLS = {"init_read": call_init_read, "track_read": call_track_read, "stbl_find": call_stbl_find, "init_protect": call_init_protect,
         "init_unprotect": call_init_unprotect}


@pytest.mark.parametrize("base,tid", CASES, ids=["%s-track%d" % c for c in CASES])
@pytest.mark.parametrize("call", list(CALLS))
def test_library_and_reference_agree_on_every_mutation(call, base, tid):
    todo = mutations(base)
    assert len(todo) > 1200
    accepted = []
    for i, b in enumerate(todo):
        got, want = CALLS[call](b, tid)
        assert (got == REFUSED) == (want == REFUSED) and got == want, (i, len(b))
        accepted.append(want != REFUSED)
    # where the base input (todo[0]) is accepted, its mutations are of both kinds: the test cannot pass by refusing everything
    if accepted[0]:
        assert 0 < sum(accepted[1:]) < len(todo) - 1


def test_the_base_inputs_are_what_the_cases_assume():
    """which call accepts which unmutated input: every call has a base input that it accepts, every two-track variant one"""
    ok = {(call, base, tid) for base, tid in CASES for call in CALLS if CALLS[call](BASES[base](), tid)[1] != REFUSED}
    assert {c for c, _, _ in ok} == set(CALLS)
    assert ("init_read", "init", 0) in ok and ("init_protect", "init", 0) in ok and ("init_unprotect", "protected", 0) in ok
    assert ("track_read", "progressive", 0) in ok and ("stbl_find", "progressive", 0) in ok and ("init_read", "progressive", 0) not in ok
    for kind in ("mp4a", "free", "same"):
        for where in ("front", "behind"):
            assert ("init_read", "%s-%s" % (kind, where), 5) in ok
    # the copy is read as track 9 only where it is a video track with an hvcC (and it has no trex: only the track reader takes it)
    assert ("track_read", "same-front", 9) in ok and ("track_read", "mp4a-front", 9) not in ok and ("init_read", "same-front", 9) not in ok


def with_broken_box_at_the_end_of(b, *path):
    """b with 8 bytes that are no box (a size field of 0x7FFFFFFF) appended to the children of the LAST box with that path; the
    sizes of that box and of the boxes that hold it grow by 8"""
    hit = [x for x in tree(b) if x[0] == path][-1]
    out = bytearray(b[:hit[3]] + struct.pack(">I", 0x7FFFFFFF) + b"free" + b[hit[3]:])
    for p, at, _, end in tree(b):
        if p == path[:len(p)] and at <= hit[1] and hit[3] <= end:
            out[at:at + 4] = struct.pack(">I", end - at + 8)
    return bytes(out)


def test_unprotect_looks_at_nothing_behind_the_four_boxes_of_its_descent():
    """hbs_mp4_init_unprotect_host takes mdia, minf, stbl and stsd of a candidate trak each as the first of its type and looks
    at nothing behind it; the reader then judges the rebuilt segment.  Where a clear trak with the SAME track id lies in front,
    the reader stops at that one, so a broken box behind the protected trak's minf or stsd goes unseen and the segment is
    accepted, as tests/_mp4_senc_ref.py states it.  (Behind the mdia it is seen: the tkhd is looked for in the whole trak.)"""
    prot = protected()
    _, trak_at, _, _ = box_of(prot, b"moov", b"trak")
    _, moov_at, _, _ = box_of(prot, b"moov")
    clear = init_segment()
    _, c_at, _, c_end = box_of(clear, b"moov", b"trak")
    twin = bytearray(prot[:trak_at] + clear[c_at:c_end] + prot[trak_at:])
    twin[moov_at:moov_at + 4] = struct.pack(">I", struct.unpack(">I", prot[moov_at:moov_at + 4])[0] + c_end - c_at)
    twin = bytes(twin)
    trak = (b"moov", b"trak")
    accepted = {}
    for name, path in (("none", None), ("stsd", trak + (b"mdia", b"minf", b"stbl")), ("minf", trak + (b"mdia",)), ("mdia", trak)):
        b = twin if path is None else with_broken_box_at_the_end_of(twin, *path)
        assert len(b) == len(twin) + (0 if path is None else 8)
        for tid in (0, 5):
            got, want = call_init_unprotect(b, tid)
            assert (got == REFUSED) == (want == REFUSED) and got == want, (name, tid)
            accepted[name, tid] = want != REFUSED
    assert accepted == {(name, tid): name != "mdia" for name in ("none", "stsd", "minf", "mdia") for tid in (0, 5)}


def test_stsd_entry_walk_looks_at_nothing_behind_the_entries_it_counts():
    """The first trak's one stsd entry is an 'mp4a' whose size field is shrunk to 40: it is well-formed, it is not HEVC, and
    entry_count (1) ends the walk there, so the bytes behind it -- which are no boxes -- are never looked at and the second trak
    is read.  The library has always accepted this and include/hevcbitstream_amd.h says so; the references tile no further than
    the library walks.  Refusing such a segment would be a separate, behavioural change, not part of any refactoring."""
    import hevcbitstream_amd as hbs
    base = two_tracks("mp4a", True)
    _, at, _, end = box_of(base, b"moov", b"trak", b"mdia", b"minf", b"stbl", b"stsd", b"mp4a")
    assert end - at > 40
    seg = base[:at] + struct.pack(">I", 40) + base[at + 4:]
    with pytest.raises(RR.Malformed):
        RR.boxes(seg, at, end)                                    # (what lies behind the 40 bytes tiles nothing)
    for tid in (0, 5):
        want = track_want(RR.init_read, base, tid)
        assert want != REFUSED and want[0]["track_id"] == 5
        assert track_want(RR.init_read, seg, tid) == want
        assert track_answer(hbs.mp4_init_read, seg, tid) == want
        assert track_answer(hbs.mp4_track_read, seg, tid) == track_want(T.track_read, seg, tid) == track_want(T.track_read, base, tid)
        assert hbs.mp4_stbl_find(seg, 0, tid).tobytes() == T.find(seg, 0, tid).tobytes() == T.find(base, 0, tid).tobytes()
        assert hbs.mp4_init_protect(seg, None, tenc=TENC, pssh=PSSH, track_id=tid) == P.init_protect(seg, TENC, PSSH, tid) != P.E_ARG
