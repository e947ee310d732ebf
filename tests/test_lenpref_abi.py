"""hbs_annexb_to_lenpref / hbs_lenpref_to_annexb on the CPU side: the symbols, and the plain-loop reference of their semantics
(tests/_lenpref_ref.py) against the oracle's find_nal_unit walk: Annex-B -> records -> Annex-B, scanned again, gives the kept
payloads."""
import numpy as np
import pytest

from tests import _filter_ref as F
from tests import _lenpref_ref as R


def test_symbols_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    for name in ("hbs_annexb_to_lenpref", "hbs_lenpref_to_annexb"):
        assert name in declared_functions()
        assert name in EXPORTS
        assert hasattr(hbs.load_library(), name)
    assert hasattr(hbs.Context, "annexb_to_lenpref") and hasattr(hbs.Context, "lenpref_to_annexb")
    assert hasattr(hbs.Context, "annexb_to_lenpref_async") and hasattr(hbs.Context, "lenpref_to_annexb_async")


def _entries(spans):
    idx = np.zeros(len(spans), dtype=F.NAL_ENTRY)
    for k, (a, b) in enumerate(spans):
        idx["start"][k], idx["end"][k] = a, b
    return idx


def _round_trip(orc, s, idx, keep, L, sc):
    """-> 1 if the stated exception occurred, 0 if not, -1 if a kept NAL does not fit the length field"""
    pay = [s[int(e["start"]):int(e["end"])] for e in idx[keep]]
    out, io, _, summ = R.to_lenpref_ref(s, idx, keep, L)
    if any(len(p) > (1 << (8 * L)) - 1 for p in pay):
        assert summ["error"] == R.E_ARG and len(out) == 0
        return -1
    assert summ["error"] == 0 and summ["nal_count"] == len(pay) and summ["stream_bytes"] == len(out) == sum(L + len(p) for p in pay)
    assert all(np.array_equal(out[int(e["start"]):int(e["end"])], p) for e, p in zip(io, pay))
    back, so, bs = R.to_annexb_ref(out, [0], [len(out)], L, sc)
    assert bs["error"] == 0 and bs["nal_count"] == len(pay) and list(so) == [0, len(back)] and len(back) == sum(sc + len(p) for p in pay)
    got, _ = orc.index_stream(back)
    found = [back[int(e["start"]):int(e["end"])] for e in got]
    # a found payload never ends in 00 unless it is the stream's last
    assert all(len(p) and p[-1] != 0 for p in pay[:-1])
    if R.rescan_misses_last(back, pay, sc):
        want = pay[:-2] + [np.concatenate([pay[-2], np.frombuffer(R.SC[3], np.uint8)])]     # one NAL exempt: the one in front is cut late
        assert len(found) == len(want) and all(np.array_equal(a, b) for a, b in zip(found, want))
        return 1
    assert len(found) == len(pay) and all(np.array_equal(a, b) for a, b in zip(found, pay))
    return 0


def test_round_trip_is_found_again_by_the_walk(orc):
    """300 streams, each with keep-all, with a random mask and with a random L / start code (keep-all): 900 cases.  In each
    the predicate and the walk agree, in both directions (_round_trip).  The exception needs a kept empty NAL behind another
    kept NAL: the walk yields one from a stream that ends in 00 00 00 01 behind a NAL (the three zeros end the NAL in front, the
    code is found, nothing follows), random_stream draws such ends, and written back behind a 3-byte code it is missed."""
    rng = np.random.default_rng(7)
    cases = misses = too_long = 0
    for it in range(300):
        size = int(rng.choice([1, 5, 40, 300, 3000, 20000]))
        mean = int(rng.choice([2, 8, 60, 500, 4000]))
        s = F.random_stream(rng, size, mean)
        idx, _, _ = orc.index_extract(s)
        for mode in range(3):
            keep = rng.random(len(idx)) < rng.random() if mode == 1 else np.ones(len(idx), dtype=bool)
            L, sc = (4, 4) if mode < 2 else (int(rng.choice([1, 2, 4])), int(rng.choice([3, 4])))
            r = _round_trip(orc, s, idx, keep, L, sc)
            misses += r == 1
            too_long += r == -1
            cases += 1
    assert cases == 900
    assert misses >= 1        # the exception occurs in these streams, and _round_trip saw it exactly as stated
    assert too_long >= 1      # a NAL longer than a 1-byte length field holds occurs too, and is refused


def test_a_walk_finds_an_empty_last_nal_behind_another(orc):
    """00 00 01 40 01 11 | 00 00 00 01: indexed as (3, 6), (10, 10).  As records and back with 3-byte codes the walk finds one
    NAL, three bytes longer; with 4-byte codes it finds both again."""
    s = np.frombuffer(b"\x00\x00\x01\x40\x01\x11\x00\x00\x00\x01", dtype=np.uint8).copy()
    idx, _ = orc.index_stream(s)
    assert [(int(e["start"]), int(e["end"])) for e in idx] == [(3, 6), (10, 10)]
    assert _round_trip(orc, s, idx, np.ones(2, bool), 4, 3) == 1
    assert _round_trip(orc, s, idx, np.ones(2, bool), 4, 4) == 0
    assert _round_trip(orc, s, idx, np.array([False, True]), 4, 3) == 0        # alone it is found


def test_a_found_payload_does_not_end_in_zero_unless_it_is_the_last(orc):
    """00 00 01 41 00 | 00 00 01 42 00: the walk gives `41` (the zero belongs to the 4-byte start code behind it) and, at the
    stream's end, `42 00`.  So the start code written in front of the next NAL cannot shorten a payload."""
    s = np.frombuffer(b"\x00\x00\x01\x41\x00\x00\x00\x01\x42\x00", dtype=np.uint8).copy()
    idx, _ = orc.index_stream(s)
    assert [bytes(s[int(e["start"]):int(e["end"])]) for e in idx] == [b"\x41", b"\x42\x00"]
    for sc in (3, 4):
        assert _round_trip(orc, s, idx, np.ones(2, bool), 1, sc) == 0
    # a hand-made record that does end in 00 is cut by one byte in front of the next start code: not what a walk finds
    back, _, _ = R.to_annexb_ref(np.frombuffer(b"\x02\x41\x00\x01\x42", np.uint8), [0], [5], 1, 4)
    got, _ = orc.index_stream(back)
    assert [bytes(back[int(e["start"]):int(e["end"])]) for e in got] == [b"\x41", b"\x42"]


@pytest.mark.parametrize("last,sc,missed", [(b"", 3, True), (b"", 4, False), (b"\x40", 3, False), (b"\x40", 4, False)])
def test_the_stated_exception(orc, last, sc, missed):
    pay = [b"\x40\x01\x11", last]
    rec = b"".join(len(p).to_bytes(2, "big") + p for p in pay)
    back, _, summ = R.to_annexb_ref(np.frombuffer(rec, np.uint8), [0], [len(rec)], 2, sc)
    assert summ["nal_count"] == 2
    assert R.rescan_misses_last(back, pay, sc) == missed
    got, _ = orc.index_stream(back)
    found = [bytes(back[int(e["start"]):int(e["end"])]) for e in got]
    assert found == ([pay[0] + b"\x00\x00\x01"] if missed else pay)
    # alone, a bare start code is found as an empty last NAL
    back, _, _ = R.to_annexb_ref(np.frombuffer(b"\x00\x00", np.uint8), [0], [2], 2, sc)
    got, why = orc.index_stream(back)
    assert len(got) == 1 and int(got["start"][0]) == int(got["end"][0]) == sc and not R.rescan_misses_last(back, [b""], sc)


def test_sample_table_with_aus_where_nothing_is_kept():
    s = np.arange(1, 101, dtype=np.uint8)
    idx = _entries([(3, 10), (13, 20), (24, 24), (27, 40), (43, 50), (60, 100)])
    idx["rbsp_len"] = [7, 7, 0, 13, 6, 40]
    idx["status"] = [0, 1, 0, 2, 0, 4]
    nal_au = np.array([0, 0, 1, 2, 2, 3], dtype=np.uint32)
    keep = np.array([1, 0, 0, 0, 7, 1], dtype=np.uint8)
    out, io, so, summ = R.to_lenpref_ref(s, idx, keep, 2, nal_au, 4)
    assert bytes(out) == b"\x00\x07" + bytes(s[3:10]) + b"\x00\x07" + bytes(s[43:50]) + b"\x00\x28" + bytes(s[60:100])
    assert list(so) == [0, 9, 9, 18, 60]                    # AU 1 is an empty sample
    assert list(io["start"]) == [2, 11, 20] and list(io["end"]) == [9, 18, 60]
    assert list(io["rbsp_off"]) == [0, 7, 13] and list(io["rbsp_len"]) == [7, 6, 40] and list(io["status"]) == [0, 0, 0]
    assert summ == dict(nal_count=3, nal_found=6, rbsp_bytes=53, stream_bytes=60, stop_reason=0, error=0)
    # an empty kept NAL is a record of L zero bytes; nothing kept at all: every sample empty
    out, io, so, _ = R.to_lenpref_ref(s, idx, [0, 0, 1, 0, 0, 0], 4, nal_au, 4)
    assert bytes(out) == b"\x00\x00\x00\x00" and list(so) == [0, 0, 4, 4, 4] and (int(io["start"][0]), int(io["end"][0])) == (4, 4)
    out, io, so, summ = R.to_lenpref_ref(s, idx, np.zeros(6), 4, nal_au, 4)
    assert len(out) == 0 and list(so) == [0] * 5 and summ["error"] == 0
    out, io, so, summ = R.to_lenpref_ref(s, idx[:0], None, 4, nal_au[:0], 0)
    assert len(out) == 0 and list(so) == [0] and summ["error"] == 0 and summ["nal_found"] == 0


def test_error_cases_of_the_forward_reference():
    s = np.arange(1, 101, dtype=np.uint8)
    idx = _entries([(3, 10), (13, 20), (27, 40)])
    au = np.array([0, 1, 1], dtype=np.uint32)
    assert R.to_lenpref_ref(s, idx, None, 4, au, 2)[3]["error"] == 0
    for bad in ([(3, 10), (21, 20), (27, 40)], [(3, 10), (13, 20), (27, 101)], [(3, 10), (9, 20), (27, 40)]):
        out, io, so, summ = R.to_lenpref_ref(s, _entries(bad), None, 4, au, 2)
        assert summ["error"] == R.E_ARG and not len(out) and not len(io) and so is None
        assert R.to_lenpref_ref(s, _entries(bad), np.zeros(3), 4)[3]["error"] == R.E_ARG      # checked whether kept or not
    for bad_au, n_aus in (([1, 1, 1], 2), ([0, 2, 2], 3), ([0, 1, 0], 2), ([0, 1, 1], 3), ([0, 1, 1], 1), ([0, 0, 0], 0)):
        assert R.to_lenpref_ref(s, idx, None, 4, np.array(bad_au, np.uint32), n_aus)[3]["error"] == R.E_ARG, (bad_au, n_aus)
    assert R.to_lenpref_ref(s, idx[:0], None, 4, au[:0], 1)[3]["error"] == R.E_ARG          # no NALs: no AUs
    out, io, so, summ = R.to_lenpref_ref(s, idx, None, 4, au, 2, out_cap=38)
    assert summ["error"] == R.E_CAPACITY and summ["stream_bytes"] == 39 and summ["nal_count"] == 3 and not len(out) and so is None
    assert R.to_lenpref_ref(s, idx, None, 4, au, 2, out_cap=39)[3]["error"] == 0


@pytest.mark.parametrize("L,limit", [(1, 255), (2, 65535)])
def test_length_field_limits(L, limit):
    s = np.full(limit + 40, 0x55, dtype=np.uint8)
    fits, over = _entries([(3, 3 + limit)]), _entries([(3, 4 + limit)])
    out, io, _, summ = R.to_lenpref_ref(s, fits, None, L)
    assert summ["error"] == 0 and bytes(out[:L]) == b"\xff" * L and len(out) == L + limit
    back, _, bs = R.to_annexb_ref(out, [0], [len(out)], L, 3)
    assert bs["error"] == 0 and len(back) == 3 + limit
    assert R.to_lenpref_ref(s, over, None, L)[3]["error"] == R.E_ARG
    assert R.to_lenpref_ref(s, over, [0], L)[3]["error"] == 0              # ... only a KEPT NAL has to fit
    assert R.to_lenpref_ref(s, over, None, 4)[3]["error"] == 0


def test_error_cases_of_the_reverse_reference():
    rec = b"\x00\x02\xaa\xbb" + b"\x00\x00" + b"\x00\x01\xcc"             # three records, L = 2
    d = np.frombuffer(b"\xee" * 5 + rec + b"\xee" * 3, dtype=np.uint8)
    out, so, summ = R.to_annexb_ref(d, [5, 9], [4, 5], 2, 3)
    assert bytes(out) == b"\x00\x00\x01\xaa\xbb" + b"\x00\x00\x01" + b"\x00\x00\x01\xcc" and list(so) == [0, 5, 12]
    assert summ == dict(nal_count=3, nal_found=2, rbsp_bytes=0, stream_bytes=12, stop_reason=-1, error=0, reserved0=0)
    # table order, not buffer order; samples may repeat
    out, so, _ = R.to_annexb_ref(d, [9, 5, 9], [5, 4, 2], 2, 4)
    assert bytes(out) == b"\x00\x00\x00\x01" + b"\x00\x00\x00\x01\xcc" + b"\x00\x00\x00\x01\xaa\xbb" + b"\x00\x00\x00\x01"
    assert list(so) == [0, 9, 15, 19]
    for off, size, bad in (([5, 9], [4, 8], 2),                    # leaves the buffer
                           ([5, (1 << 64) - 2], [4, 4], 2),        # the sum wraps
                           ([5, 9], [3, 5], 1),                    # a length larger than what is left
                           ([5, 9], [4, 3], 2),                    # one byte left in front of the end: fewer than L
                           ([5, 5], [3, 5], 1)):                   # the lowest of two
        out, so, summ = R.to_annexb_ref(d, off, size, 2, 3)
        assert summ["error"] == R.E_ARG and summ["reserved0"] == bad and not len(out) and so is None, (off, size)
    assert R.to_annexb_ref(d, [5, 9], [4, 5], 2, 3, nal_cap=2)[2]["error"] == R.E_CAPACITY
    assert R.to_annexb_ref(d, [5, 9], [4, 5], 2, 3, nal_cap=3)[2]["error"] == 0
    out, so, summ = R.to_annexb_ref(d, [5, 9], [4, 5], 2, 3, out_cap=11)
    assert summ["error"] == R.E_CAPACITY and summ["stream_bytes"] == 12 and summ["nal_count"] == 3 and so is None
    out, so, summ = R.to_annexb_ref(d, [], [], 2, 3)
    assert summ["error"] == 0 and summ["stop_reason"] == 0 and list(so) == [0] and not len(out)
    out, so, summ = R.to_annexb_ref(d, [3], [0], 2, 3)             # an empty sample
    assert summ["error"] == 0 and summ["nal_count"] == 0 and list(so) == [0, 0]
