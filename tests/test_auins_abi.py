"""hbs_au_insert on the CPU side: the symbols and constants, hbs_aud_nal_host against the plain restatement of the rule
(tests/_auins_ref.py), and that restatement against the scan (the oracle's walk of its output gives its d_index_out) and
against the access-unit rules (tests/_au_ref.py on its output gives its d_au_out)."""
import numpy as np

from tests import _au_ref as A
from tests import _auins_ref as R


def test_symbols_declared_exported_and_bound():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    for name in ("hbs_au_insert", "hbs_aud_nal_host"):
        assert name in declared_functions()
        assert name in EXPORTS
        assert hasattr(hbs.load_library(), name)
    assert hasattr(hbs.Context, "au_insert") and hasattr(hbs.Context, "au_insert_async") and callable(hbs.aud_nal)
    assert (hbs.AUINS_AUD, hbs.AUINS_PARAM_SETS, hbs.AUINS_PARAM_SETS_FIRST) == (R.AUD, R.PARAM_SETS, R.PARAM_SETS_FIRST) == (1, 2, 4)
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hevcbitstream_amd.h")).read()
    for name, val in (("AUD", 1), ("PARAM_SETS", 2), ("PARAM_SETS_FIRST", 4)):
        m = re.search(r"#define HBS_AUINS_%s\s+(\d+)u" % name, hdr)
        assert m and int(m.group(1)) == val, name


def test_aud_nal_host_against_the_reference():
    import hevcbitstream_amd as hbs
    for tid1 in range(8):
        for st in range(8):
            got = hbs.aud_nal(tid1, st)
            assert got == R.aud_nal(tid1, st), (tid1, st)
            assert got[:5] == b"\x00\x00\x00\x01\x46" and got[5] == tid1 and got[6] & 0x1F == 0x10
    assert [hbs.aud_nal(1, st)[6] >> 5 for st in range(8)] == [2, 2, 1, 2, 0, 2, 1, 2]
    assert hbs.aud_nal(9, 4) == R.aud_nal(1, 4)                      # T = temporal_id_plus1 & 7
    assert hbs.load_library().hbs_aud_nal_host(1, 4, None) == R.E_ARG


def cases(seed, count):
    rng = np.random.default_rng(seed)
    for it in range(count):
        n_aus = int(rng.choice([1, 2, 5, 17, 40]))
        case = R.random_case(rng, n_aus, irap_every=int(rng.choice([0, 1, 3, 6])), sets_at_start=bool(rng.random() < 0.8),
                             last_without_picture=bool(rng.random() < 0.3), lead_junk=int(rng.integers(1, 9)) if it % 15 == 1 else 0)
        first = int(rng.integers(0, n_aus)) if it % 3 == 0 else 0
        count_ = int(rng.integers(1, n_aus + 2)) if it % 3 == 0 else n_aus
        yield case, first, count_, int(rng.integers(0, 8))


def test_random_case_is_what_a_scan_finds(orc):
    """the index random_case computes is the oracle's walk of its stream"""
    for (stream, index, *_), _, _, _ in cases(3, 60):
        got, _, _ = orc.index_extract(stream)
        assert np.array_equal(got, index)


def test_reference_matches_the_walk_of_its_output(orc):
    """its output, scanned again, gives exactly its d_index_out -- but for the two stated exceptions, which match their formula"""
    total = plain = inserted = 0
    seen = [0, 0]
    for (stream, index, parsed, compact, au, nal_au), first, count, flags in cases(5, 240):
        out, io, src, nau, au_out, s = R.au_insert(stream, index, parsed, au, nal_au, first, count, flags)
        assert s["error"] == 0 and s["stream_bytes"] == len(out) and s["nal_count"] == len(io)
        assert s["reserved"][0] == int(np.sum(src == R.NONE))
        inserted += s["reserved"][0] + s["reserved"][1]
        got, _, why = orc.index_extract(out)
        want, junk, short = R.rescan_exceptions(stream, index, au, first, count, out, io, src)
        total += 1
        if want is None:
            plain += 1
            assert np.array_equal(got, io), (first, count, flags)
            assert why == (-1 if len(io) else 0)
        else:
            assert np.array_equal(got, want), (first, count, flags, junk, short)
            seen[0] += 1 if junk else 0
            seen[1] += 1 if short else 0
    assert plain * 10 >= total * 9, (plain, total)
    assert seen[0] > 0 and inserted > 1000


def test_leading_junk_exception_is_as_stated(orc):
    """something inserted at stream offset 0 with bytes in front of the first start code: the scan of the output attaches them
    to the inserted NAL; every NAL behind is found as d_index_out says"""
    rng = np.random.default_rng(8)
    nals = [R.nal(1, first=1, size=9), R.nal(1, first=1, size=12)]
    stream, index, parsed, compact, au, nal_au = R.build(rng, nals, lead_junk=5)
    out, io, src, _, _, s = R.au_insert(stream, index, parsed, au, nal_au, 0, 2, R.AUD)
    want, junk, short = R.rescan_exceptions(stream, index, au, 0, 2, out, io, src)
    assert s["reserved"][0] == 2 and junk == 5 and not short
    got, _, _ = orc.index_extract(out)
    assert int(got["start"][0]) == 4 and int(got["end"][0]) == 7 + 5                 # the AUD and the five bytes
    assert np.array_equal(got, want) and np.array_equal(got["end"][1:], io["end"][1:])


def test_short_last_nal_exception_is_the_filters(orc):
    rng = np.random.default_rng(12)
    nals = [R.nal(35, size=3), R.nal(1, first=1, size=9), R.nal(40, size=1, junk=2)]
    stream, index, parsed, compact, au, nal_au = R.build(rng, nals)
    out, io, src, _, _, s = R.au_insert(stream, index, parsed, au, nal_au, 0, 1, R.PARAM_SETS_FIRST | R.AUD)
    assert s["reserved"] == [0, 0, 1] and np.array_equal(out, stream)
    want, junk, short = R.rescan_exceptions(stream, index, au, 0, 1, out, io, src)
    assert short and not junk and len(want) == 2
    assert np.array_equal(orc.index_extract(out)[0][["start", "end"]], want[["start", "end"]])


def test_insertion_moves_no_au_boundary():
    """tests/_au_ref.py on the output, its records gathered through d_nal_src with a type-35 record for each inserted AUD, over the
    full range: d_au_out -- grouping, first_vcl, flags, picture order counts.  The sets in force are of layer 0 here: a copy keeps
    its nuh_layer_id, and by 7.4.2.4.4 a parameter set of another layer begins no access unit (the header states it)."""
    rng = np.random.default_rng(6)
    checked = 0
    for it in range(120):
        n_aus = int(rng.choice([1, 3, 9, 30]))
        stream, index, parsed, compact, au, nal_au = R.random_case(rng, n_aus, irap_every=int(rng.choice([1, 4, 6])),
                                                                   last_without_picture=bool(it % 4 == 0), layer_sets=False)
        flags = it % 8
        out, io, src, nau, au_out, s = R.au_insert(stream, index, parsed, au, nal_au, 0, n_aus, flags)
        p, c = R.gather_records(parsed, compact, src, au_out, nau)
        want_au, want_nal_au, _, _ = A.access_units(io, p, c, None, R.SPS_OFF)
        assert np.array_equal(want_nal_au, nau), (it, flags)
        assert len(want_au) == len(au_out)
        for f in au_out.dtype.names:
            assert np.array_equal(want_au[f], au_out[f]), (it, flags, f)
        checked += s["reserved"][0] + s["reserved"][1]
    assert checked > 500


def test_flags_zero_is_the_filter_of_the_range():
    rng = np.random.default_rng(9)
    from tests import _filter_ref as F
    stream, index, parsed, compact, au, nal_au = R.random_case(rng, 25)
    out, io, src, nau, au_out, s = R.au_insert(stream, index, parsed, au, nal_au, 4, 9, 0)
    keep = (nal_au >= 4) & (nal_au < 13)
    fout, fio, fs = F.filter_ref(stream, index, keep)
    assert np.array_equal(out, fout) and np.array_equal(io, fio) and np.array_equal(src, np.flatnonzero(keep))
    assert s["reserved"] == [0, 0, 9] and {k: s[k] for k in fs} == fs


def test_errors_of_the_reference():
    rng = np.random.default_rng(10)
    stream, index, parsed, compact, au, nal_au = R.random_case(rng, 12)
    good = R.au_insert(stream, index, parsed, au, nal_au, 0, 12, 7)[5]
    assert good["error"] == 0
    for what in range(5):
        i2, a2, n2 = index.copy(), au.copy(), nal_au.copy()
        if what == 0:
            i2["start"][3] = i2["end"][3] + 1
        elif what == 1:
            a2["first_nal"][5] += 1
        elif what == 2:
            a2["unit_end"][7] += 1
        elif what == 3:
            n2[int(au["first_nal"][6])] = 5
        else:
            a2["nal_count"][11] += 1
        s = R.au_insert(stream, i2, parsed, a2, n2, 0, 12, 7)[5]
        assert s["error"] == R.E_ARG and s["nal_count"] == 0 and s["reserved"] == [0, 0, 0], what
    s = R.au_insert(stream, index, parsed, au, nal_au, 0, 12, 7, out_cap=good["stream_bytes"] - 1, index_cap=good["nal_count"])[5]
    assert s == dict(good, error=R.E_CAPACITY)
    s = R.au_insert(stream, index, parsed, au, nal_au, 0, 12, 7, out_cap=good["stream_bytes"], index_cap=good["nal_count"] - 1)[5]
    assert s == dict(good, error=R.E_CAPACITY)
    assert R.au_insert(stream, index, parsed, au, nal_au, 12, 3, 7)[5]["nal_count"] == 0
    assert R.au_insert(stream, index, parsed, au, nal_au, 10, 30, 7)[5]["reserved"][2] == 2
