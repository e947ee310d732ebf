"""hbs_filter_annexb on the CPU side: the symbol, the record layout, the masks, and the numpy reference of its semantics
(tests/_filter_ref.py) against the oracle's find_nal_unit walk: scanning a filtered stream gives the specified output index."""
import numpy as np
import pytest

from tests import _filter_ref as F


def test_symbol_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    assert "hbs_filter_annexb" in declared_functions()
    assert "hbs_filter_annexb" in EXPORTS
    assert hasattr(hbs.load_library(), "hbs_filter_annexb")


def test_record_and_masks():
    import hevcbitstream_amd as hbs
    assert hbs.NAL_FILTER.itemsize == 24
    assert [hbs.NAL_FILTER.fields[f][1] for f in hbs.NAL_FILTER.names] == [0, 8, 12, 16, 20]

    def bits(m):
        return [t for t in range(64) if (m >> t) & 1]
    assert bits(hbs.NALMASK_VCL) == list(range(32))
    assert bits(hbs.NALMASK_IRAP) == list(range(16, 24))
    assert bits(hbs.NALMASK_PARAM_SETS) == [32, 33, 34]
    assert bits(hbs.NALMASK_SEI) == [39, 40]
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hevcbitstream_amd.h")).read()
    for name, val in (("VCL", hbs.NALMASK_VCL), ("IRAP", hbs.NALMASK_IRAP), ("PARAM_SETS", hbs.NALMASK_PARAM_SETS), ("SEI", hbs.NALMASK_SEI)):
        m = re.search(r"#define HBS_NALMASK_%s\s+(0x[0-9A-Fa-f]+)ull" % name, hdr)
        assert m and int(m.group(1), 16) == val, name


def test_header_fields_match_the_header_layout():
    s = np.array([0, 0, 1, (39 << 1) | 1, (5 << 3) | 3, 9], dtype=np.uint8)
    idx = np.zeros(1, dtype=F.NAL_ENTRY)
    idx["start"], idx["end"] = 3, 6
    t, layer, tid1, has = F.header_fields(s, idx)
    assert (int(t[0]), int(layer[0]), int(tid1[0]), bool(has[0])) == (39, 37, 3, True)


def _check_rescan(orc, stream, idx, arena, keep):
    out, io, summ = F.filter_ref(stream, idx, keep)
    assert summ["stream_bytes"] == len(out) and summ["nal_count"] == len(io)
    got, arena2, why = orc.index_extract(out)
    if F.rescan_misses_last(out, io):
        assert np.array_equal(got, io[:-1])
        return 1
    assert np.array_equal(got, io), (got[:4], io[:4])
    want = np.concatenate([arena[int(e["rbsp_off"]): int(e["rbsp_off"]) + int(e["rbsp_len"])] for e in idx[np.asarray(keep, bool)]]) \
        if len(io) else np.zeros(0, np.uint8)
    assert np.array_equal(arena2, want)
    assert why == (-1 if len(io) else 0)
    return 0


def test_reference_matches_the_walk_of_its_output(orc):
    rng = np.random.default_rng(7)
    misses = streams = 0
    for it in range(300):
        size = int(rng.choice([1, 5, 40, 300, 3000, 20000]))
        mean = int(rng.choice([2, 8, 60, 500, 4000]))
        s = F.random_stream(rng, size, mean)
        idx, arena, _ = orc.index_extract(s)
        for mode in range(3):
            if mode == 0:
                keep = rng.random(len(idx)) < rng.random()
            elif mode == 1:
                keep = F.rule_keep(s, idx, keep_types=int(rng.integers(0, 1 << 63)) | int(rng.integers(0, 2)) << 63,
                                   max_temporal_id_plus1=int(rng.integers(0, 8)), max_layer_id=int(rng.integers(0, 64)),
                                   keep_short=bool(rng.integers(0, 2)))
            else:
                keep = np.ones(len(idx), dtype=bool)
            misses += _check_rescan(orc, s, idx, arena, keep)
            streams += 1
    assert streams == 900
    assert misses > 0        # the exception occurs in these streams, and _check_rescan saw it exactly as stated


def test_keep_all_is_the_stream_up_to_the_last_nal(orc):
    rng = np.random.default_rng(11)
    for _ in range(50):
        s = F.random_stream(rng, 2000, 100)
        idx, _, _ = orc.index_extract(s)
        out, io, _ = F.filter_ref(s, idx, np.ones(len(idx), bool))
        assert np.array_equal(out, s[: int(idx["end"][-1])] if len(idx) else s[:0])


@pytest.mark.parametrize("prefix,payload,missed", [
    (b"\x00\x00\x01", b"\x40", False),             # start code begins its unit: found
    (b"\x00\x00\x00\x07\x00\x00\x01", b"\x40", True),          # 3-byte code behind junk, 1 payload byte: not found
    (b"\x00\x00\x00\x07\x00\x00\x01", b"\x40\x01", False),     # ... 2 payload bytes: found
    (b"\x00\x00\x00\x07\x00\x00\x00\x01", b"\x40", False),     # 4-byte code behind junk, 1 payload byte: found
    (b"\x00\x00\x00\x07\x00\x00\x00\x01", b"", True),          # ... no payload: not found
])
def test_the_stated_exception(orc, prefix, payload, missed):
    """a kept last NAL whose unit is `prefix + payload`, behind one ordinary NAL (junk in a unit follows the 00 00 00 that
    ended the NAL in front)"""
    first = b"\x00\x00\x01\x40\x01\x11\x22\x33"
    out = np.frombuffer(first + prefix + payload, dtype=np.uint8).copy()
    io = np.zeros(2, dtype=F.NAL_ENTRY)
    io["start"] = [3, len(first) + len(prefix)]
    io["end"] = [len(first), len(out)]
    assert F.rescan_misses_last(out, io) == missed
    got, _ = orc.index_stream(out)
    assert len(got) == (1 if missed else 2)
    assert int(got["end"][0]) == len(first)
