"""hbs_mp4_stbl_write / hbs_mp4_stbl_write_bytes_host / hbs_mp4_moov_host on the CPU side: the symbols declared, exported and
bound, the parameter record's size and fields, the rules in the header, the call's place in the header's list of calls that may
be captured."""
import os
import re

from tests import _mp4_stbl_write_ref as Wr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hevcbitstream_amd.h")


def test_symbols_declared_exported_and_bound():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    for name in ("hbs_mp4_stbl_write", "hbs_mp4_stbl_write_bytes_host", "hbs_mp4_moov_host"):
        assert name in declared_functions()
        assert name in EXPORTS
        assert hasattr(hbs.load_library(), name)
    assert hasattr(hbs.Context, "mp4_stbl_write") and hasattr(hbs.Context, "mp4_stbl_write_async")
    assert callable(hbs.mp4_moov) and callable(hbs.mp4_stbl_write_bytes) and callable(hbs.mp4_stbl_write_params)
    for name in ("MP4_STBL_WRITE_PARAMS", "mp4_stbl_write_params", "mp4_stbl_write_bytes", "mp4_moov"):
        assert name in hbs.__all__


def test_params_are_32_bytes_and_match_field_for_field():
    import hevcbitstream_amd as hbs
    assert hbs.MP4_STBL_WRITE_PARAMS.itemsize == 32 and hbs.MP4_STBL_WRITE_PARAMS == Wr.PARAMS
    text = open(HEADER).read()
    body = re.search(r"typedef struct hbs_mp4_stbl_write_params \{\s*/\* HOST memory, 32 bytes \*/(.*?)\} hbs_mp4_stbl_write_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(name.strip(), kind) for kind, names in re.findall(r"(uint32_t|uint64_t)\s+([^;]+);", body) for name in names.split(",")]
    assert fields == [("flags", "uint32_t"), ("max_chunk_samples", "uint32_t"), ("sample_duration", "uint32_t"), ("reserved0", "uint32_t"),
                      ("base_time", "uint64_t"), ("data_offset", "uint64_t")]
    at = 0
    for name, kind in fields:
        assert hbs.MP4_STBL_WRITE_PARAMS.fields[name][1] == at, name
        at += 4 if kind == "uint32_t" else 8
    assert at == 32
    p = hbs.mp4_stbl_write_params(flags=1, max_chunk_samples=2, sample_duration=3, base_time=4, data_offset=5)
    assert p.tobytes() == bytes([1, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0])
    # the bound: an entry a sample in every box
    assert hbs.mp4_stbl_write_bytes(0) == 100 and hbs.mp4_stbl_write_bytes(0, False, False) == 68
    assert hbs.mp4_stbl_write_bytes(10, True, True, 1) == 100 + 10 * (8 + 8 + 4 + 12 + 4 + 8)
    assert hbs.mp4_stbl_write_bytes((1 << 32) - 1, False, False) == 68 + ((1 << 32) - 1) * 28 and hbs.mp4_stbl_write_bytes(1 << 32) == 0


def test_header_states_the_rules_the_limits_and_the_capture():
    text = open(HEADER).read()
    listed = text.split("HIP graphs.")[1].split("The list is what")[0]
    assert "hbs_mp4_stbl_write" in listed.replace("hbs_mp4_stbl_write_", "")
    assert "tests/test_gpu_mp4_stbl_write.py" in text.split("The list is what")[1].split("replay")[0]
    assert text.index("progressive MP4 -> sample table") < text.index("sample table -> progressive MP4")
    section = text.split("sample table -> progressive MP4")[1].split("int64_t hbs_mp4_moov_host(")[0].replace("\n * ", " ")
    section = re.sub(r"\s+", " ", section)
    for words in ("CHUNKS", "contiguous iff", "s(k)", "max_chunk_samples > 0 and (k - s(k)) % max_chunk_samples == 0", "stco", "co64", "(c + 1, L_c, 1)",
                  "L_c != L_(c-1)", "sample_size = z(0)", "delta(k) = dts(k+1) - dts(k)", "delta(k) != delta(k-1)", "written iff d_pts != NULL",
                  "version 1 (signed offsets) iff some cts(k) < 0", "written iff d_sample_flags != NULL", "0x00010000", "A SAMPLE ERROR",
                  "A BOX SIZE ERROR", "reserved[2] = 1 + the lowest such sample", "reserved[0] = 1 + the box", "HBS_E_CAPACITY", "plan only",
                  "reserved[1] = the sum of all deltas", "hbs_mp4_stbl_find_host", "no host synchronisation", "no allocation once the scratch has its size",
                  "sized by n_samples alone", "never by a count computed on the device", "no sample byte is read", "no mvex", "no empty tables",
                  "ftyp + mdat + moov", "ftyp + moov + mdat", "data_offset = F + 8", "data_offset = P + T + 8", "T does not depend on data_offset",
                  "mdat header is the caller's 8 bytes", "one track", "no edit list", "no stz2", "no sdtp", "one sample entry", "no encryption",
                  "duration above 2^32 - 1", "not a multiple of 4", "past 2^32 - 1"):
        assert words in section, words
