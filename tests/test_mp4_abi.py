"""hbs_mp4_fragment / hbs_mp4_init_host on the CPU side: the symbols declared, exported and bound, the record sizes, the flags."""
from tests import _mp4_ref as R


def test_symbols_declared_exported_and_bound():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    for name in ("hbs_mp4_fragment", "hbs_mp4_fragment_bytes_host", "hbs_mp4_init_host"):
        assert name in declared_functions()
        assert name in EXPORTS
        assert hasattr(hbs.load_library(), name)
    assert hasattr(hbs.Context, "mp4_fragment") and hasattr(hbs.Context, "mp4_fragment_async")
    assert callable(hbs.mp4_init) and callable(hbs.mp4_params) and callable(hbs.mp4_fragment_bytes)


def test_record_sizes_and_flags():
    import hevcbitstream_amd as hbs
    assert (hbs.MP4_PARAMS.itemsize, hbs.MP4_INIT_PARAMS.itemsize, hbs.MP4_FRAG.itemsize) == (32, 32, 48)
    assert hbs.MP4_PARAMS == R.PARAMS and hbs.MP4_INIT_PARAMS == R.INIT_PARAMS and hbs.MP4_FRAG == R.FRAG
    assert hbs.MP4_CUT_AT_IRAP == R.CUT_AT_IRAP == 1 and hbs.MP4_HEV1 == R.HEV1 == 1
    assert hbs.AU_IRAP == R.AU_IRAP and hbs.ACCESS_UNIT == R.ACCESS_UNIT and hbs.NAL_ENTRY == R.NAL_ENTRY
    p = hbs.mp4_params(length_size=2, flags=1, track_id=3, sequence=4, max_samples=5, sample_duration=6, base_time=7)
    assert p.tobytes() == R.params_record(R.params(2, 1, 3, 4, 5, 6, 7)).tobytes()


def test_header_states_the_sizes_and_flags():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hevcbitstream_amd.h")).read()
    assert re.search(r"#define\s+HBS_MP4_CUT_AT_IRAP\s+1u", text) and re.search(r"#define\s+HBS_MP4_HEV1\s+1\b", text)
    assert "hbs_mp4_fragment" in text.split("HIP graphs.")[1].split("The list is what")[0]
