"""hbs_mp4_samples / hbs_mp4_init_read_host on the CPU side: the symbols declared, exported and bound, the record sizes, the
call's place in the header's list of calls that may be captured."""
import os

from tests import _mp4_read_ref as Q


def test_symbols_declared_exported_and_bound():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    for name in ("hbs_mp4_samples", "hbs_mp4_init_read_host"):
        assert name in declared_functions()
        assert name in EXPORTS
        assert hasattr(hbs.load_library(), name)
    assert hasattr(hbs.Context, "mp4_samples") and hasattr(hbs.Context, "mp4_samples_async")
    assert callable(hbs.mp4_read_params) and callable(hbs.mp4_init_read)
    for name in ("MP4_READ_PARAMS", "MP4_TRACK", "mp4_read_params", "mp4_init_read"):
        assert name in hbs.__all__


def test_record_sizes():
    import hevcbitstream_amd as hbs
    assert (hbs.MP4_READ_PARAMS.itemsize, hbs.MP4_TRACK.itemsize) == (32, 64)
    assert hbs.MP4_READ_PARAMS == Q.READ_PARAMS and hbs.MP4_TRACK == Q.TRACK
    p = hbs.mp4_read_params(track_id=3, trex_duration=4, trex_size=5, trex_flags=6)
    assert p.tobytes() == b"".join(int(v).to_bytes(4, "little") for v in (0, 3, 4, 5, 6, 0, 0, 0))


def test_header_declares_the_structs_and_lists_the_call():
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hevcbitstream_amd.h")).read()
    assert re.search(r"typedef struct hbs_mp4_read_params \{\s*/\* HOST memory, 32 bytes \*/", text)
    assert re.search(r"typedef struct hbs_mp4_track \{\s*/\* 64 bytes \*/", text)
    listed = text.split("HIP graphs.")[1].split("The list is what")[0]
    assert "hbs_mp4_samples" in listed and "hbs_mp4_fragment" in listed
    assert "tests/test_gpu_mp4_read.py" in text.split("The list is what")[1].split("replay")[0]
    assert "nothing reads MP4 on the device" not in text
