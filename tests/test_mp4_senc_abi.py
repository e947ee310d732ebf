"""hbs_mp4_senc_samples and hbs_mp4_init_unprotect_host on the CPU side: the params struct as ctypes lays it out against the numpy
records and against a C compiler's view of the header, the symbols in the built library's export list, the header's list of
graph-safe calls and the pointers from the sections that said the tables come "from elsewhere"."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hbs_mp4_senc_samples", "hbs_mp4_init_unprotect_host")


class Params(C.Structure):
    _fields_ = [("iv_size", C.c_uint32), ("track_id", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 5)]


SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "hevcbitstream_amd.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu\n", sizeof(hbs_mp4_senc_params), offsetof(hbs_mp4_senc_params, iv_size), offsetof(hbs_mp4_senc_params, track_id),
           offsetof(hbs_mp4_senc_params, flags), offsetof(hbs_mp4_senc_params, reserved));
    printf("%u\n", HBS_SENC_CLEAR_IF_ABSENT);
    return 0;
}
"""


def layout(struct):
    return [C.sizeof(struct)] + [getattr(struct, name).offset for name, _ in struct._fields_]


def test_struct_sizes_and_offsets():
    import hevcbitstream_amd as hbs
    from tests import _mp4_senc_ref as S
    assert layout(Params) == [32, 0, 4, 8, 12]
    for dtype in (hbs.MP4_SENC_PARAMS, S.PARAMS):
        assert layout(Params) == [dtype.itemsize] + [dtype.fields[name][1] for name, _ in Params._fields_]
    assert hbs.MP4_SENC_CLEAR_IF_ABSENT == S.CLEAR_IF_ABSENT == 1


def test_layouts_as_compiled(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = tmp_path / "layout"
    built = subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    rows = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert rows == [layout(Params), [1]]


def test_symbols_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    lib = hbs.load_library()
    nm = shutil.which("nm")
    listed = subprocess.run([nm, "-D", "--defined-only", hbs.library_path()], capture_output=True, text=True, check=True).stdout if nm else None
    for name, args in zip(NAMES, (13, 11)):
        assert name in declared_functions() and name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == args
        if listed is not None:
            assert re.search(r" T %s$" % name, listed, re.M)


def test_header_lists_the_call_among_the_graph_safe_ones_and_is_pointed_at():
    hdr = open(os.path.join(ROOT, "include", "hevcbitstream_amd.h")).read()
    graphs = hdr[hdr.index("HIP graphs."):hdr.index("int  hbs_ctx_create")]
    assert re.search(r"\bhbs_mp4_senc_samples\b", graphs.split("The list is what")[0]) and "tests/test_gpu_mp4_senc.py" in graphs.split("The list is what")[1]
    rd = hdr[hdr.index("STATED LIMITS: one track a call"):hdr.index("typedef struct hbs_mp4_read_params")]
    cenc = hdr[hdr.index("---- Common Encryption (ISO/IEC 23001-7, scheme `cenc`)"):hdr.index("#define HBS_CENC_ALIGN16")]
    cbcs = hdr[hdr.index("---- Common Encryption, scheme `cbcs`"):hdr.index("#define HBS_CBCS_DECRYPT")]
    prot = hdr[hdr.index("---- protected fragments: saiz, saio and senc"):hdr.index("typedef struct hbs_mp4_protect_params")]
    for section in (rd, cenc, cbcs, prot):
        assert "hbs_mp4_senc_samples" in section
    assert "hbs_mp4_init_unprotect_host" in rd and "hbs_mp4_init_unprotect_host" in cbcs and "hbs_mp4_init_unprotect_host" in prot
    own = hdr[hdr.index("---- protected fragments read back"):hdr.index("#define HBS_SENC_CLEAR_IF_ABSENT")]
    for word in ("STATED LIMITS", "PIFF", "saio but no senc", "sbgp", "several tracks", "cens / cbc1", "no host synchronisation", "never an authority",
                 "HBS_SENC_CLEAR_IF_ABSENT", "plan only", "16 bytes a sample"):
        assert word in own, word


def test_params_helper():
    import hevcbitstream_amd as hbs
    assert hbs.mp4_senc_params().tobytes() == bytes([8, 0, 0, 0]) + bytes(28)
    assert hbs.mp4_senc_params(iv_size=16, track_id=2, flags=1).tobytes() == bytes([16, 0, 0, 0, 2, 0, 0, 0, 1, 0, 0, 0]) + bytes(20)
