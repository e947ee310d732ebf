"""hbs_cbcs_crypt on the CPU side: the params struct as ctypes lays it out against the numpy record and against a C compiler's
view of the header, the flags, the symbol in the built library's export list, the header's list of graph-safe calls."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Params(C.Structure):
    _fields_ = [("key", C.c_uint8 * 16), ("iv0", C.c_uint8 * 16), ("iv_mode", C.c_uint32), ("flags", C.c_uint32), ("crypt_byte_block", C.c_uint8),
                ("skip_byte_block", C.c_uint8), ("reserved0", C.c_uint16), ("reserved1", C.c_uint32)]


SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "hevcbitstream_amd.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(hbs_cbcs_params), offsetof(hbs_cbcs_params, key), offsetof(hbs_cbcs_params, iv0),
           offsetof(hbs_cbcs_params, iv_mode), offsetof(hbs_cbcs_params, flags), offsetof(hbs_cbcs_params, crypt_byte_block),
           offsetof(hbs_cbcs_params, skip_byte_block), offsetof(hbs_cbcs_params, reserved0), offsetof(hbs_cbcs_params, reserved1));
    printf("%u %u\n", HBS_CBCS_DECRYPT, HBS_CBCS_WHOLE_RUNS);
    return 0;
}
"""


def layout(struct):
    return [C.sizeof(struct)] + [getattr(struct, name).offset for name, _ in struct._fields_]


def test_struct_size_and_offsets():
    import hevcbitstream_amd as hbs
    from tests import _cbcs_ref as R
    assert layout(Params) == [48, 0, 16, 32, 36, 40, 41, 42, 44]
    for dtype in (hbs.CBCS_PARAMS, R.PARAMS):
        assert layout(Params) == [dtype.itemsize] + [dtype.fields[name][1] for name, _ in Params._fields_]


def test_layout_and_constants_as_compiled(tmp_path):
    import hevcbitstream_amd as hbs
    from tests import _cbcs_ref as R
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = tmp_path / "layout"
    built = subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    rows = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert rows[0] == layout(Params)
    assert rows[1] == [hbs.CBCS_DECRYPT, hbs.CBCS_WHOLE_RUNS] == [R.DECRYPT, R.WHOLE_RUNS] == [1, 2]


def test_symbol_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    lib = hbs.load_library()
    nm = shutil.which("nm")
    listed = subprocess.run([nm, "-D", "--defined-only", hbs.library_path()], capture_output=True, text=True, check=True).stdout if nm else None
    name = "hbs_cbcs_crypt"
    assert name in declared_functions() and name in EXPORTS and hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == 11
    if listed is not None:
        assert re.search(r" T %s$" % name, listed, re.M)


def test_header_lists_the_call_among_the_graph_safe_ones():
    hdr = open(os.path.join(ROOT, "include", "hevcbitstream_amd.h")).read()
    graphs = hdr[hdr.index("HIP graphs."):hdr.index("int  hbs_ctx_create")]
    assert re.search(r"\bhbs_cbcs_crypt\b", graphs) and "tests/test_gpu_cbcs.py" in graphs
    assert "capture" in graphs[graphs.index("So does hbs_cbcs_crypt"):]
    # hbs_cenc_crypt's own comment points at the call and still says that it refuses the scheme
    cenc = hdr[hdr.index("---- Common Encryption (ISO/IEC 23001-7, scheme `cenc`)"):hdr.index("#define HBS_CENC_ALIGN16")]
    assert "hbs_cbcs_crypt" in cenc and "anything but cenc is refused" in cenc


def test_params_helper():
    import hevcbitstream_amd as hbs
    p = hbs.cbcs_params(bytes(range(16)), iv0=b"\x07" * 16, flags=hbs.CBCS_DECRYPT | hbs.CBCS_WHOLE_RUNS, crypt_byte_block=3, skip_byte_block=7)
    assert p.tobytes() == bytes(range(16)) + b"\x07" * 16 + bytes([1, 0, 0, 0, 3, 0, 0, 0, 3, 7, 0, 0, 0, 0, 0, 0])
    q = hbs.cbcs_params(bytes(16))
    assert (int(q["iv_mode"][0]), int(q["flags"][0]), int(q["crypt_byte_block"][0]), int(q["skip_byte_block"][0])) == (0, 0, 1, 9)
    assert int(hbs.cbcs_params(bytes(16), iv0=bytes(16), iv_mode=0)["iv_mode"][0]) == 0
