"""hbs_cenc_subsamples / hbs_cenc_crypt on the CPU side: the three structs as ctypes lays them out against the numpy records and
against a C compiler's view of the header, the constants, both symbols in the built library's export list."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Subsample(C.Structure):
    _fields_ = [("clear", C.c_uint32), ("protect", C.c_uint32)]


class PlanParams(C.Structure):
    _fields_ = [("length_size", C.c_int32), ("flags", C.c_uint32), ("clear_lead", C.c_uint32), ("reserved", C.c_uint32)]


class Params(C.Structure):
    _fields_ = [("key", C.c_uint8 * 16), ("iv0", C.c_uint8 * 16), ("scheme", C.c_uint32), ("iv_mode", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "hevcbitstream_amd.h"
int main(void)
{
    printf("%zu %zu %zu\n", sizeof(hbs_cenc_subsample), offsetof(hbs_cenc_subsample, clear), offsetof(hbs_cenc_subsample, protect));
    printf("%zu %zu %zu %zu %zu\n", sizeof(hbs_cenc_plan_params), offsetof(hbs_cenc_plan_params, length_size), offsetof(hbs_cenc_plan_params, flags),
           offsetof(hbs_cenc_plan_params, clear_lead), offsetof(hbs_cenc_plan_params, reserved));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(hbs_cenc_params), offsetof(hbs_cenc_params, key), offsetof(hbs_cenc_params, iv0),
           offsetof(hbs_cenc_params, scheme), offsetof(hbs_cenc_params, iv_mode), offsetof(hbs_cenc_params, flags), offsetof(hbs_cenc_params, reserved));
    printf("%u %u\n", HBS_CENC_ALIGN16, HBS_CENC_SCHEME_CENC);
    return 0;
}
"""


def layout(struct):
    return [C.sizeof(struct)] + [getattr(struct, name).offset for name, _ in struct._fields_]


def test_struct_sizes_and_offsets():
    import hevcbitstream_amd as hbs
    assert layout(Subsample) == [8, 0, 4]
    assert layout(PlanParams) == [16, 0, 4, 8, 12]
    assert layout(Params) == [48, 0, 16, 32, 36, 40, 44]
    for struct, dtype in ((Subsample, hbs.CENC_SUBSAMPLE), (PlanParams, hbs.CENC_PLAN_PARAMS), (Params, hbs.CENC_PARAMS)):
        assert layout(struct) == [dtype.itemsize] + [dtype.fields[name][1] for name, _ in struct._fields_]


def test_layout_and_constants_as_compiled(tmp_path):
    import hevcbitstream_amd as hbs
    from tests import _cenc_ref as R
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = tmp_path / "layout"
    built = subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    rows = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert rows[:3] == [layout(Subsample), layout(PlanParams), layout(Params)]
    assert rows[3] == [hbs.CENC_ALIGN16, hbs.CENC_SCHEME_CENC] == [R.ALIGN16, R.SCHEME_CENC] == [1, int.from_bytes(b"cenc", "big")]
    assert R.SUBSAMPLE == hbs.CENC_SUBSAMPLE


def test_symbols_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    lib = hbs.load_library()
    nm = shutil.which("nm")
    listed = subprocess.run([nm, "-D", "--defined-only", hbs.library_path()], capture_output=True, text=True, check=True).stdout if nm else None
    for name, args in (("hbs_cenc_subsamples", 14), ("hbs_cenc_crypt", 11)):
        assert name in declared_functions() and name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == args
        if listed is not None:
            assert re.search(r" T %s$" % name, listed, re.M)


def test_header_lists_the_calls_among_the_graph_safe_ones():
    hdr = open(os.path.join(ROOT, "include", "hevcbitstream_amd.h")).read()
    graphs = hdr[hdr.index("HIP graphs."):hdr.index("int  hbs_ctx_create")]
    assert re.search(r"\bhbs_cenc_subsamples\b", graphs) and re.search(r"\bhbs_cenc_crypt\b", graphs) and "tests/test_gpu_cenc.py" in graphs
    assert "captured" in graphs[graphs.index("hbs_cenc_crypt takes its key"):]


def test_params_helpers():
    import hevcbitstream_amd as hbs
    p = hbs.cenc_plan_params(length_size=2, flags=hbs.CENC_ALIGN16, clear_lead=7)
    assert p.tobytes() == bytes([2, 0, 0, 0, 1, 0, 0, 0, 7, 0, 0, 0, 0, 0, 0, 0])
    q = hbs.cenc_params(bytes(range(16)), iv0=b"\x01" * 8)
    assert q.tobytes() == bytes(range(16)) + b"\x01" * 8 + bytes(8) + b"cnec" + bytes([1, 0, 0, 0]) + bytes(8)
    assert int(hbs.cenc_params(bytes(16))["iv_mode"][0]) == 0
