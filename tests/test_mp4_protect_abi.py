"""hbs_mp4_protect and hbs_mp4_init_protect_host on the CPU side: both structs as ctypes lays them out against the numpy records and
against a C compiler's view of the header, the symbols in the built library's export list, the header's list of graph-safe
calls."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hbs_mp4_protect", "hbs_mp4_protect_bytes_host", "hbs_mp4_init_protect_host")


class Params(C.Structure):
    _fields_ = [("iv_size", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class Tenc(C.Structure):
    _fields_ = [("scheme", C.c_uint32), ("crypt_byte_block", C.c_uint8), ("skip_byte_block", C.c_uint8), ("iv_size", C.c_uint8),
                ("constant_iv_size", C.c_uint8), ("kid", C.c_uint8 * 16), ("constant_iv", C.c_uint8 * 16), ("reserved", C.c_uint32 * 6)]


SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "hevcbitstream_amd.h"
int main(void)
{
    printf("%zu %zu %zu %zu\n", sizeof(hbs_mp4_protect_params), offsetof(hbs_mp4_protect_params, iv_size), offsetof(hbs_mp4_protect_params, flags),
           offsetof(hbs_mp4_protect_params, reserved));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(hbs_mp4_tenc), offsetof(hbs_mp4_tenc, scheme), offsetof(hbs_mp4_tenc, crypt_byte_block),
           offsetof(hbs_mp4_tenc, skip_byte_block), offsetof(hbs_mp4_tenc, iv_size), offsetof(hbs_mp4_tenc, constant_iv_size),
           offsetof(hbs_mp4_tenc, kid), offsetof(hbs_mp4_tenc, constant_iv), offsetof(hbs_mp4_tenc, reserved));
    return 0;
}
"""


def layout(struct):
    return [C.sizeof(struct)] + [getattr(struct, name).offset for name, _ in struct._fields_]


def test_struct_sizes_and_offsets():
    import hevcbitstream_amd as hbs
    from tests import _mp4_protect_ref as P
    assert layout(Params) == [32, 0, 4, 8]
    assert layout(Tenc) == [64, 0, 4, 5, 6, 7, 8, 24, 40]
    for struct, dtypes in ((Params, (hbs.MP4_PROTECT_PARAMS, P.PARAMS)), (Tenc, (hbs.MP4_TENC, P.TENC))):
        for dtype in dtypes:
            assert layout(struct) == [dtype.itemsize] + [dtype.fields[name][1] for name, _ in struct._fields_]


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
    assert rows == [layout(Params), layout(Tenc)]


def test_symbols_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    lib = hbs.load_library()
    nm = shutil.which("nm")
    listed = subprocess.run([nm, "-D", "--defined-only", hbs.library_path()], capture_output=True, text=True, check=True).stdout if nm else None
    for name, args in zip(NAMES, (16, 3, 9)):
        assert name in declared_functions() and name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == args
        if listed is not None:
            assert re.search(r" T %s$" % name, listed, re.M)


def test_header_lists_the_call_among_the_graph_safe_ones():
    hdr = open(os.path.join(ROOT, "include", "hevcbitstream_amd.h")).read()
    graphs = hdr[hdr.index("HIP graphs."):hdr.index("int  hbs_ctx_create")]
    assert re.search(r"\bhbs_mp4_protect\b", graphs.split("The list is what")[0]) and "tests/test_gpu_mp4_protect.py" in graphs.split("The list is what")[1]
    # the three calls that said "not written" point at the writer, and still say what they do not do themselves
    frag = hdr[hdr.index("hbs_mp4_fragment writes the container"):hdr.index("typedef struct hbs_mp4_params")]
    cenc = hdr[hdr.index("---- Common Encryption (ISO/IEC 23001-7, scheme `cenc`)"):hdr.index("#define HBS_CENC_ALIGN16")]
    cbcs = hdr[hdr.index("---- Common Encryption, scheme `cbcs`"):hdr.index("#define HBS_CBCS_DECRYPT")]
    assert "hbs_mp4_protect" in frag and "no box says so yet" in frag
    assert "hbs_mp4_protect" in cenc and "NOT written or read: senc, saiz, saio, sinf / tenc, pssh" in cenc
    assert "hbs_mp4_protect" in cbcs and "hbs_mp4_init_protect_host" in cbcs
    own = hdr[hdr.index("---- protected fragments: saiz, saio and senc"):hdr.index("typedef struct hbs_mp4_protect_params")]
    for word in ("OUT OF SCOPE", "sbgp", "cens", "several tracks", "No host synchronisation".lower()):
        assert word in own, word


def test_params_helper():
    import hevcbitstream_amd as hbs
    assert hbs.mp4_protect_params().tobytes() == bytes([8, 0, 0, 0]) + bytes(28)
    assert hbs.mp4_protect_params(iv_size=16, flags=3).tobytes() == bytes([16, 0, 0, 0, 3, 0, 0, 0]) + bytes(24)
    assert (hbs.MP4_SCHEME_CENC, hbs.MP4_SCHEME_CBCS) == (int.from_bytes(b"cenc", "big"), int.from_bytes(b"cbcs", "big"))
