"""hbs_au_times on the CPU side: the symbol, the layout of hbs_au_times_params as a C compiler sees it against the numpy record,
the three constants."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "hevcbitstream_amd.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(hbs_au_times_params), offsetof(hbs_au_times_params, flags),
           offsetof(hbs_au_times_params, tick), offsetof(hbs_au_times_params, base_time), offsetof(hbs_au_times_params, delay),
           offsetof(hbs_au_times_params, reserved), sizeof(((hbs_au_times_params*)0)->reserved));
    printf("%u %u %u %d\n", HBS_AUT_MAX_SPAN, HBS_AUT_DELAY_GIVEN, HBS_AUT_WRAP33, HBS_E_DEPTH);
    return 0;
}
"""


def test_symbol_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    lib = hbs.load_library()
    assert "hbs_au_times" in declared_functions() and "hbs_au_times" in EXPORTS and hasattr(lib, "hbs_au_times")
    assert len(lib.hbs_au_times.argtypes) == 9


def test_params_layout_and_constants_as_compiled(tmp_path):
    import hevcbitstream_amd as hbs
    from tests import _au_times_ref as T
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = tmp_path / "layout"
    built = subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    layout, consts = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    P = hbs.AU_TIMES_PARAMS
    assert layout == [P.itemsize] + [P.fields[f][1] for f in ("flags", "tick", "base_time", "delay", "reserved")] + [P.fields["reserved"][0].itemsize]
    assert layout == [32, 0, 4, 8, 16, 20, 12]
    assert consts == [hbs.AUT_MAX_SPAN, hbs.AUT_DELAY_GIVEN, hbs.AUT_WRAP33, T.E_DEPTH] == [1024, 1, 2, -6]
    assert (T.MAX_SPAN, T.DELAY_GIVEN, T.WRAP33) == (1024, 1, 2)
    assert (T.CVS_START, T.NO_PICTURE) == (hbs.AU_CVS_START, hbs.AU_NO_PICTURE)


def test_header_lists_the_call_among_the_graph_safe_ones():
    hdr = open(os.path.join(ROOT, "include", "hevcbitstream_amd.h")).read()
    graphs = hdr[hdr.index("HIP graphs."):hdr.index("int  hbs_ctx_create")]
    assert re.search(r"\bhbs_au_times\b", graphs) and "tests/test_gpu_au_times.py" in graphs


def test_params_helper():
    import hevcbitstream_amd as hbs
    p = hbs.au_times_params(tick=3003, base_time=7, delay=4, flags=hbs.AUT_WRAP33)
    assert p.dtype == hbs.AU_TIMES_PARAMS and p.tobytes() == bytes([3, 0, 0, 0]) + (3003).to_bytes(4, "little") + (7).to_bytes(8, "little") + \
        (4).to_bytes(4, "little") + bytes(12)
    assert int(hbs.au_times_params()["flags"][0]) == 0
