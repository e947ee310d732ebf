#!/usr/bin/env python3
"""Generate tests/golden/fuzz_answers.json.gz from the REAL reference: its answers on the seeded fuzz inputs of
  test_oracle_l2.py::test_fuzz_vs_reference         find_nal_unit / nal_to_rbsp / rbsp_to_nal on 4000 short buffers
  test_oracle_l2.py::test_stream_loop_vs_reference  the hevc_analyze.c:135-205 loop on 300 short streams
  test_oracle_parse.py::test_parse_fuzz_vs_reference read_hevc_nal_unit on 120 synthetic sequences (rc, every struct, slice data)
  test_ext_types.py::test_oracle_against_the_reference_driver_fuzz  the extension readers on 6000 random NALs
so that those tests compare the oracle with the reference where oracle/_ref cannot be built (they compare with the live
reference where it can).  The tests regenerate the inputs from their seeds; per input this file keeps digest(answer), the
first 16 hex digits of the sha256 of the answer's repr.  Nothing of the reference's source is stored.

Run in the dev container only (needs oracle/_ref built from the reference sources by `make -C oracle ref`)."""
import gzip
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "fuzz_answers.json.gz")


def digest(answer):
    return hashlib.sha256(repr(answer).encode()).hexdigest()[:16]


def load(key):
    """the reference's answer digests for one test's inputs, in input order"""
    return json.load(gzip.open(PATH, "rt"))[key]


def main():
    sys.path.insert(0, ROOT)
    from tests import _orc
    from tests import test_ext_types as te
    from tests import test_oracle_l2 as l2
    from tests import test_oracle_parse as tp
    ref = _orc.reference()
    assert ref is not None, "build oracle/_ref first (make -C oracle ref)"
    out = {"l2_fuzz": [digest(l2.l2_answer(ref, b)) for b in l2.l2_fuzz_inputs()],
           "stream_loop": [digest(l2.reference_stream_loop(ref, s)) for s in l2.stream_loop_inputs()],
           "parse_fuzz": [digest(a) for a in tp.parse_fuzz_answers(_orc.ReferenceHevc())],
           "ext_fuzz": [digest(te.reference_ext_answer(te.reference_ext_driver(), nal)) for nal in te.ext_fuzz_inputs()]}
    with gzip.GzipFile(PATH, "wb", mtime=0) as f:
        f.write((json.dumps(out, separators=(",", ":")) + "\n").encode())
    print(PATH, {k: len(v) for k, v in out.items()}, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
