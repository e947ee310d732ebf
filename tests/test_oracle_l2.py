"""Pin the oracle's byte layer: against golden vectors generated from the real
reference (tests/golden/l2_vectors.json, made by make_golden_l2.py) and against
the reference itself on fuzz -- live when oracle/_ref is present (dev container),
else through its answers recorded on the same inputs (make_golden_fuzz.py)."""
import json
import os

import numpy as np
import pytest

from tests import _orc
from tests.golden.make_golden_fuzz import digest as answer_digest, load as load_answers

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "l2_vectors.json")))


def test_find_nal_unit_golden(orc):
    for hx, want in GOLD["find"]:
        assert list(orc.find_nal_unit(bytes.fromhex(hx))) == want, hx


def test_nal_to_rbsp_golden(orc):
    for hx, (r, ns, rs, data) in GOLD["n2r"]:
        got = orc.nal_to_rbsp(bytes.fromhex(hx))
        assert got[0] == r, hx
        if r >= 0:  # sizes are untouched (== input) on error in both
            assert got[1] == ns and got[2] == rs and got[3].hex() == data, hx
        else:
            assert got[1] == ns and got[2] == rs, hx


def test_rbsp_to_nal_golden(orc):
    for hx, (r, data) in GOLD["r2n"]:
        got = orc.rbsp_to_nal(bytes.fromhex(hx))
        assert got[0] == r and got[2].hex() == data, hx


def test_ten_nal_index_golden(orc):
    stream = np.fromfile(os.path.join(HERE, "golden", "ten_nal.hevc"), dtype=np.uint8)
    want = json.load(open(os.path.join(HERE, "golden", "ten_nal.index.json")))
    idx, why = orc.index_stream(stream)
    assert why == -1
    assert [[int(a), int(b)] for a, b in zip(idx["start"], idx["end"])] == [w[:2] for w in want]
    assert idx["status"][-1] & 4 and not idx["status"][:-1].any()


ALPHA = np.array([0, 0, 0, 0, 1, 1, 2, 3, 3, 4, 0x40, 0x80, 0xFF], dtype=np.uint8)


def l2_fuzz_inputs():
    rng = np.random.RandomState(7)
    for _ in range(4000):
        yield bytes(ALPHA[rng.randint(0, len(ALPHA), size=rng.randint(3, 64))])


def l2_answer(lib, b):
    return lib.find_nal_unit(b), lib.nal_to_rbsp(b), lib.rbsp_to_nal(b)


def test_fuzz_vs_reference(orc):
    """the oracle's three byte functions against the reference's: live where oracle/_ref is built, else against the
    reference's answers recorded on the same inputs (golden/fuzz_answers.json.gz, make_golden_fuzz.py)"""
    ref = _orc.reference()
    want = load_answers("l2_fuzz") if ref is None else None
    k = -1
    for k, b in enumerate(l2_fuzz_inputs()):
        got = l2_answer(orc, b)
        if ref is not None:
            assert got == l2_answer(ref, b), b.hex()
        else:
            assert answer_digest(got) == want[k], b.hex()
    assert k + 1 == 4000 and (want is None or len(want) == 4000)


def stream_loop_inputs():
    rng = np.random.RandomState(11)
    for _ in range(300):
        n = rng.randint(4, 400)
        s = ALPHA[rng.randint(0, len(ALPHA), size=n)].copy()
        s[rng.rand(n) < 0.5] = 0x55          # thin out so NALs have some length
        yield s


def reference_stream_loop(ref, s):
    """the hevc_analyze.c:135-205 loop driven on the reference: [(start, end)] of every NAL"""
    data = bytes(s)
    want, p = [], 0
    while True:
        r, st, en = ref.find_nal_unit(data[p:])
        if r <= 0:
            if r == -1:
                want.append((p + st, p + en))
            break
        want.append((p + st, p + en))
        p += en
    return want


def test_stream_loop_vs_reference(orc):
    """orc_index_stream == the hevc_analyze.c:135-205 loop driven on the reference (live where oracle/_ref is built, else
    the loop's answers recorded on the same streams)."""
    ref = _orc.reference()
    want = load_answers("stream_loop") if ref is None else None
    k = -1
    for k, s in enumerate(stream_loop_inputs()):
        idx, why = orc.index_stream(s)
        got = [(int(a), int(b)) for a, b in zip(idx["start"], idx["end"])]
        if ref is not None:
            assert got == reference_stream_loop(ref, s), bytes(s).hex()
        else:
            assert answer_digest(got) == want[k], bytes(s).hex()
    assert k + 1 == 300 and (want is None or len(want) == 300)


@pytest.mark.ref
def test_reference_baseline_driver(orc, ref):
    """oracle/ref_driver.c (what bench.py times as the "reference" CPU baseline) walks a stream like the oracle does:
    same NAL starts, same RBSP bytes"""
    import ctypes as C
    import os
    drv = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_driver.so")
    if not os.path.exists(drv):
        pytest.skip("oracle/_ref/libref_driver.so not built")
    lib = C.CDLL(drv)
    u8p = C.POINTER(C.c_uint8)
    lib.ref_walk.restype = C.c_int64
    lib.ref_walk.argtypes = [u8p, C.c_int64, u8p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.c_int64]
    for mode in (0, 1):
        stream, idx, arena = orc.gen_stream(0x77 + mode, 150, mode)
        buf = stream.copy()
        out = np.zeros(len(buf) + 64, dtype=np.uint8)
        starts = np.zeros(len(idx) + 8, dtype=np.uint64)
        tot = C.c_int64(0)
        n = lib.ref_walk(buf.ctypes.data_as(u8p), len(buf), out.ctypes.data_as(u8p), len(out), C.byref(tot),
                         starts.ctypes.data_as(C.POINTER(C.c_uint64)), len(starts))
        assert n == len(idx) and np.array_equal(starts[:n], idx["start"])
        assert tot.value == len(arena) and np.array_equal(out[:tot.value], arena)


def test_roundtrip_property(orc):
    """rbsp_to_nal(nal_to_rbsp(x)) == x for accepted x not ending in 00 00 03
    (SURVEY.md App. B); and the synthetic generator's arena/index are what the
    oracle extracts from its stream."""
    for mode in (0, 1):
        s, idx, arena = orc.gen_stream(0x1234, 40, mode)
        i2, a2, why = orc.index_extract(s)
        assert why == -1
        assert np.array_equal(i2, idx) and np.array_equal(a2, arena)
        assert np.array_equal(orc.emit_annexb(a2, i2), s)
