"""tests/_au_times_ref.py, the restatement of hbs_au_times' header comment, on tables whose answers are worked out here by hand; and
the two forms of o(a) against each other on random tables."""
import numpy as np
import pytest

from tests import _au_times_ref as T

LO, HI = -(1 << 31), (1 << 31) - 1

# (name, POCs in decode order, heads, AUs without a picture, o(a), R, the largest span)
HAND = [
    ("I P B B", [0, 3, 1, 2], [], [], [0, 3, 1, 2], 1, 2),
    ("GOP-8 pyramid", [0, 8, 4, 2, 1, 3, 6, 5, 7], [], [], [0, 8, 4, 2, 1, 3, 6, 5, 7], 3, 7),
    ("CRA first, RASL pictures of lower POC behind it", [16, 13, 14, 15, 17, 18], [], [], [3, 0, 1, 2, 4, 5], 1, 3),
    ("two IDR segments, POC falls across the head", [0, 2, 1, 0, 2, 1], [3], [], [0, 2, 1, 3, 5, 4], 1, 1),
    ("a high key in front of a head is not counted behind it", [0, 9, 1, 2], [2], [], [0, 1, 2, 3], 0, 0),
    ("equal POCs go in decode order", [5, 5, 5, 3, 3], [], [], [2, 3, 4, 0, 1], 3, 4),
    ("AUs without a picture in front, in the middle, at the end", [9, 9, 4, 2, 7, 3, 1], [], [0, 1, 4, 6], [0, 1, 6, 2, 3, 4, 5], 1, 4),
    ("the lowest and the highest POC", [HI, LO, 0, HI, LO], [], [], [3, 0, 2, 4, 1], 3, 4),
    ("a head without a picture takes the key in front of it", [5, 1, 7, 3], [2], [2], [1, 0, 2, 3], 1, 1),
]


@pytest.mark.parametrize("name,pocs,heads,nopic,want,R,span", HAND, ids=[h[0] for h in HAND])
def test_hand_worked(name, pocs, heads, nopic, want, R, span):
    au = T.table(pocs, heads, nopic)
    n = len(au)
    r = T.au_times(au, tick=10, base_time=100)
    assert r["order"].tolist() == want
    # a permutation that maps every segment onto itself
    for s, e in T.segments(au):
        assert sorted(want[s:e]) == list(range(s, e))
    assert [int(r["display"][o]) for o in want] == list(range(n))
    back, fwd = T.spans(au)
    assert max(back.max(), fwd.max()) == span
    s = r["summary"]
    assert s == dict(nal_count=n, nal_found=len(heads) + 1, rbsp_bytes=heads[-1] if heads else 0, stream_bytes=0, stop_reason=0, error=0,
                     reserved=[R, R, 0])
    assert r["dts"].tolist() == [100 + 10 * a for a in range(n)]
    assert r["pts"].tolist() == [100 + 10 * (o + R) for o in want]
    assert len(set(r["pts"].tolist())) == n and all(p >= d for p, d in zip(r["pts"].tolist(), r["dts"].tolist()))
    for d in range(R + 3):
        g = T.au_times(au, tick=10, base_time=100, delay=d)
        late = sum(1 for a in range(n) if want[a] + d < a)
        assert g["summary"]["reserved"] == [d, R, late] and (late == 0) == (d >= R)
        assert g["pts"].tolist() == [100 + 10 * (o + d) for o in want] and g["order"].tolist() == want
    # modulo 2^33, both tables
    w = T.au_times(au, tick=10, base_time=(1 << 33) - 25, flags=T.WRAP33)
    assert w["dts"].tolist() == [((1 << 33) - 25 + 10 * a) % (1 << 33) for a in range(n)]
    assert w["pts"].tolist() == [((1 << 33) - 25 + 10 * (o + R)) % (1 << 33) for o in want]
    assert w["exact_pts"] == [(1 << 33) - 25 + 10 * (o + R) for o in want]


def test_pyramids_span_one_less_than_the_gop():
    for gop in (2, 4, 8, 16, 32, 64):
        au = T.table(T.pyramid(gop, 3))
        back, fwd = T.spans(au)
        assert max(back.max(), fwd.max()) == gop - 1
        r = T.au_times(au)
        assert r["order"].tolist() == T.pyramid(gop, 3) and r["summary"]["reserved"][1] == gop.bit_length() - 1


def test_span_limit():
    ok = T.table([0] * 3 + [9] + [1] * T.MAX_SPAN)
    assert T.au_times(ok)["summary"]["reserved"][1] == 1 and int(T.spans(ok)[1].max()) == T.MAX_SPAN
    over = T.table([0] * 3 + [9] + [1] * (T.MAX_SPAN + 1))
    r = T.au_times(over)
    # the 9 looks too far forwards; the last 1 looks as far backwards, but lies behind it
    assert r["summary"] == dict(nal_count=0, nal_found=0, rbsp_bytes=0, stream_bytes=0, stop_reason=0, error=T.E_DEPTH, reserved=[4, 0, 0])
    assert r["order"] is None
    cut = T.table([0] * 3 + [9] + [1] * (T.MAX_SPAN + 1), heads=[600])
    assert T.au_times(cut)["summary"]["error"] == 0


def test_refusals():
    assert not T.refused(0) and not T.refused((1 << 32) - 1) and T.refused(1 << 32)
    assert T.refused(5, tick=0) and T.refused(5, flags=4) and T.refused(5, reserved=(0, 1, 0)) and T.refused(5, base_time=T.LIMIT)
    assert not T.refused(5, base_time=T.LIMIT - 1 - (5 + T.MAX_SPAN)) and T.refused(5, base_time=T.LIMIT - (5 + T.MAX_SPAN))
    assert not T.refused(5, base_time=T.LIMIT - 1 - 7 * 3, tick=3, delay=2) and T.refused(5, base_time=T.LIMIT - 7 * 3, tick=3, delay=2)
    assert T.refused(0, base_time=T.LIMIT - T.MAX_SPAN) and not T.refused(0, base_time=T.LIMIT - 1, delay=0)


def test_the_two_forms_of_the_output_slot_agree():
    rng = np.random.default_rng(11)
    for _ in range(200):
        n = int(rng.integers(1, 80))
        au = T.table(rng.integers(-6, 6, n).tolist(), heads=rng.integers(0, n, int(rng.integers(0, 4))).tolist(),
                     nopic=rng.integers(0, n, int(rng.integers(0, 5))).tolist())
        key, o = T.keys(au), T.order(au)
        for s, e in T.segments(au):
            for a in range(s, e):
                assert o[a] == a + sum(1 for b in range(a + 1, e) if key[b] < key[a]) - sum(1 for b in range(s, a) if key[b] > key[a])
