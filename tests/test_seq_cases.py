"""The cases of tests/test_gpu_sequences.py are what that file takes them for, by the plain reference loops alone: the plan
workgroups each one fills, no error in the good ones, HBS_E_ARG with the edited entry named in the malformed ones, HBS_E_CAPACITY
in the ones a byte short.  No GPU."""
import numpy as np
import pytest

from tests import _seq_cases as S

PARAMS = [(c, 188) for c in S.CALLS] + [(c, B) for c in S.PACKET_CALLS for B in (192, 204)]
IDS = ["%s-%d" % p if p[0] in S.PACKET_CALLS else p[0] for p in PARAMS]


@pytest.mark.parametrize("call,B", PARAMS, ids=IDS)
def test_plan_workgroups_of_every_case(call, B):
    small, large, odd = (S.case(call, w, B=B) for w in S.SIZES)
    assert all(b == 1 for b in S.plan_blocks(small)), (small, S.items(small))
    for n, per in S.items(large):
        assert S.blocks(n, per) >= 3 and n % per, (large, n, per)
    for lo, mid, hi in zip(S.plan_blocks(small), S.plan_blocks(odd), S.plan_blocks(large)):
        assert lo < mid < hi, (odd, S.items(odd), S.items(large))
    assert S.items(S.empty(call, B))[0][0] == 0      # (hbs_au_insert: no NALs under a table of AUs)
    if call == "tsd":                              # more scratch than the small case's: 64 bytes a block, carved in units of 256
        assert S.plan_blocks(large)[0] * 64 > 256
    if call == "tsm":                              # three copy workgroups and more, the last one ragged
        packets = S.summary_of(large)["nal_count"]
        assert packets > 2 * S.TSM_COPY_BLOCK and packets % S.TSM_COPY_BLOCK, packets
        assert S.blocks(S.summary_of(small)["nal_count"], S.TSM_COPY_BLOCK) == 1
    for c in (small, large, odd):                  # short payloads, outputs of a few MB at the most
        assert 0 < c.caps["out_cap"] < (4 << 20), (c, c.caps)


@pytest.mark.parametrize("call,B", PARAMS, ids=IDS)
def test_the_odd_case_differs(call, B):
    small, large, odd = (S.case(call, w, B=B).a for w in S.SIZES)
    if call in ("a2l", "l2a"):
        assert odd["L"] != small["L"] == large["L"]
        assert call == "a2l" or odd["sc"] != small["sc"] == large["sc"]
    elif call == "tsd":
        assert odd["B"] != small["B"] == large["B"] == B and odd["pid"] != small["pid"]
    elif call == "tsm":
        assert odd["prm"]["packet_bytes"] != small["prm"]["packet_bytes"] == large["prm"]["packet_bytes"] == B
        assert odd["prm"]["flags"] != small["prm"]["flags"] == large["prm"]["flags"]
    else:
        assert odd["flags"] != small["flags"] == large["flags"]


@pytest.mark.parametrize("call,B", PARAMS, ids=IDS)
def test_good_cases_and_the_empty_one_have_no_error(call, B):
    for c in [S.case(call, w, B=B) for w in S.SIZES]:
        for plan in (True, False):
            s = S.summary_of(c, plan)
            assert s["error"] == 0 and S.reserved0(s) == (s["reserved"][0] if call == "ins" else 0), (c, plan, s)
        assert S.summary_of(c)["stream_bytes"] == c.caps["out_cap"] == c.room["out"] == len(S.want(c)[0])
    e = S.empty(call, B)
    s = S.summary_of(e)
    assert s["error"] == 0 and s["nal_count"] == 0 and s["stream_bytes"] == 0 and len(S.want(e)[0]) == 0, s
    assert s["nal_found"] == 0 and s["stop_reason"] == 0 and S.reserved0(s) == 0


@pytest.mark.parametrize("call,B", PARAMS, ids=IDS)
def test_malformed_variants_name_their_entry(call, B):
    for which in S.SIZES:
        good = S.case(call, which, B=B)
        n, per = S.items(good)[-1]
        for what in ("bad_early", "bad_late"):
            v = S.variant(good, what)
            if what == "bad_early":
                assert 0 <= v.bad < min(per, n), (v, v.bad)
            else:
                assert (S.blocks(n, per) - 1) * per <= v.bad < n, (v, v.bad)
            for plan in (True, False):             # an argument error shows in a plan as well
                s = S.summary_of(v, plan)
                assert s["error"] == S.E_ARG, (v, plan, s)
                assert S.reserved0(s) == (v.bad + 1 if S.names_the_entry(call) else 0), (v, plan, s)
            assert all(len(x) == 0 for x in S.want(v)[:-1] if x is not None), v


@pytest.mark.parametrize("call,B", PARAMS, ids=IDS)
def test_short_variants_lack_capacity(call, B):
    for which in S.SIZES:
        good = S.case(call, which, B=B)
        v = S.variant(good, "short")
        s = S.summary_of(v)
        assert s["error"] == S.E_CAPACITY and v.caps["out_cap"] == good.caps["out_cap"] - 1, (v, s)
        assert S.summary_of(v, plan=True)["error"] == 0
        assert all(len(x) == 0 for x in S.want(v)[:-1] if x is not None), v
        for k in ("nal_count", "stream_bytes"):    # the sizes of the good case are reported all the same
            assert s[k] == S.summary_of(good)[k], (v, k)


def test_the_sequence_is_the_ten_steps():
    for call in S.CALLS:
        steps = S.sequence(call)
        assert [(c.name, plan) for c, plan in steps] == [("large", False), ("small", False), ("large bad-late", False), ("small", False),
                                                          ("small bad-early", False), ("odd", False), ("empty", False), ("large short", False),
                                                          ("large", True), ("large", False)]
        assert steps[0][0] is steps[9][0] is S.case(call, "large") and steps[1][0] is steps[3][0]


def test_the_demux_of_a_mux_case_gives_its_access_units_back():
    for which, lo in (("small", 1), ("large", 3)):
        mux = S.case("tsm", which)
        d = S.demux_of(mux)
        assert d is S.demux_of(mux) and (S.plan_blocks(d)[0] == 1 if which == "small" else S.plan_blocks(d)[0] >= lo)
        out, pes, s = S.want(d)
        au = mux.a["au"]
        assert s["error"] == 0 and len(pes) == len(au) and s["reserved"][1] == 0
        assert out.tobytes() == b"".join(mux.a["stream"][int(b):int(e)].tobytes() for b, e in zip(au["unit_begin"], au["unit_end"]))


def test_cases_are_built_once_and_by_their_seed():
    a, b = S.case("tsd", "small", 1), S.case("tsd", "small", 2)
    assert a is S.case("tsd", "small", 1) and not np.array_equal(a.a["ts"], b.a["ts"])
    assert S.want(a) is S.want(a)
